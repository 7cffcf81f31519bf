#!/usr/bin/env python3
"""The N > 1 frame gather on ONE GPU: the child process of tests/test_gpu_loopback_gather.py.

librm_hip.so is started with RM_RCCL_LIBRARY naming the loop-back stand-in (tests/native/rccl_loopback.cpp), and this
one process plays every rank in turn: rm_comm_init(id, N, r) .. rm_comm_destroy() per rank, the stand-in keeping what
was sent in between.  What is checked is the library's own decision of WHAT is sent, HOW MANY bytes, and WHERE it lands
(rm_gather_frame, rm_gather_frame_root in csrc/rm_gather.hip): every gathered frame must equal the unsharded render bit
for bit, four poisoned rows behind the frame must stay poisoned, and the stand-in's call and byte counts must be the
plan's.  A fresh process because the library caches the RCCL handle; no torch (its wheel maps a second HIP runtime).

usage: RM_RCCL_LIBRARY=<stand-in> loopback_gather_check.py <group>      group: cyclic | contiguous | reuse

The cases (scene, W, H, N; the plan is asserted against sharding.plan_rows and rm_shard_rows before it is relied on):
  cyclic      64 x 16 / 2, 4   smallest band-cyclic frame; rows of 16 n bytes: the 16-byte form of the placement kernel
              67 x 24 / 2, 3   hit rows of 67 B (byte form), depth / iters rows of 268 B (no multiple of 16)
              200 x 96 / 8     eight ranks, three bands each
  contiguous  333 x 50 / 3     per = 20, last = 10: padded short shard; hit slots at 6660 r bytes, unaligned
              64 x 8 / 4       per = 4: ranks 2 and 3 empty
              4 x 20 / 8       per = 4: ranks 5 - 7 empty; one 16-byte depth row
              100 x 37 / 2     per = 20, last = 17: H no multiple of 4
              1 x 9 / 2        per = 8, last = 1: one-pixel rows
  reuse       landing buffers across frames of changing size on a communicator that stays open (64 x 12, 333 x 58,
              333 x 50, 67 x 24, 64 x 12 on 3 ranks), then the two negative checks (a receive nobody sent for, a send of another size:
              both RM_E_RCCL, never a hang), each followed by a positive case in the same process.
Roots of the gather-to-root form: 0, N - 1 and N // 2."""
import contextlib
import ctypes
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from loopback_stub import declare                                          # noqa: E402
from raymarch_algo_compare_amd import _native, registry, sharding          # noqa: E402
from raymarch_algo_compare_amd.camera import Camera                        # noqa: E402

vp = ctypes.c_void_p
EB = (4, 4, 1)                       # bytes per pixel of depth, iters, hit
MAPS = ("depth", "iters", "hit")
POISON, TAIL = 0xA5, 4
RM_E_RCCL = -7
SPHERE, CUBE, MANDELBULB = 0, 2, 10

# (scene, W, H, N, cyclic, rows every rank contributes, rows of the last rank)
CASES = {
    "cyclic": [(SPHERE, 64, 16, 2, True, 8, 8), (CUBE, 64, 16, 4, True, 4, 4), (MANDELBULB, 64, 16, 4, True, 4, 4),
               (CUBE, 67, 24, 2, True, 12, 12), (SPHERE, 67, 24, 3, True, 8, 8), (SPHERE, 200, 96, 8, True, 12, 12)],
    "contiguous": [(CUBE, 333, 50, 3, False, 20, 10), (SPHERE, 64, 8, 4, False, 4, 0), (CUBE, 4, 20, 8, False, 4, 0),
                   (SPHERE, 100, 37, 2, False, 20, 17), (CUBE, 1, 9, 2, False, 8, 1)],
}
# small, large, small.  The frame of 58 rows comes before the large one to leave 18 rows of an earlier frame in the pad
# buffer of rank 2, whose next short shard has 10: what it sends must still end in zeros.  The gather-to-root form uses the
# landing buffers for band-cyclic frames only, so a last, smaller band-cyclic frame follows the 67 x 24 one: there too a
# small frame lands in a buffer a larger one has left.
REUSE = [(SPHERE, 64, 12, 3, True, 4, 4), (CUBE, 333, 58, 3, False, 20, 18), (CUBE, 333, 50, 3, False, 20, 10), (SPHERE, 67, 24, 3, True, 8, 8),
         (CUBE, 64, 12, 3, True, 4, 4)]


class Mismatch(Exception):
    pass


L = S = None
IDENT = ctypes.create_string_buffer(128)


def cam(sid, w, h):
    sc = registry.SCENES[sid]
    return Camera(sc.camera_position or (0.0, 0.0, 5.0), sc.camera_target or (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 60.0, w, h).params14()


def alloc(w, rows):
    p = [vp(), vp(), vp()]
    _native.check(L.rm_alloc_frame(w, rows, *[ctypes.byref(q) for q in p]))
    return p


def fill(p, w, rows, byte=POISON):
    for k in range(3):
        e = S.lb_fill(p[k], w * rows * EB[k], byte)
        if e:
            raise RuntimeError(f"hipMemset failed with HIP error {e}")


def counts():
    c = (ctypes.c_ulonglong * 6)()
    S.lb_counts(c)
    return [int(v) for v in c]


def reason():
    return S.lb_last_reason().decode("utf-8", "replace")


@contextlib.contextmanager
def as_rank(n, r):
    """This process is rank r of n until the block ends."""
    _native.check(L.rm_comm_init(IDENT.raw, n, r))
    try:
        yield
        _native.check(L.rm_stream_synchronize(None))
    finally:
        _native.check(L.rm_comm_destroy())


class Frame:
    """One case: the expectation, every rank's rendered shard on the device, one poisoned full-frame buffer."""

    def __init__(self, case):
        self.sid, self.W, self.H, self.N, cyclic, per, last = case
        self.name = f"{registry.SCENES[self.sid].name} {self.W}x{self.H} / {self.N}"
        W, H, N = self.W, self.H, self.N
        self.plans = [sharding.plan_rows(H, N, r) for r in range(N)]
        got = (self.plans[0].cyclic, self.plans[0].rows if cyclic else L.rm_shard_rows(H, N), self.plans[-1].rows)
        if got != (cyclic, per, last) or sum(p.rows for p in self.plans) != H:
            raise Mismatch(f"{self.name}: the plan is (cyclic, per, last) = {got}, the case table says {(cyclic, per, last)}")
        self.per = per
        c = cam(self.sid, W, H)
        self.ref = _native.render(_native.make_desc(self.sid, 0, c, W, H))
        self.descs = [_native.make_desc(self.sid, 0, c, W, H, **p.desc_kwargs()) for p in self.plans]
        self.shards = [alloc(W, max(p.rows, 1)) for p in self.plans]
        for d, s, p in zip(self.descs, self.shards, self.plans):
            fill(s, W, max(p.rows, 1), 0x5A)
            _native.check(L.rm_render_device(ctypes.byref(d), s[0], s[1], s[2], None, None))
        _native.check(L.rm_stream_synchronize(None))
        self.full = alloc(W, H + TAIL)

    def rows(self, r):
        return self.plans[r].rows

    def roots(self):
        return sorted({0, self.N // 2, self.N - 1})

    def poison(self):
        fill(self.full, self.W, self.H + TAIL)

    def gather(self, r):
        s, f = self.shards[r], self.full
        return L.rm_gather_frame(ctypes.byref(self.descs[r]), s[0], s[1], s[2], f[0], f[1], f[2], None)

    def gather_root(self, r, root, desc=None):
        s, f = self.shards[r], self.full if r == root else [None] * 3
        return L.rm_gather_frame_root(ctypes.byref(desc or self.descs[r]), s[0], s[1], s[2], f[0], f[1], f[2], root, None)

    def check(self, what):
        """The full-frame buffer: rows [0, H) the unsharded render bit for bit, the TAIL rows behind them still poison."""
        W, H = self.W, self.H
        _native.check(L.rm_stream_synchronize(None))
        got = {"depth": np.empty((H + TAIL, W), np.float32), "iters": np.empty((H + TAIL, W), np.int32), "hit": np.empty((H + TAIL, W), np.uint8)}
        _native.check(L.rm_copy_frame_to_host(W, H + TAIL, self.full[0], self.full[1], self.full[2], *[got[m].ctypes.data_as(vp) for m in MAPS]))
        for m in MAPS:
            bits = np.uint8 if m == "hit" else np.uint32
            bad = np.argwhere(got[m][:H].view(bits) != self.ref[m].view(bits))
            if len(bad):
                y, x = (int(v) for v in bad[0])
                raise Mismatch(f"{self.name}, {what}: {m} differs at {len(bad)} pixels, first at (row {y}, column {x}): "
                               f"{got[m][y, x]!r} instead of {self.ref[m][y, x]!r}")
            tail = np.argwhere(got[m][H:].view(np.uint8) != POISON)
            if len(tail):
                y, x = (int(v) for v in tail[0])
                raise Mismatch(f"{self.name}, {what}: {m} was written past the frame, first at (row {H + y}, byte {x})")

    def check_sent(self, r, epoch=0):
        """What rank r handed to each of the three all-gathers: per * W * {4, 4, 1} bytes -- its shard (the rows of its
        bands on a cyclic plan) and, where a contiguous shard is short, zeros behind it."""
        rows, image_rows = self.plans[r].rows, self.plans[r].image_rows()
        for k, m in enumerate(MAPS):
            n = self.per * self.W * EB[k]
            got = np.empty(n + 1, np.uint8)          # room for one byte more: a larger deposit is reported, not cut
            size = S.lb_peek(epoch, k, r, got.ctypes.data_as(vp), n + 1)
            expect(size == n, f"{self.name}: rank {r} handed {size} bytes to all-gather {k} ({m}), not {n}")
            got = got[:n]
            want = np.zeros(n, np.uint8)
            want[:rows * self.W * EB[k]] = np.ascontiguousarray(self.ref[m][image_rows]).view(np.uint8).ravel()
            bad = np.flatnonzero(got != want)
            expect(not len(bad), f"{self.name}: the {m} rows rank {r} sent differ from its shard padded with zeros, first at byte "
                   f"{bad[0] if len(bad) else 0} ({'in the pad' if len(bad) and bad[0] >= rows * self.W * EB[k] else 'in the shard'})")

    def free(self):
        for p in self.shards + [self.full]:
            _native.check(L.rm_free_frame(*p))


WHERE = ""                           # what was going on when an rm_* call failed (main)


def at(what):
    global WHERE
    WHERE = what


def expect(cond, msg):
    if not cond:
        raise Mismatch(msg)


def all_gather_form(fr):
    """Pass 1 deposits every rank's shard (frames incomplete, not checked); in pass 2 EVERY rank's frame is complete."""
    S.lb_reset()
    one = 9 * fr.per * fr.W
    for turn in (1, 2):
        for r in range(fr.N):
            before = counts()
            at(f"{fr.name}, all-gather, pass {turn}, rank {r}")
            with as_rank(fr.N, r):
                fr.poison()
                _native.check(fr.gather(r))
                if turn == 2:
                    fr.check(f"all-gather, rank {r}")
                    fr.check_sent(r)
            c = counts()
            expect(c[4] - before[4] == 3 and c[5] - before[5] == one and c[:4] == [0] * 4,
                   f"{fr.name}, all-gather, rank {r}: counts {before} -> {c}, not 3 all-gathers of {one} bytes in all")
    expect(counts()[4:] == [6 * fr.N, 2 * fr.N * one], f"{fr.name}, all-gather: counts {counts()}")


def root_form(fr, root):
    """Every other rank in turn, then the root: its frame is whole, nothing stays parked, the counts are the plan's."""
    S.lb_reset()
    for r in range(fr.N):
        if r != root:
            at(f"{fr.name}, gather to root {root}, rank {r} sends")
            with as_rank(fr.N, r):
                _native.check(fr.gather_root(r, root))
    at(f"{fr.name}, gather to root {root}, the root receives")
    senders = sum(1 for r in range(fr.N) if r != root and fr.rows(r) > 0)
    nbytes = 9 * fr.W * (fr.H - fr.rows(root))
    expect(counts()[:2] == [3 * senders, nbytes] and S.lb_pending() == 3 * senders, f"{fr.name}, root {root}: after the sends, counts {counts()}, "
           f"{S.lb_pending()} parked; {3 * senders} sends of {nbytes} bytes in all expected")
    with as_rank(fr.N, root):
        fr.poison()
        _native.check(fr.gather_root(root, root))
        fr.check(f"gather to root {root}")
    expect(S.lb_pending() == 0, f"{fr.name}, root {root}: {S.lb_pending()} sends were never received")
    expect(counts() == [3 * senders, nbytes, 3 * senders, nbytes, 0, 0], f"{fr.name}, root {root}: counts {counts()}, "
           f"{3 * senders} sends and receives of {nbytes} bytes in all expected")


def run_case(case):
    t0 = time.perf_counter()
    fr = Frame(case)
    try:
        all_gather_form(fr)
        for root in fr.roots():
            root_form(fr, root)
    finally:
        fr.free()
    print(f"ok  {fr.name}: all-gather on {fr.N} ranks, roots {fr.roots()}  ({time.perf_counter() - t0:.2f} s)", flush=True)


def reuse():
    """R.gather / R.pad across frames of changing size: one communicator stays open for five frames (small band-cyclic,
    two contiguous with a short last shard, the second shorter, a larger and a small band-cyclic); the other ranks' shards are in the stand-in beforehand."""
    at("landing-buffer reuse")
    frames = [Frame(c) for c in REUSE]
    n, keep = 3, 2                                   # the rank that stays open holds the short shard of the middle frame
    try:
        S.lb_reset()
        for r in range(n):
            if r != keep:
                with as_rank(n, r):
                    for fr in frames:                # parked in frame order
                        _native.check(fr.gather_root(r, keep))
        with as_rank(n, keep):
            for fr in frames:
                at(f"landing-buffer reuse, {fr.name}, gather to root {keep}")
                fr.poison()
                _native.check(fr.gather_root(keep, keep))
                fr.check(f"landing-buffer reuse, gather to root {keep}")
        expect(S.lb_pending() == 0, f"landing-buffer reuse: {S.lb_pending()} sends were never received")
        S.lb_reset()
        for e, fr in enumerate(frames):              # the mailboxes of frame e
            S.lb_epoch(e)
            for r in range(n):
                if r != keep:
                    with as_rank(n, r):
                        _native.check(fr.gather(r))
        with as_rank(n, keep):
            for e, fr in enumerate(frames):
                S.lb_epoch(e)
                at(f"landing-buffer reuse, {fr.name}, all-gather on rank {keep}")
                fr.poison()
                _native.check(fr.gather(keep))
                fr.check(f"landing-buffer reuse, all-gather on rank {keep}")
                fr.check_sent(keep, e)
    finally:
        for fr in frames:
            fr.free()
    print("ok  landing-buffer reuse: " + ", ".join(fr.name for fr in frames), flush=True)


def refused(rc, what, *needles):
    """A deliberately wrong TEST-side sequence: the library must answer RM_E_RCCL (from the stand-in, at once)."""
    why, err = reason(), L.rm_last_error().decode("utf-8", "replace")
    expect(rc == RM_E_RCCL, f"{what}: returned {rc} ({err}), not RM_E_RCCL")
    expect(all(s in why for s in needles), f"{what}: the stand-in's reason {why!r} lacks {needles}")
    print(f"ok  {what}: RM_E_RCCL, {why}", flush=True)


def negatives():
    at("negative checks")
    # the root gathers before rank 2 has sent: real RCCL would wait for ever
    fr = Frame((SPHERE, 64, 16, 4, True, 4, 4))
    try:
        S.lb_reset()
        for r in (1, 3):
            with as_rank(4, r):
                _native.check(fr.gather_root(r, 0))
        _native.check(L.rm_comm_init(IDENT.raw, 4, 0))
        try:
            rc = fr.gather_root(0, 0)
        finally:
            _native.check(L.rm_comm_destroy())
        refused(rc, "root gather before rank 2 has sent", "peer 2", "sent nothing")
        S.lb_reset()
        root_form(fr, 0)                             # the same case, now in order: green in the same process
    finally:
        fr.free()
    # rank 1 sends its shard of a frame of 33 rows (13 rows), the root expects that of 37 rows (17 rows)
    fr = Frame((SPHERE, 100, 37, 2, False, 20, 17))
    try:
        S.lb_reset()
        short = sharding.plan_rows(33, 2, 1)
        expect((short.row0, short.rows) == (20, 13), f"plan of 33 rows on 2 ranks: {short}")
        with as_rank(2, 1):
            _native.check(fr.gather_root(1, 0, _native.make_desc(SPHERE, 0, cam(SPHERE, 100, 33), 100, 33, **short.desc_kwargs())))
        _native.check(L.rm_comm_init(IDENT.raw, 2, 0))
        try:
            rc = fr.gather_root(0, 0)
        finally:
            _native.check(L.rm_comm_destroy())
        refused(rc, "a shard of another height than the root expects", "count")
        S.lb_reset()
        root_form(fr, 0)
        all_gather_form(fr)
    finally:
        fr.free()


def main():
    global L, S
    t0 = time.perf_counter()
    group = sys.argv[1]
    stub = os.environ.get("RM_RCCL_LIBRARY")
    if not stub:
        print("RM_RCCL_LIBRARY is not set: this check must never reach a real RCCL")
        return 2
    info = _native.runtime_info()
    if info["hip_runtimes_loaded"] != 1:
        print(f"{info['hip_runtimes_loaded']} HIP runtimes are mapped ({info['hip_runtime_path']}, {info['other_runtime_path']}): stream handles would not be shared")
        return 2
    L = _native.init(0)
    _native.check(L.rm_comm_unique_id(IDENT))         # loads the stand-in, RTLD_LOCAL ...
    S = declare(ctypes.CDLL(stub))                    # ... and this is the same object: its state is the library's
    info = _native.runtime_info()
    if info["hip_runtimes_loaded"] != 1 or not any(IDENT.raw):
        print(f"after loading {stub}: {info['hip_runtimes_loaded']} HIP runtimes mapped, id {IDENT.raw[:8]!r}")
        return 2
    try:
        if group == "reuse":
            reuse()
            negatives()
        else:
            for case in CASES[group]:
                run_case(case)
    except Mismatch as e:
        print(f"LOOPBACK_MISMATCH {e}\n  stand-in: {reason()!r}", flush=True)
        return 1
    except _native.RmError as e:                      # an rm_* call that had to succeed: where, and what the stand-in refused
        print(f"LOOPBACK_ERROR {WHERE}: {e}\n  stand-in: {reason()!r}", flush=True)
        return 1
    print(f"LOOPBACK_OK {group} in {time.perf_counter() - t0:.2f} s", flush=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
