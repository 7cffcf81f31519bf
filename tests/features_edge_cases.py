"""Edge cases of the discovery features (csrc/rm_features.h, csrc/rm_features.hip), shared by tests/test_features_edges_host.py
(the host build of the header over the CPU oracle) and tests/test_gpu_features_edges.py (the device): seeded NumPy, no fixture.

Nothing here injects SDF values.  `ts` and `seglen` are the caller's arrays, so on Sphere (scene 0) the chord (0, 0, 0) ->
(0, 0, 2) with ts[i] = 0.25 for an inside sample and 0.75 for an outside one produces any sign pattern exactly, the reversed
chord its complement, and with chord_steps = 2 and both samples inside a chord has one run of length exactly 2 * seglen: the
seglen array is the median select's input, value for value.  gmag comes from the scene, so a p99 sample is built by choosing,
ordering and repeating points of a pool whose gmag the NumPy statement over the oracle has computed.

Both suites call the check_* functions below with their own `run`:
  run_intrinsic(scene_id, sets) -> [(fields dict, gmag (n_lip,), slab_counts (n_chords,))] per set
  run_view(captures, cameras)   -> [view dict as _native.view_features gives it] per capture
The conditions the cases rest on (the intended inside flags, the tie and rank structure, which points are left out, both
branches of feat_quantile) are asserted by the check_*_conditions functions over the oracle, without a GPU."""
import functools

import numpy as np

import features_cases as C
from raymarch_algo_compare_amd import features

SPHERE, MANDELBULB, BAD_SPHERE = 0, 10, 11
TS2 = np.array([0.0, 1.0])
NO_PTS, NO_CHORDS, NO_SEGLEN = np.empty((0, 3)), np.empty((0, 6)), np.empty(0)


# ---- 1. run detection ------------------------------------------------------------------------------------------------------

RUN_STEPS = [2, 3, 63, 64, 65, 127, 128, 129, 160, 1023, 1024]
CHORD = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 2.0])               # ts 0.25 -> z = 0.5 (inside), 0.75 -> z = 1.5 (outside)
REVERSED = np.array([0.0, 0.0, 2.0, 0.0, 0.0, 0.0])            # ts 0.25 -> z = 1.5, 0.75 -> z = 0.5: the complement
ALL_IN = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.5])
ALL_OUT = np.array([0.0, 0.0, 2.0, 0.0, 0.0, 3.0])
RUN_SEGLEN = [2.718281828, 1.4142135623730951, 0.5, 1.0]      # one per chord kind: a length mistaken for another's shows


def numpy_runs(inside, seglen):
    """the reference's expressions"""
    inside = np.asarray(inside, bool)
    steps = len(inside)
    if not inside.any():
        return np.empty(0)
    d = np.diff(inside.astype(np.int8))
    starts, ends = np.where(d == 1)[0] + 1, np.where(d == -1)[0] + 1
    if inside[0]:
        starts = np.r_[0, starts]
    if inside[-1]:
        ends = np.r_[ends, steps]
    step_len = seglen / (steps - 1)
    return np.array([(e - s) * step_len for s, e in zip(starts, ends)])


def sign_patterns(steps):
    rng = np.random.default_rng(steps)
    idx = np.arange(steps)
    out = [("all inside", np.ones(steps, bool)), ("none inside", np.zeros(steps, bool)), ("alternating from 0", idx % 2 == 0),
           ("alternating from 1", idx % 2 == 1), ("both ends", (idx < 1) | (idx >= steps - 1)),
           ("both ends wide", (idx < steps // 3) | (idx >= steps - steps // 4)), ("first only", idx == 0), ("last only", idx == steps - 1),
           ("random", rng.random(steps) < 0.5), ("sparse", rng.random(steps) < 0.1), ("dense", rng.random(steps) < 0.9)]
    for edge in (64, 128):
        if steps > edge:
            out += [(f"across {edge - 1}/{edge}", (idx >= edge - 1) & (idx <= edge)), (f"ends at {edge - 1}", (idx >= edge - 3) & (idx < edge)),
                    (f"starts at {edge}", (idx >= edge) & (idx < edge + 2)), (f"long across {edge}", (idx >= 5) & (idx < steps - 2)),
                    (f"one at {edge - 1} one at {edge + 1}", (idx == edge - 1) | (idx == edge + 1))]
    return out


def seam_patterns(steps):
    """at most two runs each, so the median and the count fix every start and every end.  Around the last full seam of the
    chord, and at 1024 steps the last chunk (960 .. 1023) and the last sample"""
    idx = np.arange(steps)
    out = []
    last = 64 * ((steps - 1) // 64)                            # first sample of the last chunk
    if last >= 64:
        out += [(f"across {last - 1}/{last}", (idx >= last - 1) & (idx <= last)), (f"ends at {last - 1}", (idx >= last - 2) & (idx < last)),
                (f"starts at {last}", idx == last), (f"one at {last - 1} one at {last + 1}", (idx == last - 1) | ((idx == last + 1) & (idx < steps))),
                (f"from {last - 1} to the end", idx >= last - 1), ("the last chunk", idx >= last), ("all but the last chunk", idx < last),
                ("sample 63 and the last chunk", (idx == 63) | (idx >= last))]
    if steps == 1024:
        out += [("960 and 1023", (idx == 960) | (idx == 1023)), ("1022/1023", idx >= 1022), ("959/960 and 1023", ((idx >= 959) & (idx <= 960)) | (idx == 1023)),
                ("0 and 1023", (idx == 0) | (idx == 1023)), ("1 .. 1022", (idx >= 1) & (idx <= 1022)), ("63 .. 960", (idx >= 63) & (idx <= 960))]
    assert all(len(numpy_runs(p, 1.0)) <= 2 and len(numpy_runs(~p, 1.0)) <= 3 for _, p in out), steps      # the complement: one more
    return out


def run_ts(inside):
    return np.where(np.asarray(inside, bool), 0.25, 0.75)


def one_chord(chord, seglen, ts):
    return {"pts": NO_PTS, "chords": np.asarray(chord, np.float64).reshape(1, 6), "seglen": np.array([seglen], np.float64), "ts": ts}


@functools.lru_cache(maxsize=None)
def run_cases(steps):
    """[(name, four sets of one chord, the four chords' inside flags)]: the pattern, its complement, all inside, all outside"""
    out = []
    for name, inside in sign_patterns(steps) + seam_patterns(steps):
        ts = run_ts(inside)
        sets = [one_chord(c, s, ts) for c, s in zip((CHORD, REVERSED, ALL_IN, ALL_OUT), RUN_SEGLEN)]
        out.append((name, sets, [inside, ~inside, np.ones(steps, bool), np.zeros(steps, bool)]))
    return out


def expected_runs(inside, seglen):
    """(count, median bits) of one sample of chords: inside (n_chords, steps), seglen (n_chords,)"""
    lengths = [numpy_runs(i, s) for i, s in zip(inside, seglen)]
    counts = np.array([len(x) for x in lengths], np.int32)
    allx = np.concatenate(lengths) if lengths else np.empty(0)
    return counts, (C.bits(np.median(allx))[0] if len(allx) else np.uint64(C.NAN_BITS))


def check_run_conditions(sdf):
    """every run case's ts gives the intended inside flags under the oracle; 512 runs (feat_max_runs) occur at 1023 and 1024"""
    for steps in RUN_STEPS:
        most = 0
        for name, sets, inside in run_cases(steps):
            for s, want in zip(sets, inside):
                a, b = s["chords"][0, :3], s["chords"][0, 3:]
                seg = a[None, :] + s["ts"][:, None] * (b - a)[None, :]
                assert np.array_equal(sdf(SPHERE, seg) < 0.0, want), (steps, name)
                most = max(most, len(numpy_runs(want, 1.0)))
        assert most == (steps + 1) // 2, (steps, most)


def check_runs(run_intrinsic, steps):
    for name, sets, inside in run_cases(steps):
        got = run_intrinsic(SPHERE, sets)
        assert len(got) == 4
        for k, ((res, gmag, counts), flags, seglen) in enumerate(zip(got, inside, RUN_SEGLEN)):
            want_counts, want_median = expected_runs([flags], [seglen])
            label = (steps, name, ("pattern", "complement", "all inside", "all outside")[k])
            assert np.array_equal(np.asarray(counts, np.int32), want_counts), (label, counts, want_counts)
            assert res["n_slabs"] == int(want_counts.sum()), (label, res)
            assert C.bits(res["slab_median"])[0] == want_median, (label, res["slab_median"], want_median.view(np.float64))
            assert res["n_finite"] == 0 and C.bits(res["lipschitz_p99"])[0] == C.NAN_BITS, label


MIXED_STEPS, MIXED_CHORDS, MIXED_SETS = 160, 75, 3


@functools.lru_cache(maxsize=None)
def mixed_batch():
    """(sets, inside (set, chord, steps)): 75 chords a set, the four chord kinds in a seeded random order, every chord with a
    length of its own, so a chord's block read at another chord's offset changes the counts or the median"""
    rng = np.random.default_rng(75)
    inside = rng.random(MIXED_STEPS) < 0.5
    ts = run_ts(inside)
    kinds = [(CHORD, inside), (REVERSED, ~inside), (ALL_IN, np.ones(MIXED_STEPS, bool)), (ALL_OUT, np.zeros(MIXED_STEPS, bool))]
    sets, flags = [], []
    for s in range(MIXED_SETS):
        pick = rng.integers(0, 4, MIXED_CHORDS)
        pick[:4] = rng.permutation(4)                          # every kind occurs
        sets.append({"pts": NO_PTS, "chords": np.stack([kinds[k][0] for k in pick]), "seglen": rng.uniform(0.1, 9.0, MIXED_CHORDS), "ts": ts})
        flags.append(np.stack([kinds[k][1] for k in pick]))
    return sets, flags


def check_mixed_batch(run_intrinsic):
    sets, flags = mixed_batch()
    got = run_intrinsic(SPHERE, sets)
    for i, ((res, gmag, counts), s, f) in enumerate(zip(got, sets, flags)):
        want_counts, want_median = expected_runs(f, s["seglen"])
        assert np.array_equal(np.asarray(counts, np.int32), want_counts), (i, counts, want_counts)
        assert res["n_slabs"] == int(want_counts.sum()) and C.bits(res["slab_median"])[0] == want_median, (i, res)


# ---- 2. the median select -----------------------------------------------------------------------------------------------------

MEDIAN_N = [1, 2, 3, 100, 101, 255, 256, 257, 1500, 4096]


def ulps_above(x, k):
    return (np.float64(x).view(np.uint64) + np.asarray(k, np.uint64)).view(np.float64)


def _tied(rng, n, at):
    """n values whose sorted order holds one tie: s[i] == s[i + 1] for i = `at` (clipped into the sample), all else distinct"""
    s = np.sort(rng.random(n)) + np.arange(n)                  # distinct
    if n >= 2:
        i = min(max(at, 0), n - 2)
        s[i + 1] = s[i]
    return rng.permutation(s)


def median_families(n):
    """[(name, seglen (n,))]: the host test's five sample families and the key-structure families of the radix select"""
    rng = np.random.default_rng(9000 + n)
    j = n // 2 if n % 2 else n // 2 - 1                        # score_rank_med
    fams = [("uniform", rng.random(n) * 3.0), ("quarters", np.round(rng.random(n) * 4.0) / 4.0), ("all equal", np.full(n, 0.75)),
            ("descending", np.sort(rng.random(n))[::-1].copy()), ("zeros and tiny", np.r_[np.zeros(n // 2), rng.random(n - n // 2) * 1e-300]),
            ("last byte only", ulps_above(1.0, rng.integers(0, 256, n))),
            ("top bytes only", np.where(rng.random(n) < 0.1, 0.0, np.ldexp(1.0, rng.integers(-1074, 1023, n)))),
            ("with 1e300", np.r_[rng.random(n - 1), 1e300][rng.permutation(n)]),
            ("tie at j/j+1", _tied(rng, n, j)), ("tie at j-1/j", _tied(rng, n, j - 1)), ("tie at j+1/j+2", _tied(rng, n, j + 1))]
    if n >= 3:
        fams.append(("one +inf above", np.r_[rng.random(n - 1), np.inf][rng.permutation(n)]))
    return fams


@functools.lru_cache(maxsize=None)
def median_case(n, steps=2):
    """(sets, want bits per set, names): every family with all chords inside, then with every third chord outside (its slot is
    kScoreNoKey); steps = 3 puts the one run in the first of two slots"""
    ts = TS2 if steps == 2 else np.linspace(0.0, 1.0, steps)
    sets, want, names = [], [], []
    for name, seglen in median_families(n):
        for thirds in (False, True):
            outside = (np.arange(n) % 3 == 2) if thirds else np.zeros(n, bool)
            chords = np.where(outside[:, None], ALL_OUT[None, :], ALL_IN[None, :])
            sets.append({"pts": NO_PTS, "chords": chords, "seglen": seglen, "ts": ts})
            lengths = (2.0 * seglen if steps == 2 else np.float64(steps) * (seglen / (steps - 1)))[~outside]
            want.append((int((~outside).sum()), C.bits(np.median(lengths))[0] if len(lengths) else np.uint64(C.NAN_BITS)))
            names.append(f"n={n} steps={steps} {name}{' every third outside' if thirds else ''}")
    return sets, want, names


def check_median_conditions():
    for n in MEDIAN_N:
        fams = dict(median_families(n))
        j = n // 2 if n % 2 else n // 2 - 1
        assert all(len(v) == n and not np.isnan(v).any() and not np.signbit(v).any() for v in fams.values()), n
        keys = C.bits(2.0 * fams["last byte only"])
        assert len(np.unique(keys >> np.uint64(8))) == 1 and (n < 100 or len(np.unique(keys)) > 50), n
        top = fams["top bytes only"]
        assert np.all((C.bits(top) & np.uint64((1 << 52) - 1) == 0) | (top < 2.3e-308)), n      # a power of two, or a subnormal one
        if n >= 100:
            assert np.ptp(np.frexp(top[top > 0])[1]) >= 200 and (top == 0).any() and ((top > 0) & (top < 2.2e-308)).any(), n
        if n >= 4:
            for name, at in (("tie at j/j+1", j), ("tie at j-1/j", j - 1), ("tie at j+1/j+2", j + 1)):
                s = np.sort(fams[name])
                assert s[at] == s[at + 1] and len(np.unique(s)) == n - 1, (n, name)
        if n >= 3:
            s = np.sort(fams["one +inf above"])
            assert np.isinf(s[-1]) and np.isfinite(s[j if n % 2 else j + 1]), n      # the ranks the median reads stay finite


def check_median(run_intrinsic, n, steps=2):
    sets, want, names = median_case(n, steps)
    got = run_intrinsic(SPHERE, sets)
    assert len(got) == len(sets)
    for (res, gmag, counts), (count, median), name, s in zip(got, want, names, sets):
        assert res["n_slabs"] == count and int(np.sum(counts)) == count, (name, res)
        assert np.array_equal(np.asarray(counts) == 1, s["chords"][:, 5] == 0.5), name
        assert C.bits(res["slab_median"])[0] == median, (name, res["slab_median"], median.view(np.float64))


# ---- 3. the p99 select --------------------------------------------------------------------------------------------------------

P99_N = [1, 2, 3, 26, 27, 51, 100, 101, 102, 255, 256, 257, 1500, 65536]
P99_SCENES = [SPHERE, BAD_SPHERE, MANDELBULB]
P99_FAMILIES = ("random", "all equal", "tie at j/j+1", "tie ends at j", "descending")
LEFT_OUT_N = [3, 27, 102, 257, 1500]
LEFT_OUT_SCENES = [SPHERE, BAD_SPHERE]      # both overflow at 1e200 on one axis
LEFT_OUT_FAMILIES = ("left out at the start", "left out at the end", "left out at stride 256", "all left out")


def p99_rank(n):
    return int(np.floor((n - 1) * 0.99))


def p99_gamma(n):
    v = (n - 1) * 0.99
    return v - np.floor(v)


def lip_set(pts):
    return {"pts": np.ascontiguousarray(pts, np.float64).reshape(-1, 3), "chords": NO_CHORDS, "seglen": NO_SEGLEN, "ts": TS2}


class Pool:
    """points of one scene with the gmag the NumPy statement gives them over `sdf`; `rank` orders the distinct finite values"""

    def __init__(self, scene, sdf):
        rng = np.random.default_rng(500 + scene)
        base = rng.uniform(-1.3, 1.3, (300, 3))
        if scene == SPHERE:                                    # a coarse lattice of difference quotients from 1e5 on: zeros, ties
            base = np.concatenate([base[:24] * 10.0 ** k for k in range(13)])
        self.scene, self.pts = scene, base
        self.gmag = features.intrinsic_features_numpy(scene, [lip_set(base)], sdf=lambda p: sdf(scene, p))[0]["gmag"]
        assert np.isfinite(self.gmag).all(), scene
        self.values, self.first = np.unique(self.gmag, return_index=True)      # sorted distinct gmag, a pool point of each
        assert len(self.values) >= 40, (scene, len(self.values))
        if scene == SPHERE:
            assert (self.gmag == 0.0).sum() >= 2 and len(self.values) < len(self.gmag), "the lattice has zeros and ties"
        if scene in LEFT_OUT_SCENES:
            bad = rng.uniform(-1.0, 1.0, (8, 3))
            bad[np.arange(8), np.arange(8) % 3] = np.array([1e200, -1e200] * 4)          # |p|^2 overflows: f = inf, inf - inf
            self.bad = bad
            g = features.intrinsic_features_numpy(scene, [lip_set(bad)], sdf=lambda p: sdf(scene, p))[0]["gmag"]
            assert np.isnan(g).all(), (scene, "the left-out points are non-finite under the oracle", g)

    def ranks(self, family, n, rng):
        """n ranks into `values`, in sample order"""
        m, j = len(self.values), p99_rank(n)
        if family == "random":
            return rng.integers(0, m, n)
        if family == "all equal":
            return np.full(n, rng.integers(0, m))
        if family == "descending":
            return np.sort(rng.integers(0, m, n))[::-1]
        v = int(rng.integers(m // 3, 2 * m // 3))              # the tied value: ranks below and above it exist
        if family == "tie at j/j+1":                           # s[j - 1] < s[j] == s[j + 1] < s[j + 2]
            if j + 1 > n - 1:
                return None
            r = np.r_[rng.integers(0, v, j), v, v, rng.integers(v + 1, m, n - j - 2)]
        else:                                                  # s[j - 2] < s[j - 1] == s[j] < s[j + 1]
            if j < 1 or j + 1 > n - 1:
                return None
            r = np.r_[rng.integers(0, v, j - 1), v, v, rng.integers(v + 1, m, n - j - 1)]
        return rng.permutation(r)


@functools.lru_cache(maxsize=None)
def _pool(scene, sdf):
    return Pool(scene, sdf)


def p99_case(scene, n, sdf):
    """(sets, want gmag per set, names) of one call: every family that n admits.  At 65536 two sets only."""
    pool, rng = _pool(scene, sdf), np.random.default_rng(7000 * scene + n)
    sets, want, names = [], [], []
    for fam in (P99_FAMILIES if n < 65536 else ("random", "tie at j/j+1")):
        r = pool.ranks(fam, n, rng)
        if r is None:
            continue
        idx = pool.first[r]
        sets.append(lip_set(pool.pts[idx]))
        want.append(pool.gmag[idx])
        names.append(f"scene {scene} n={n} {fam}")
    return sets, want, names


def left_out_case(scene, n, sdf):
    """(sets, want gmag per set (NaN = left out), names)"""
    pool, rng = _pool(scene, sdf), np.random.default_rng(8000 * scene + n)
    sets, want, names = [], [], []
    for fam in LEFT_OUT_FAMILIES:
        out = np.zeros(n, bool)
        if fam == "left out at the start":
            out[:max(1, n // 10)] = True
        elif fam == "left out at the end":
            out[n - max(1, n // 10):] = True
        elif fam == "left out at stride 256":
            out[::256] = True
        else:
            out[:] = True
        idx = pool.first[rng.integers(0, len(pool.values), n)]
        pts, g = pool.pts[idx].copy(), pool.gmag[idx].copy()
        pts[out], g[out] = pool.bad[rng.integers(0, len(pool.bad), int(out.sum()))], np.nan
        sets.append(lip_set(pts))
        want.append(g)
        names.append(f"scene {scene} n={n} {fam}")
    return sets, want, names


def check_p99_conditions(sdf):
    """each family has the structure its name claims (the sorted oracle gmag at j - 1, j, j + 1), occurs at an n of either
    branch of feat_quantile, and no more than the intended points are left out"""
    for scene in P99_SCENES:
        branches = {f: set() for f in P99_FAMILIES}
        for n in P99_N:
            j = p99_rank(n)
            sets, want, names = p99_case(scene, n, sdf)
            for s, g, name in zip(sets, want, names):
                fam = name.split(f"n={n} ")[1]
                branches[fam].add(bool(p99_gamma(n) < 0.5))
                srt = np.sort(g)
                assert len(g) == n and np.isfinite(g).all(), name
                if fam == "all equal":
                    assert srt[0] == srt[-1], name
                elif fam == "tie at j/j+1":
                    assert srt[j] == srt[j + 1] and (j == 0 or srt[j - 1] < srt[j]) and (j + 2 >= n or srt[j + 1] < srt[j + 2]), name
                elif fam == "tie ends at j":
                    assert srt[j - 1] == srt[j] < srt[j + 1], name
                elif fam == "descending":
                    assert np.all(np.diff(g) <= 0), name
        assert all(b == {True, False} for b in branches.values()), (scene, branches)
    for scene in LEFT_OUT_SCENES:
        branches = {f: set() for f in LEFT_OUT_FAMILIES[:3]}
        for n in LEFT_OUT_N:
            for s, g, name in zip(*left_out_case(scene, n, sdf)):
                if int(np.isfinite(g).sum()):
                    branches[name.split(f"n={n} ")[1]].add(bool(p99_gamma(int(np.isfinite(g).sum())) < 0.5))
                live = features.intrinsic_features_numpy(scene, [s], sdf=lambda p: sdf(scene, p))[0]["gmag"]
                assert np.array_equal(np.isnan(live), np.isnan(g)) and np.isnan(g).any(), name
                assert ("stride" not in name) or np.array_equal(np.flatnonzero(np.isnan(g)), np.arange(0, n, 256)), name
        assert all(b == {True, False} for b in branches.values()), (scene, branches)


def check_lip_sets(run_intrinsic, scene, case):
    sets, want, names = case
    got = run_intrinsic(scene, sets)
    assert len(got) == len(sets)
    for (res, gmag, counts), g, name in zip(got, want, names):
        finite = g[np.isfinite(g)]
        assert np.array_equal(C.bits(gmag), C.bits(np.where(np.isfinite(g), g, np.nan))), (name, "gmag", int((C.bits(gmag) != C.bits(g)).sum()))
        assert np.all(C.bits(gmag)[~np.isfinite(g)] == C.NAN_BITS), name
        assert res["n_finite"] == len(finite), (name, res["n_finite"], len(finite))
        want_p99 = C.bits(np.percentile(finite, 99))[0] if len(finite) else np.uint64(C.NAN_BITS)
        assert C.bits(res["lipschitz_p99"])[0] == want_p99, (name, res["lipschitz_p99"], want_p99.view(np.float64))
        assert res["n_slabs"] == 0 and C.bits(res["slab_median"])[0] == C.NAN_BITS, name


# ---- 4. the view features -------------------------------------------------------------------------------------------------------

VIEW_SHAPES = [(31, 7), (32, 8), (33, 9), (64, 16), (65, 17), (1, 9), (9, 1)]      # (W, H); tiles are 32 x 8
EVALS_MAX = float(1 << 24)


def _single(w, h, *pixels):
    m = np.zeros((h, w), bool)
    for x, y in pixels:
        m[y, x] = True
    return m


def view_mask_cases(w, h):
    """[(label, capture, camera)]: features_cases.masks, one hit at each corner, and on 64 x 16 one hit on each side of the
    tile seams"""
    ms = list(C.masks(w, h)) + [(f"corner {x},{y}", _single(w, h, (x, y))) for x, y in sorted({(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)})]
    if (w, h) == (64, 16):
        ms += [(f"seam {x},{y}", _single(w, h, (x, y))) for x, y in ((31, 7), (32, 7), (31, 8), (32, 8))]
        ms.append(("the four seam pixels", _single(w, h, (31, 7), (32, 7), (31, 8), (32, 8))))
    return [(f"{w}x{h} {name}", C.capture_of(mask, 3000 * w + 7 * h + i), C.camera(w, h)) for i, (name, mask) in enumerate(ms)]


def _full(w, h, seed):
    return C.capture_of(np.ones((h, w), bool), seed)


def view_value_cases():
    """[(label, capture, camera, expected dict of exact values or None)]: evals, normals, depths off the ordinary"""
    from raymarch_algo_compare_amd.runner import ray_directions
    out = []
    w, h = 65, 17
    cam = C.camera(w, h)
    cap = _full(w, h, 11)
    cap["evals"][:] = 37.0
    out.append(("evals all equal", cap, cam, {"sum_evals": 37 * w * h, "hardness_mean": 37.0, "hardness_cv": 0.0}))
    cap = _full(w, h, 12)
    cap["evals"][:] = 0.0
    out.append(("evals all 0", cap, cam, {"sum_evals": 0, "hardness_mean": 0.0, "hardness_cv": 0.0}))
    cap = _full(w, h, 13)
    cap["evals"][:] = EVALS_MAX
    out.append(("evals all 2^24", cap, cam, {"sum_evals": (1 << 24) * w * h, "hardness_mean": EVALS_MAX, "hardness_cv": 0.0}))
    # evals outside the domain of counts, on hits: NaN and -1 are 0, 2.5 is 2, +inf and 3e38 are 2^24
    for name, v, count in (("NaN", np.nan, 0), ("-1", -1.0, 0), ("2.5", 2.5, 2), ("+inf", np.inf, 1 << 24), ("3e38", 3e38, 1 << 24),
                           ("2^24 + 2", EVALS_MAX + 2.0, 1 << 24), ("-inf", -np.inf, 0), ("-0.0", -0.0, 0)):
        cap = _full(33, 9, 14)
        cap["evals"][:] = 5.0
        cap["evals"][0, 0] = cap["evals"][8, 32] = cap["evals"][4, 17] = v
        out.append((f"evals {name} on three hits", cap, C.camera(33, 9), {"sum_evals": 5 * (33 * 9 - 3) + 3 * count}))
    cap = _full(33, 9, 15)
    cap["hit"][2, 3] = False
    cap["evals"][2, 3] = np.nan                                # off the mask: never read as a count
    out.append(("evals NaN on a non-hit", cap, C.camera(33, 9), {"sum_evals": int(cap["evals"][cap["hit"]].sum())}))
    # normals: a NaN normal is not grazing; |cosine| a relative 1e-5 below 0.20 is, the same above is not
    cam = C.camera(33, 9)
    rd = ray_directions(cam)
    for name, scale, grazing in (("NaN normal", np.nan, 0), ("cosine just below 0.20", 0.20 * (1 - 1e-5), 33 * 9), ("cosine just above 0.20", 0.20 * (1 + 1e-5), 0),
                                 ("cosine just above -0.20", -0.20 * (1 - 1e-5), 33 * 9), ("cosine just below -0.20", -0.20 * (1 + 1e-5), 0)):
        cap = _full(33, 9, 16)
        cap["normal"] = (rd * scale).astype(np.float32)        # |rd| = 1: the cosine is `scale` to a few 1e-8
        out.append((name, cap, cam, {"n_grazing": grazing}))
    cap = _full(33, 9, 17)
    cap["normal"][3, 5] = np.nan
    out.append(("one NaN normal", cap, cam, None))
    return out


def view_depth_cases():
    """[(label, capture, camera, the axes that are NaN)]: a non-finite depth on a hit of a 65 x 17 all-hit frame (tile 0 is
    x < 32, y < 8: lane = 32 * y + x), and on a non-hit"""
    w, h = 65, 17
    out = []
    for name, (x, y), v in (("NaN depth at lane 0", (0, 0), np.nan), ("NaN depth at lane 255", (31, 7), np.nan), ("NaN depth at lane 128", (0, 4), np.nan),
                            ("NaN depth in the second tile", (40, 3), np.nan), ("NaN depth in the last tile", (64, 16), np.nan),
                            ("+inf depth on a hit", (10, 5), np.inf), ("-inf depth on a hit", (50, 12), -np.inf)):
        cap = _full(w, h, 21)
        cap["depth"][y, x] = v
        out.append((name, cap, C.camera(w, h), np.isnan(v)))
    cap = _full(w, h, 22)
    cap["hit"][0, 0] = False
    cap["depth"][0, 0] = np.nan
    out.append(("NaN depth on a non-hit", cap, C.camera(w, h), False))
    cap = C.capture_of(_single(w, h, (40, 3)), 23)
    cap["depth"][3, 40] = np.nan
    out.append(("NaN depth on the only hit", cap, C.camera(w, h), True))
    return out


def check_view_against_numpy(got, want, label):
    """features_cases.check_view_against_numpy, with a box corner that is not finite in NumPy's answer equal to it exactly"""
    finite = np.isfinite(want["box_lo"]) & np.isfinite(want["box_hi"])
    if want["n_hit"] and not finite.all():
        for k in ("box_lo", "box_hi"):
            bad = ~np.isfinite(want[k])
            assert np.array_equal(C.bits(got[k])[bad], C.bits(np.where(np.isnan(want[k]), np.nan, want[k]))[bad]), (label, k, got[k], want[k])
            got, want = dict(got), dict(want)
            got[k], want[k] = np.where(bad, 0.0, got[k]), np.where(bad, 0.0, want[k])
    C.check_view_against_numpy(got, want, label)


def many_views(n, w=9, h=3):
    """n distinct captures of one size with their cameras"""
    yy, xx = np.mgrid[0:h, 0:w]
    caps = [C.capture_of((xx * 7 + yy * 3 + v) % 5 != 0 if v % 4 else (xx + yy + v) % 2 == 0, 40000 + v) for v in range(n)]
    from raymarch_algo_compare_amd.camera import Camera
    cams = [Camera((0.3 + 0.01 * v, 0.4, 5.0 - 0.005 * v), (0.0, 0.1, 0.0), (0.0, 1.0, 0.0), 60.0, w, h) for v in range(n)]
    return caps, cams


def check_views(run_view, host, cases, expect_nan=None):
    """one batch of (label, capture, camera[, exact values | NaN flag]) rows of one frame size: bit for bit the host build,
    and NumPy by check_view_against_numpy's rule"""
    got = run_view([c[1] for c in cases], [c[2] for c in cases])
    assert len(got) == len(cases)
    for row, r in zip(cases, got):
        label, cap, cam = row[:3]
        C.same_view(r, host.view(cap, cam.params14()), label)
        with np.errstate(all="ignore"):
            want = features.view_features_numpy(cap, cam)
        check_view_against_numpy(r, want, label)
        if len(row) > 3 and isinstance(row[3], dict):
            for k, v in row[3].items():
                assert r[k] == v, (label, k, r[k], v)
        elif len(row) > 3 and row[3] is not None:
            nan = np.isnan(r["box_lo"])
            assert np.array_equal(nan, np.isnan(r["box_hi"])) and nan.all() == bool(row[3]) and nan.any() == bool(row[3]), (label, r)
            assert np.all(C.bits(r["box_lo"])[nan] == C.NAN_BITS) and np.all(C.bits(r["box_hi"])[nan] == C.NAN_BITS), label
