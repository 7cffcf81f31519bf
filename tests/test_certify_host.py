"""The certified first hit without a GPU: csrc/rm_certify.h compiled for the host by g++ (tests/native/certify_check.cpp)
against the exact caster's host build on the eleven frames with an exact form, against the pointwise interpreter on every
catalogue program, twin and fixture tree, against the host interval oracle on Pillar Forest and Hollow Cube, on constructed
rays, and the host-only behaviour of the C ABI, of certified_oracle.py and of the sweep's cert_* columns."""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from conftest import ROOT
import certify_cases as cc
import exact_cases as ec
from certify_cases import HIT, MISS, OPEN

from raymarch_algo_compare_amd import _native, certified_oracle, scoring, sweep
from raymarch_algo_compare_amd import scene_program as sp

dp = ctypes.POINTER(ctypes.c_double)
INF = float("inf")


def counts(status):
    return [int((status == s).sum()) for s in (MISS, HIT, OPEN)]


# ---- 1. the eleven frames with an exact form ---------------------------------------------------------------------------------

@pytest.mark.parametrize("sid", ec.EXACT_IDS, ids=[ec.NAMES[s] for s in ec.EXACT_IDS])
def test_bracket_holds_the_exact_first_hit(sid):
    """MISS implies an exact miss, a finite t_hi an exact hit, and every exact-hit pixel has t_lo - s <= t_exact <= t_hi + s.
    Measured with s = 0 on the host builds of rm_certify.h and rm_exact.h: the largest violation over the eleven frames is 0
    (certify_cases.BRACKET_SLACK_MEASURED), so s = 4 x 0 = 0 and the bracket is asserted as it stands.  OPEN pixels lie in
    the k = 2 silhouette band of the exact mask only, and are at most 0.5 % of the exact-hit pixels (measured: 0 OPEN pixels
    on each of the eleven frames)."""
    key = cc.exact_key(sid)
    f, ex = cc.host_frame(key), ec.host_frame(sid)
    st, e_hit, t_e = f["status"], ex["hit"], ex["depth"]
    s = 4.0 * cc.BRACKET_SLACK_MEASURED
    viol = np.maximum(np.maximum(f["t_lo"] - t_e, t_e - f["t_hi"]), 0.0)[e_hit & (st != MISS)]
    n_open_hit = int(((st == OPEN) & e_hit).sum())
    print(f"{ec.NAMES[sid]}: MISS / HIT / OPEN {counts(st)}, exact hits {int(e_hit.sum())}, OPEN on exact hits {n_open_hit}, "
          f"largest violation of the bracket with s = 0: {viol.max() if viol.size else 0.0:.3e}, steps median "
          f"{np.median(f['steps'][st == HIT]):.0f} max {int(f['steps'].max())}")
    assert not ((st == MISS) & e_hit).any(), "a MISS on an exact hit"
    assert not (np.isfinite(f["t_hi"]) & ~e_hit).any(), "a witness on an exact miss"
    assert np.all(f["t_lo"][e_hit] - s <= t_e[e_hit]), float((f["t_lo"] - t_e)[e_hit].max())
    assert np.all(t_e[e_hit] <= f["t_hi"][e_hit] + s), float((t_e - f["t_hi"])[e_hit].max())
    band = scoring.silhouette_band(e_hit, k=2)
    assert not ((st == OPEN) & ~band).any(), "an OPEN pixel outside the silhouette band"
    assert n_open_hit <= 0.005 * e_hit.sum()


# ---- 2. every catalogue program, twin and fixture tree against the pointwise interpreter -------------------------------------

def check_sound(expr, o, d, t_lo, t_hi, status, t_max, what):
    """program_eval at 2048 evenly spaced points of [0, min(t_lo, t_max)) is >= -1e-12 (test_never_past_a_surface's bound);
    at a finite t_hi it is <= 1e-12 (1 + |t_hi|); a HIT's bracket keeps the width rule"""
    K = 2048
    s = np.arange(K) / K
    end = np.minimum(t_lo, t_max)
    some = end > 0.0                                       # [0, 0) is empty: an eye in the solid has nothing before it
    worst = INF
    for a in range(0, len(d), 1024):
        sel = slice(a, min(a + 1024, len(d)))
        pts = o[sel][some[sel], None, :] + (end[sel][some[sel], None] * s[None, :])[..., None] * d[sel][some[sel], None, :]
        if pts.size:
            worst = min(worst, float(ec.pointwise(expr, pts).min()))
    assert worst >= -1e-12, f"{what}: the SDF is {worst} before t_lo"
    fin = np.isfinite(t_hi)
    if fin.any():
        g = ec.pointwise(expr, o[fin] + t_hi[fin, None] * d[fin])
        assert np.all(g <= 1e-12 * (1.0 + np.abs(t_hi[fin]))), (what, float(g.max()))
    hit = status == HIT
    assert np.all(fin[hit]) and np.all(t_hi[hit] - t_lo[hit] <= cc.WIDTH_REL * (1.0 + t_lo[hit])), what
    assert np.all(t_lo[hit] <= t_hi[hit]) and np.all(np.isinf(t_lo[status == MISS])) and np.all(np.isinf(t_hi[status == MISS]))
    assert np.all(np.isfinite(t_lo[status != MISS])), what
    return worst


@pytest.mark.parametrize("key", cc.frame_keys(), ids=[f"{k}{i}" for k, i in cc.frame_keys()])
def test_frames_are_sound_pointwise(key):
    f = cc.host_frame(key)
    o, d = cc.frame_rays(key)
    o = np.broadcast_to(o, d.shape)
    worst = check_sound(cc.frame_expression(key), o, d, f["t_lo"].ravel(), f["t_hi"].ravel(), f["status"].ravel(), cc.T_MAX, key)
    print(f"{key}: MISS / HIT / OPEN {counts(f['status'])}, least pointwise SDF before t_lo {worst:.3e}, steps max "
          f"{int(f['steps'].max())}")


TREES = cc.trees()


@pytest.mark.parametrize("idx", range(len(TREES)))
def test_trees_are_sound_pointwise(idx):
    """rays between two points of the region -- of its one cell for a tree that repeats, where g is continuous -- with t_max
    the distance between them; l_global is left out of play (1e9): the trees' Lipschitz bounds are not recorded"""
    expr = TREES[idx]
    o, d, length = cc.tree_rays(idx, expr, 64)
    out = [cc.host_march(expr, o[i:i + 1], d[i:i + 1], _native.certify_config(t_max=float(length[i]), l_global=1e9))
           for i in range(len(d))]
    t_lo, t_hi, status, steps = (np.concatenate([r[k] for r in out]) for k in range(4))
    worst = check_sound(expr, o, d, t_lo, t_hi, status, length, f"tree {idx}")
    print(f"tree {idx}: MISS / HIT / OPEN {counts(status)}, least pointwise SDF before t_lo {worst:.3e}, steps max {int(steps.max())}")


# ---- 3. the interval oracle's false hits ---------------------------------------------------------------------------------------

def false_hits(key):
    f, iv = cc.host_frame(key), cc.host_interval_frame(key)
    return iv["hit"] & ((f["status"] == MISS) | (f["t_lo"] - iv["depth"] > 1e-3)), iv["hit"]


def test_interval_oracle_false_hits():
    """Pixels the interval oracle (tol 1e-5, no prune) reports as hits and the certificate proves free: the bracket ends MISS,
    or t_lo lies more than 1e-3 past the oracle's t.  Measured at 64 x 48, each scene's default camera: Pillar Forest 2232
    of its 2972 oracle hits (316 of them MISS, the others hit the floor or a pillar metres further on), Hollow Cube 0 of 240
    (and 0 of 339 from (2, 2, 4)): the oracle's hit at the boundary of a repeat cell is false, its mask on Hollow Cube is
    not.  A count of 0 on both would mean that the second proof does not work."""
    n = {}
    for sid in (cc.PILLAR_FOREST, cc.HOLLOW_CUBE):
        false, o_hit = false_hits(("c", sid))
        n[sid] = int(false.sum())
        print(f"scene {sid}: {n[sid]} of {int(o_hit.sum())} interval-oracle hits are proven free, "
              f"{int((false & (cc.host_frame(('c', sid))['status'] == MISS)).sum())} of them MISS")
    assert n[cc.PILLAR_FOREST] + n[cc.HOLLOW_CUBE] >= 1
    assert n == cc.FALSE_HITS_MEASURED


def test_error_bar_of_a_capture():
    """certified_oracle.error_bar (host arithmetic) on the host builds' frames of Pillar Forest and Sphere"""
    key = ("c", cc.PILLAR_FOREST)
    f, iv = cc.host_frame(key), cc.host_interval_frame(key)
    bar = certified_oracle.error_bar(f, iv)
    assert [bar["n_miss"], bar["n_hit"], bar["n_open"]] == counts(f["status"]) and bar["n_pixels"] == 64 * 48
    assert bar["false_hits"] == cc.FALSE_HITS_MEASURED[cc.PILLAR_FOREST] and bar["n_oracle_hit"] == int(iv["hit"].sum())
    assert bar["lag_max"] > 1.0 and bar["oracle_miss_hit"] == 0
    bar = certified_oracle.error_bar(cc.host_frame(("c", 0)), cc.host_interval_frame(("c", 0)))
    assert bar["false_hits"] == 0 and bar["n_open"] == 0 and bar["n_hit"] == bar["n_oracle_hit"]
    assert 0.0 < bar["lag_median"] <= bar["lag_p95"] <= bar["lag_max"] < 1e-4       # the oracle is early by up to its lag


# ---- 4. constructed rays -------------------------------------------------------------------------------------------------------

SPHERE = sp.sd_sphere(1.0)


def one(expr, o, d, **cfg):
    t_lo, t_hi, status, steps = cc.host_march(expr, [o], [d], _native.certify_config(**cfg) if cfg else None)
    return float(t_lo[0]), float(t_hi[0]), int(status[0]), int(steps[0])


@pytest.mark.parametrize("o,d,t_star", [((-5.0, 1.0, 0.0), (1.0, 0.0, 0.0), 5.0), ((0.0, 1.0, -5.0), (0.0, 0.0, 1.0), 5.0),
                                        ((3.0, -1.0, 0.0), (-1.0, 0.0, 0.0), 3.0), ((-5.25, 0.0, 1.0), (1.0, 0.0, 0.0), 5.25)])
def test_tangent_contact_stays_open(o, d, t_star):
    """a tangent of the unit sphere (discriminant exactly 0): g >= 0 everywhere, g = 0 at t_star.  Never HIT (the computed g
    is 0 within 2^-27 of the contact, which is no witness), never MISS (the contact is not free): OPEN with t_lo just short of
    the contact and no witness."""
    t_lo, t_hi, status, steps = one(SPHERE, o, d)
    assert status == OPEN and t_hi == INF
    assert t_star - 1e-7 < t_lo <= t_star and steps < 200


def test_eye_inside_a_solid():
    assert one(SPHERE, (0.2, 0.1, 0.0), (0.0, 0.0, 1.0)) == (0.0, 0.0, HIT, 0)
    assert one(sp.catalogue_expressions()[6], (0.99, 0.99, 0.99), (-1.0, 0.0, 0.0)) == (0.0, 0.0, HIT, 0)   # a corner of Hollow Cube
    t_lo, t_hi, status, _ = one(SPHERE, (0.0, 0.0, 0.0), (0.0, 0.0, 1.0), max_steps=1)
    assert (t_lo, t_hi, status) == (0.0, 0.0, HIT)


def test_unnormalised_direction():
    """d = 2.5 x a unit vector: t scales by 1 / 2.5 and l_global = |d| keeps the second proof sound"""
    t_lo, t_hi, status, _ = one(SPHERE, (0.0, 0.0, 5.0), (0.0, 0.0, -2.5), l_global=2.5)
    assert status == HIT and t_lo <= 1.6 <= t_hi and t_hi - t_lo <= cc.WIDTH_REL * (1.0 + t_lo)
    u_lo, u_hi, u_status, _ = one(SPHERE, (0.0, 0.0, 5.0), (0.0, 0.0, -1.0))
    assert u_status == HIT and u_lo <= 4.0 <= u_hi


def test_t_max_around_a_root():
    """the root is at 4: t_max well below it is a MISS; just below it the witness past t_max closes the bracket (a HIT's t_lo
    is within t_max, its t_hi past it by no more than the width); above it the HIT is the same"""
    assert one(SPHERE, (0.0, 0.0, 5.0), (0.0, 0.0, -1.0), t_max=4.0 - 1e-3)[:3] == (INF, INF, MISS)
    below = one(SPHERE, (0.0, 0.0, 5.0), (0.0, 0.0, -1.0), t_max=4.0 - 1e-12)
    above = one(SPHERE, (0.0, 0.0, 5.0), (0.0, 0.0, -1.0), t_max=4.0 + 1e-3)
    assert below == above and below[2] == HIT and below[0] <= 4.0 - 1e-12 and below[0] <= 4.0 <= below[1]
    assert below[1] - below[0] <= cc.WIDTH_REL * 5.0


def test_one_step_ends_open_with_a_sound_bracket():
    assert one(SPHERE, (0.0, 0.0, 5.0), (0.0, 0.0, -1.0), max_steps=1) == (0.25, INF, OPEN, 1)
    t_lo, t_hi, status, steps = one(SPHERE, (0.0, 0.0, 5.0), (0.0, 0.0, -1.0), max_steps=12)
    assert status == OPEN and steps == 12 and t_lo <= 4.0 <= t_hi


def test_width_larger_than_tol():
    t_lo, t_hi, status, steps = one(SPHERE, (0.0, 0.0, 5.0), (0.0, 0.0, -1.0), width=1e-3, tol=1e-5)
    fine = one(SPHERE, (0.0, 0.0, 5.0), (0.0, 0.0, -1.0))
    assert status == HIT and t_lo <= 4.0 <= t_hi and 1e-5 < t_hi - t_lo <= 1e-3 and steps < fine[3]
    assert t_lo <= fine[0] and fine[1] <= t_hi


def test_zero_direction():
    """g is the constant f(o): outside the solid every probe is proven by the first proof, inside the eye is the witness"""
    assert one(SPHERE, (0.0, 0.0, 5.0), (0.0, 0.0, 0.0))[:3] == (INF, INF, MISS)
    assert one(SPHERE, (0.0, 0.0, 0.5), (0.0, 0.0, 0.0)) == (0.0, 0.0, HIT, 0)


def test_rows_of_a_frame():
    key = ("c", cc.HOLLOW_CUBE)
    W, H = cc.frame_size(key)
    part = cc.host_render(cc.frame_expression(key), cc.frame_camera(key).params14(), W, H, cc.frame_config(key), row0=7, rows=11)
    whole = cc.host_frame(key)
    assert cc.same(part, {k: v[7:18] for k, v in whole.items()})
    pruned = cc.host_render(cc.frame_expression(("c", 0)), cc.frame_camera(("c", 0)).params14(), 64, 48, None, cc.lib().rmc_scene_bound(0))
    free = cc.host_frame(("c", 0))
    assert np.array_equal(pruned["status"], free["status"]) and np.array_equal(cc.bits(pruned["t_hi"]), cc.bits(free["t_hi"]))
    assert (pruned["steps"] == 0).sum() > 2000 and np.all(pruned["status"][pruned["steps"] == 0] == MISS)


# ---- 5. the configuration and the C ABI without a device -----------------------------------------------------------------------

FIELDS = ["t_max", "tol", "h0", "growth", "h_max", "bound_radius", "width", "l_global", "k_min", "max_steps", "reserved"]


def test_config_layout():
    L = cc.lib()
    assert ctypes.sizeof(_native.RmCertifyConfig) == L.rmc_sizeof_config() == 80
    for i, n in enumerate(FIELDS):
        assert getattr(_native.RmCertifyConfig, n).offset == L.rmc_offsetof_config(i), n


def test_abi_layout_gcc():
    """RmCertifyConfig and the status values as gcc reads them from include/rm_hip.h"""
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "rm_hip.h"\nint main(void){printf("%zu %zu %zu %zu %d %d %d\\n", '
           'sizeof(RmCertifyConfig), offsetof(RmCertifyConfig, width), offsetof(RmCertifyConfig, max_steps), '
           'offsetof(RmCertifyConfig, reserved), RM_CERTIFY_MISS, RM_CERTIFY_HIT, RM_CERTIFY_OPEN);return 0;}\n')
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "a.c")
        with open(c, "w") as f:
            f.write(src)
        exe = os.path.join(td, "a")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, c], check=True)
        got = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    C = _native.RmCertifyConfig
    assert got == [ctypes.sizeof(C), C.width.offset, C.max_steps.offset, C.reserved.offset, MISS, HIT, OPEN] and (MISS, HIT, OPEN) == (0, 1, 2)


def test_resolve_defaults():
    L = cc.lib()
    out = np.empty(11)
    why = ctypes.create_string_buffer(256)
    assert L.rmc_resolve(None, 1.65, out.ctypes.data_as(dp), why, 256) == 0
    # t_max, tol, h0, growth, h_max as RmIntervalConfig; bound; width (absolute, relative); l_global, k_min as RmSegmentConfig
    assert out.tolist() == [100.0, 1e-5, 0.25, 1.5, 10.0, 1.65, 0.0, 1e-10, 1.0, 1e-6, 20000.0]
    cfg = _native.certify_config(7.0, 1e-3, 0.2, 2.0, 3.0, -1.0, 1e-4, 2.5, 1e-2, 99)
    assert L.rmc_resolve(ctypes.byref(cfg), 1.65, out.ctypes.data_as(dp), why, 256) == 0
    assert out.tolist() == [7.0, 1e-3, 0.2, 2.0, 3.0, -1.0, 1e-4, 0.0, 2.5, 1e-2, 99.0]
    cfg = _native.certify_config(max_steps=_native.RM_INTERVAL_MAX_STEPS)
    assert L.rmc_resolve(ctypes.byref(cfg), -1.0, out.ctypes.data_as(dp), why, 256) == 0 and out[10] == _native.RM_INTERVAL_MAX_STEPS


BAD_CONFIGS = [(f, v) for f in FIELDS[:5] + FIELDS[6:9] for v in (-1.0, float("nan"), float("inf"))] + \
    [("bound_radius", float("nan")), ("bound_radius", float("inf")), ("growth", 1.0), ("growth", 0.5), ("max_steps", -1),
     ("max_steps", _native.RM_INTERVAL_MAX_STEPS + 1), ("reserved", 1)]


@pytest.mark.parametrize("field,value", BAD_CONFIGS)
def test_bad_config(field, value):
    """every bad field: the host build refuses it with the reason, the C ABI returns RM_E_BAD_ARG with the same reason, before
    any device is looked for"""
    cfg = _native.RmCertifyConfig()
    setattr(cfg, field, value)
    out = np.empty(11)
    why = ctypes.create_string_buffer(256)
    assert cc.lib().rmc_resolve(ctypes.byref(cfg), -1.0, out.ctypes.data_as(dp), why, 256) == -2
    assert field in why.value.decode(), why.value
    L = _native.load()
    o, t, st = np.zeros(3), np.empty(1), np.empty(1, np.uint8)
    rc = L.rm_certify_march_rays(0, ctypes.byref(cfg), o.ctypes.data_as(dp), o.ctypes.data_as(dp), 1, t.ctypes.data_as(dp),
                                 t.ctypes.data_as(dp), st.ctypes.data, None)
    assert rc == _native.RM_E_BAD_ARG, rc
    assert why.value.decode() in L.rm_last_error().decode() and "RmCertifyConfig" in L.rm_last_error().decode()
    desc = _native.make_desc(0, 0, np.zeros(14), 4, 4)
    assert L.rm_certify_render(ctypes.byref(desc), ctypes.byref(cfg), None, None, None, None, None) == _native.RM_E_BAD_ARG


def test_supported_bad_scene_and_no_device():
    L = _native.load()
    for sid in list(range(20)) + [-1, 20, 1023, 999999]:
        assert L.rm_certify_supported(sid) == L.rm_segment_supported(sid) == (1 if sid in cc.CATALOGUE_IDS else 0), sid
    ops, nops = sp.to_ctypes(sp.op_union(sp.sd_sphere(0.5), sp.sd_box((0.2, 0.3, 0.4))))
    pid = _native.scene_program_create(ops, nops)
    assert L.rm_certify_supported(pid) == 1 and certified_oracle.has_certify(pid)
    _native.scene_program_destroy(pid)
    assert L.rm_certify_supported(pid) == 0
    assert [certified_oracle.has_certify(s) for s in ("Sphere", "Pillar Forest", "Mandelbulb", 17, 9, "no such scene")] == \
        [True, True, False, True, False, False]
    o, t, st = np.zeros(8), np.empty(4), np.empty(4, np.uint8)
    for sid in (9, 10, 11, 15, 16, 18, 20, -1, 5000, pid):           # no interval form; a destroyed program
        rc = L.rm_certify_march_rays(sid, None, o.ctypes.data_as(dp), o.ctypes.data_as(dp), 1, t.ctypes.data_as(dp),
                                     t.ctypes.data_as(dp), st.ctypes.data, None)
        assert rc == _native.RM_E_BAD_SCENE, (sid, rc)
        desc = _native.make_desc(sid, 0, np.zeros(14), 4, 4)
        assert L.rm_certify_render(ctypes.byref(desc), None, None, None, None, None, None) == _native.RM_E_BAD_SCENE, sid
    assert L.rm_certify_render(None, None, None, None, None, None, None) == _native.RM_E_BAD_ARG
    # every call that passes the host checks needs a device: a fresh process that never called rm_init
    code = (
        "import ctypes, numpy as np\n"
        "from raymarch_algo_compare_amd import _native\n"
        "L = _native.load(); dp = ctypes.POINTER(ctypes.c_double)\n"
        "o = np.zeros(8); a = np.empty(16); b = np.empty(16); s = np.empty(16, np.uint8)\n"
        "desc = _native.make_desc(3, 0, np.zeros(14), 4, 4)\n"
        "print(L.rm_certify_march_rays(0, None, o.ctypes.data_as(dp), o.ctypes.data_as(dp), 1, a.ctypes.data_as(dp),"
        " b.ctypes.data_as(dp), s.ctypes.data, None),"
        " L.rm_certify_render(ctypes.byref(desc), None, a.ctypes.data, b.ctypes.data, s.ctypes.data, None, None))\n")
    env = dict(os.environ, PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, check=True, capture_output=True, text=True).stdout
    assert [int(x) for x in out.split()] == [_native.RM_E_NO_DEVICE] * 2, out


# ---- 6. the sweep's columns ---------------------------------------------------------------------------------------------------------

def test_certify_columns():
    """a 1 x 6 frame: certificate HIT HIT MISS MISS OPEN OPEN, the frame hits pixels 0, 2, 4"""
    status = np.array([[HIT, HIT, MISS, MISS, OPEN, OPEN]], np.uint8)
    t_hi = np.array([[2.0, 3.0, INF, INF, INF, 5.0]])
    cert = {"status": status, "capture": {"hit": status == HIT, "depth": np.where(status == HIT, t_hi, 0.0)}}
    frame = {"hit": np.array([[1, 0, 1, 0, 1, 0]], bool), "depth": np.array([[2.5, 0.0, 9.0, 0.0, 4.0, 0.0]])}
    c = sweep.certify_columns(frame, cert)
    assert list(c) == sweep.CERTIFY_FIELDS == ["cert_open_frac", "cert_iou_lo", "cert_iou_hi", "cert_depth_mae", "cert_depth_p95"]
    # decided pixels: intersection 1, union 3; against: the two OPEN pixels join the union; for: pixel 4 joins both
    assert c["cert_open_frac"] == pytest.approx(2 / 6) and c["cert_iou_lo"] == pytest.approx(1 / 5) and c["cert_iou_hi"] == pytest.approx(2 / 4)
    assert c["cert_depth_mae"] == pytest.approx(0.5) and c["cert_depth_p95"] == pytest.approx(0.5)
    assert sweep.certify_columns(frame, None) == dict.fromkeys(sweep.CERTIFY_FIELDS)
    full = {"status": np.full((1, 6), MISS, np.uint8), "capture": {"hit": np.zeros((1, 6), bool), "depth": np.zeros((1, 6))}}
    c = sweep.certify_columns({"hit": np.zeros((1, 6), bool), "depth": np.zeros((1, 6))}, full)
    assert c["cert_iou_lo"] == c["cert_iou_hi"] == 1.0 and c["cert_open_frac"] == 0.0 and np.isnan(c["cert_depth_mae"])


def test_sweep_rejects_certify_without_the_interval_oracle():
    for oracle in (None, "exact"):
        with pytest.raises(ValueError):
            sweep.run_sweep(["Sphere"], ["Standard"], oracle=oracle, certify=True)
    assert sweep.ORACLES == ("interval", "exact")
    with pytest.raises(SystemExit):
        sweep.main(["--scenes", "Sphere", "--certify"])
