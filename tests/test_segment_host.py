"""The sound segment tracer without a GPU: csrc/rm_segment.h compiled for the host by g++ (tests/native/segment_check.cpp)
against the reference's own results (tests/golden/segment_*.npz, written by tools/gen_segment_golden.py), its value half
against the interval oracle bit for bit, the Lipschitz property the tracer rests on against the pointwise interpreter,
the host-only behaviour of the C ABI, scoring.residual, and the code object of the kernels (segment.o)."""
import ctypes
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, build_native
from test_interval_host import DEEP_PROGRAMS

from raymarch_algo_compare_amd import _native, scoring
from raymarch_algo_compare_amd import faithful_segment as fs
from raymarch_algo_compare_amd import scene_program as sp

CATALOGUE_IDS = [0, 1, 2, 3, 4, 5, 6, 7, 8, 12, 13, 14, 17, 19]
dp = ctypes.POINTER(ctypes.c_double)
vp = ctypes.c_void_p


def load_host_lib():
    """tests/native/segment_check.cpp built by g++, prototypes declared"""
    L = ctypes.CDLL(build_native("segment_check"))
    L.rms_eval.argtypes = [vp, ctypes.c_int32, dp, ctypes.c_size_t, dp, ctypes.c_char_p, ctypes.c_int]
    L.rms_eval_interval.argtypes = [vp, ctypes.c_int32, dp, ctypes.c_size_t, dp, dp, ctypes.c_char_p, ctypes.c_int]
    L.rms_march.argtypes = [vp, ctypes.c_int32, vp, dp, dp, ctypes.c_size_t, dp, vp, dp, ctypes.c_char_p, ctypes.c_int]
    L.rms_render.argtypes = [vp, ctypes.c_int32, vp, ctypes.c_double, dp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                             dp, vp, vp, dp, ctypes.c_char_p, ctypes.c_int]
    L.rms_resolve.argtypes = [vp, ctypes.c_double, dp, ctypes.c_char_p, ctypes.c_int]
    L.rms_scene_bound.restype = ctypes.c_double
    L.rms_sizeof_config.restype = ctypes.c_size_t
    L.rms_offsetof_config.restype = ctypes.c_size_t
    return L


@pytest.fixture(scope="module")
def lib():
    return load_host_lib()


@pytest.fixture(scope="module")
def prog_lib():
    L = ctypes.CDLL(build_native("program_check"))
    L.rmp_eval.argtypes = [vp, ctypes.c_int32, dp, ctypes.c_size_t, dp, ctypes.c_char_p, ctypes.c_int]
    return L


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def seg_cfg(a):
    """RmSegmentConfig from a fixture's cfg array (t_max, tol, h0, kappa, h_min, h_max, k_min, l_global, bound_radius, budget)"""
    return _native.segment_config(*(float(x) for x in a[:9]), budget=int(a[9]))


def host_eval(lib, ops, nops, segs):
    segs = np.ascontiguousarray(segs, np.float64)
    out = np.empty((len(segs), 4))
    why = ctypes.create_string_buffer(256)
    assert lib.rms_eval(ops, nops, segs.ctypes.data_as(dp), len(segs), out.ctypes.data_as(dp), why, 256) == 0, why.value
    return out


def host_eval_interval(lib, ops, nops, segs):
    segs = np.ascontiguousarray(segs, np.float64)
    out, pt = np.empty((len(segs), 2)), np.empty(len(segs))
    why = ctypes.create_string_buffer(256)
    rc = lib.rms_eval_interval(ops, nops, segs.ctypes.data_as(dp), len(segs), out.ctypes.data_as(dp), pt.ctypes.data_as(dp), why, 256)
    assert rc == 0, why.value
    return out, pt


def host_march(lib, ops, nops, cfg, o, d):
    o = np.ascontiguousarray(o, np.float64)
    d = np.ascontiguousarray(d, np.float64)
    n = len(o)
    t, iters, cursor = np.empty(n), np.empty(n, np.int32), np.empty(n)
    why = ctypes.create_string_buffer(256)
    rc = lib.rms_march(ops, nops, ctypes.byref(cfg), o.ctypes.data_as(dp), d.ctypes.data_as(dp), n, t.ctypes.data_as(dp),
                       iters.ctypes.data, cursor.ctypes.data_as(dp), why, 256)
    assert rc == 0, why.value
    return t, iters, cursor


def host_render(lib, ops, nops, cfg, scene_bound, cam14, W, H, row0=0, rows=None):
    rows = H if rows is None else rows
    cam = np.ascontiguousarray(cam14, np.float64)
    n = W * rows
    depth, hit, iters, cursor = np.empty(n), np.empty(n, np.uint8), np.empty(n, np.int32), np.empty(n)
    why = ctypes.create_string_buffer(256)
    rc = lib.rms_render(ops, nops, ctypes.byref(cfg), scene_bound, cam.ctypes.data_as(dp), W, H, row0, rows,
                        depth.ctypes.data_as(dp), hit.ctypes.data, iters.ctypes.data, cursor.ctypes.data_as(dp), why, 256)
    assert rc == 0, why.value
    return depth, hit, iters, cursor


def pointwise(prog_lib, ops, nops, pts):
    pts = np.ascontiguousarray(pts, np.float64)
    out = np.empty(len(pts))
    why = ctypes.create_string_buffer(256)
    assert prog_lib.rmp_eval(ops, nops, pts.ctypes.data_as(dp), len(pts), out.ctypes.data_as(dp), why, 256) == 0, why.value
    return out


def catalogue_ops(sid):
    return sp.to_ctypes(sp.catalogue_expressions()[sid])


# ---- 1. the reference's fixtures, bit for bit ---------------------------------------------------------------------------

def dsdf_cases():
    z = np.load(os.path.join(GOLDEN, "segment_dsdf.npz"))
    for sid in range(4):
        yield sid, z[f"s{sid}_segs"], z[f"s{sid}_out"]


def frame_cases():
    z = np.load(os.path.join(GOLDEN, "segment_frames.npz"))
    W, H = (int(x) for x in z["shape"])
    for key in sorted(k for k in z.files if k.endswith("_cam")):
        p = key[: -len("cam")]
        sid = int(p[1:p.index("_")])
        yield p, sid, W, H, z[p + "cam"], z[p + "cfg"], np.unpackbits(z[p + "hit"])[: W * H].astype(bool), z[p + "t"], z[p + "iters"]


def ray_cases():
    z = np.load(os.path.join(GOLDEN, "segment_rays.npz"))
    for key in sorted(k for k in z.files if k.endswith("_o")):
        p = key[:-1]
        sid = int(p.split("_s")[1].rstrip("_"))
        yield p, sid, z[p + "o"], z[p + "d"], z[p + "cfg"], z[p + "t"], z[p + "iters"]


def check_frame(depth, hit, iters, cursor, want_hit, want_t, want_iters, what):
    assert np.array_equal(hit.astype(bool), want_hit), (what, int((hit.astype(bool) != want_hit).sum()))
    assert np.array_equal(bits(depth[want_hit]), want_t), what
    assert np.all(depth[~want_hit] == 0.0), what
    assert np.array_equal(iters, want_iters), (what, np.nonzero(iters != want_iters)[0][:8])
    assert np.array_equal(cursor[want_hit], depth[want_hit]) and np.all(cursor[want_iters == 0] == 0.0), what


@pytest.mark.parametrize("sid", range(4))
def test_dual_sdf_matches_reference(lib, sid):
    for s, segs, want in dsdf_cases():
        if s != sid:
            continue
        ops, nops = catalogue_ops(sid)
        got = bits(host_eval(lib, ops, nops, segs))
        assert np.array_equal(got, want), (sid, np.argwhere(got != want)[:8])


@pytest.mark.parametrize("case", [c[0] for c in frame_cases()])
def test_frames_match_reference(lib, case):
    for p, sid, W, H, cam, cfg, want_hit, want_t, want_iters in frame_cases():
        if p != case:
            continue
        ops, nops = catalogue_ops(sid)
        depth, hit, iters, cursor = host_render(lib, ops, nops, seg_cfg(cfg), lib.rms_scene_bound(sid), cam, W, H)
        check_frame(depth, hit, iters, cursor, want_hit, want_t, want_iters, case)
        assert iters.max() <= int(cfg[9])


@pytest.mark.parametrize("case", [c[0] for c in ray_cases()])
def test_rays_match_reference(lib, case):
    for p, sid, o, d, cfg, want_t, want_iters in ray_cases():
        if p != case:
            continue
        ops, nops = catalogue_ops(sid)
        t, iters, _ = host_march(lib, ops, nops, seg_cfg(cfg), o, d)
        assert np.array_equal(bits(t), want_t), (case, np.nonzero(bits(t) != want_t)[0][:8])
        assert np.array_equal(iters, want_iters), case


def test_default_frames_use_no_budget():
    """the reference's own figures: on its four scenes no candidate ray uses up the budget of 4096"""
    for p, sid, W, H, cam, cfg, want_hit, want_t, want_iters in frame_cases():
        if p.endswith("default_"):
            assert want_iters.max() < 4096, p


# ---- 2. - 4. the value half, the Lipschitz property, degenerate segments -------------------------------------------------

def _programs():
    ex = sp.catalogue_expressions()
    out = [(f"catalogue {sid}", ex[sid]) for sid in CATALOGUE_IDS]
    with open(os.path.join(GOLDEN, "programs_trees.json"), encoding="utf-8") as f:
        trees = json.load(f)["trees"]
    out += [(f"tree {i}", sp.expr_from_json(t)) for i, t in enumerate(trees)]
    return out


PROGRAMS = _programs() + DEEP_PROGRAMS      # value slots 6-7 and point slot 3; a fused translate (test_interval_host.py)
IDS = [p[0] for p in PROGRAMS]
REGION = 3.0


def random_segments(rng, n, lo=None, hi=None):
    """n segments (n x 8) between two random points of the box [lo, hi] (default the cube of half edge REGION): unit
    direction, a random t0, lengths from 1e-6 up to the box's diagonal"""
    lo = np.full(3, -REGION) if lo is None else lo
    hi = np.full(3, REGION) if hi is None else hi
    a = rng.uniform(lo, hi, size=(n, 3))
    b = rng.uniform(lo, hi, size=(n, 3))
    b = a + (b - a) * (10.0 ** rng.uniform(-6.0, 0.0, size=(n, 1)))
    length = np.linalg.norm(b - a, axis=1)
    d = (b - a) / length[:, None]
    t0 = rng.uniform(0.0, 4.0, size=n)
    return np.concatenate([a - t0[:, None] * d, d, t0[:, None], (t0 + length)[:, None]], axis=1)


@pytest.mark.parametrize("idx", range(len(PROGRAMS)), ids=IDS)
def test_value_half_is_the_interval_program(lib, idx):
    name, expr = PROGRAMS[idx]
    ops, nops = sp.to_ctypes(expr)
    segs = random_segments(np.random.default_rng(3000 + idx), 1500)
    segs[::9, 3:6] *= 2.5                                  # some unnormalised directions
    dual = host_eval(lib, ops, nops, segs)
    ival, _ = host_eval_interval(lib, ops, nops, segs)
    assert np.array_equal(bits(dual[:, :2]), bits(ival)), (name, np.argwhere(bits(dual[:, :2]) != bits(ival))[:8])
    assert np.all(dual[:, 2] <= dual[:, 3]), name


def one_cell(expr):
    """The world-space box inside which no op_repeat of the tree wraps: the central cell of each repeated coordinate, in
    the frame the enclosing op_translates give it (inside its central cell an op_repeat is the identity, so a nested one
    keeps that frame).  None for a tree without op_repeat."""
    lo, hi, found = np.full(3, -REGION), np.full(3, REGION), [False]

    def walk(e, offset):
        if e.op == "op_translate":
            offset = offset + np.array(e.param("offset"))
        elif e.op == "op_repeat":
            found[0] = True
            for ax, s in enumerate(e.param("spacing")):
                if s > 0.0:
                    lo[ax] = max(lo[ax], offset[ax] - 0.5 * s)
                    hi[ax] = min(hi[ax], offset[ax] + 0.5 * s)
        for c in e.children:
            walk(c, offset)

    walk(expr, np.zeros(3))
    return (lo, hi) if found[0] else None


@pytest.mark.parametrize("idx", range(len(PROGRAMS)), ids=IDS)
def test_der_bounds_the_change_along_the_ray(lib, prog_lib, idx):
    """|g(tb) - g(ta)| <= K (tb - ta) (1 + 1e-9) + 1e-12 for 32 pairs ta < tb inside each random segment, g the pointwise
    program_eval along the ray and K = max |der| unclamped.  The slack is the rounding of to-nearest arithmetic.  The bound
    presupposes that g is continuous on the segment: a tree that repeats a shape which is not even in the repeated
    coordinate jumps at cell boundaries, so the trees with an op_repeat draw their segments inside one cell (one_cell);
    the catalogue programs are continuous and take unrestricted segments."""
    name, expr = PROGRAMS[idx]
    ops, nops = sp.to_ctypes(expr)
    rng = np.random.default_rng(4000 + idx)
    cell = one_cell(expr) if name.startswith("tree") else None
    if cell is not None:
        w = cell[1] - cell[0]
        assert np.all(w > 0.0), (name, "the repeats of this tree share no cell")
        segs = random_segments(rng, 400, cell[0] + 1e-9 * w, cell[1] - 1e-9 * w)
    else:
        segs = random_segments(rng, 400)
    K = np.abs(host_eval(lib, ops, nops, segs)[:, 2:]).max(axis=1)
    o, d, t0, t1 = segs[:, 0:3], segs[:, 3:6], segs[:, 6], segs[:, 7]
    u = np.sort(rng.uniform(0.0, 1.0, size=(len(segs), 32, 2)), axis=2)
    u[:, 0] = (0.0, 1.0)                                   # the whole segment too
    ta = np.clip(t0[:, None] + u[..., 0] * (t1 - t0)[:, None], t0[:, None], t1[:, None])
    tb = np.clip(t0[:, None] + u[..., 1] * (t1 - t0)[:, None], t0[:, None], t1[:, None])
    ga = pointwise(prog_lib, ops, nops, (o[:, None, :] + ta[..., None] * d[:, None, :]).reshape(-1, 3)).reshape(ta.shape)
    gb = pointwise(prog_lib, ops, nops, (o[:, None, :] + tb[..., None] * d[:, None, :]).reshape(-1, 3)).reshape(ta.shape)
    bad = np.abs(gb - ga) > K[:, None] * (tb - ta) * (1.0 + 1e-9) + 1e-12
    assert not bad.any(), (name, int(bad.sum()), np.argwhere(bad)[:4])


@pytest.mark.parametrize("idx", range(len(PROGRAMS)), ids=IDS)
def test_degenerate_segment_is_the_point(lib, idx):
    name, expr = PROGRAMS[idx]
    ops, nops = sp.to_ctypes(expr)
    segs = random_segments(np.random.default_rng(5000 + idx), 1000)
    segs[:, 7] = segs[:, 6]
    dual = host_eval(lib, ops, nops, segs)
    _, pt = host_eval_interval(lib, ops, nops, segs)
    assert np.array_equal(bits(dual[:, 0]), bits(dual[:, 1])), name
    assert np.array_equal(bits(dual[:, 0]), bits(pt)), name


# ---- 5. the C ABI without a device ---------------------------------------------------------------------------------------

FIELDS = ["t_max", "tol", "h0", "kappa", "h_min", "h_max", "k_min", "l_global", "bound_radius", "budget", "reserved"]


def test_supported():
    L = _native.load()
    for sid in list(range(20)) + [-1, 20, 1023, 999999]:
        assert L.rm_segment_supported(sid) == L.rm_interval_supported(sid) == (1 if sid in CATALOGUE_IDS else 0), sid
    ops, nops = sp.to_ctypes(sp.op_union(sp.sd_sphere(0.5), sp.sd_box((0.2, 0.3, 0.4))))
    pid = _native.scene_program_create(ops, nops)
    assert L.rm_segment_supported(pid) == 1
    _native.scene_program_destroy(pid)
    assert L.rm_segment_supported(pid) == 0
    assert [fs.has_segment(s) for s in ("Sphere", "Thin Torus", "Mandelbulb", "Menger Sponge", 17, 9)] == \
        [True, True, False, False, True, False]


def test_config_layout(lib):
    assert ctypes.sizeof(_native.RmSegmentConfig) == lib.rms_sizeof_config() == 80
    for i, n in enumerate(FIELDS):
        assert getattr(_native.RmSegmentConfig, n).offset == lib.rms_offsetof_config(i), n


def test_abi_layout_gcc():
    """RmSegmentConfig as gcc lays it out from include/rm_hip.h"""
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "rm_hip.h"\nint main(void){printf("%zu %zu %zu %zu %d\\n", '
           'sizeof(RmSegmentConfig), offsetof(RmSegmentConfig, bound_radius), offsetof(RmSegmentConfig, budget), '
           'offsetof(RmSegmentConfig, reserved), RM_SEGMENT_MAX_STEPS);return 0;}\n')
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "a.c")
        with open(c, "w") as f:
            f.write(src)
        exe = os.path.join(td, "a")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, c], check=True)
        got = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    C = _native.RmSegmentConfig
    assert got == [ctypes.sizeof(C), C.bound_radius.offset, C.budget.offset, C.reserved.offset, _native.RM_SEGMENT_MAX_STEPS]


def test_resolve_defaults(lib):
    out = np.empty(10)
    why = ctypes.create_string_buffer(256)
    assert lib.rms_resolve(None, 1.65, out.ctypes.data_as(dp), why, 256) == 0
    assert out.tolist() == [100.0, 1e-4, 0.1, 1.5, 1e-5, 10.0, 1e-6, 1.0, 1.65, 4096.0]
    cfg = _native.segment_config(7.0, 1e-3, 0.2, 2.0, 1e-4, 3.0, 1e-2, 0.5, -1.0, 99)
    assert lib.rms_resolve(ctypes.byref(cfg), 1.65, out.ctypes.data_as(dp), why, 256) == 0
    assert out.tolist() == [7.0, 1e-3, 0.2, 2.0, 1e-4, 3.0, 1e-2, 0.5, -1.0, 99.0]


BAD_CONFIGS = [(f, v) for f in FIELDS[:8] for v in (-1.0, float("nan"), float("inf"))] + \
    [("bound_radius", float("nan")), ("bound_radius", float("inf")), ("budget", -1),
     ("budget", _native.RM_SEGMENT_MAX_STEPS + 1), ("reserved", 1)]


@pytest.mark.parametrize("field,value", BAD_CONFIGS)
def test_bad_config(lib, field, value):
    cfg = _native.RmSegmentConfig()
    setattr(cfg, field, value)
    out = np.empty(10)
    why = ctypes.create_string_buffer(256)
    assert lib.rms_resolve(ctypes.byref(cfg), -1.0, out.ctypes.data_as(dp), why, 256) == -2
    assert field in why.value.decode() or field == "reserved", why.value
    L = _native.load()
    o = np.zeros(3)
    t = np.empty(1)
    rc = L.rm_segment_march_rays(0, ctypes.byref(cfg), o.ctypes.data_as(dp), o.ctypes.data_as(dp), 1, t.ctypes.data_as(dp), None, None)
    assert rc == _native.RM_E_BAD_ARG, rc
    desc = _native.make_desc(0, 0, np.zeros(14), 4, 4)
    assert L.rm_segment_render(ctypes.byref(desc), ctypes.byref(cfg), None, None, None, None, None) == _native.RM_E_BAD_ARG


def test_bad_scene_and_no_device():
    L = _native.load()
    o = np.zeros(8)
    t = np.empty(4)
    for sid in (9, 10, 11, 15, 16, 18, 20, -1, 5000):
        rc = L.rm_segment_march_rays(sid, None, o.ctypes.data_as(dp), o.ctypes.data_as(dp), 1, t.ctypes.data_as(dp), None, None)
        assert rc == _native.RM_E_BAD_SCENE, (sid, rc)
        assert L.rm_segment_sdf_eval(sid, o.ctypes.data_as(dp), 1, t.ctypes.data_as(dp)) == _native.RM_E_BAD_SCENE, sid
        desc = _native.make_desc(sid, 0, np.zeros(14), 4, 4)
        assert L.rm_segment_render(ctypes.byref(desc), None, None, None, None, None, None) == _native.RM_E_BAD_SCENE, sid
    # every call that passes the host checks needs a device: a fresh process that never called rm_init
    code = (
        "import ctypes, numpy as np\n"
        "from raymarch_algo_compare_amd import _native\n"
        "L = _native.load(); dp = ctypes.POINTER(ctypes.c_double)\n"
        "o = np.zeros(8); t = np.empty(4); d = np.empty(16); h = np.empty(16, np.uint8)\n"
        "desc = _native.make_desc(3, 0, np.zeros(14), 4, 4)\n"
        "print(L.rm_segment_march_rays(0, None, o.ctypes.data_as(dp), o.ctypes.data_as(dp), 1, t.ctypes.data_as(dp), None, None),"
        " L.rm_segment_sdf_eval(0, o.ctypes.data_as(dp), 1, t.ctypes.data_as(dp)),"
        " L.rm_segment_render(ctypes.byref(desc), None, d.ctypes.data_as(dp), h.ctypes.data, None, None, None))\n")
    env = dict(os.environ, PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, check=True, capture_output=True, text=True).stdout
    assert [int(x) for x in out.split()] == [_native.RM_E_NO_DEVICE] * 3, out


def test_sweep_rejects_unknown_ceiling_before_the_device():
    from raymarch_algo_compare_amd import sweep
    with pytest.raises(ValueError):
        sweep.run_sweep(["Sphere"], ["Standard"], ceiling="affine")
    assert sweep.CEILING_FIELDS == ["ceiling_iou", "ceiling_depth_med", "ceiling_iters_median", "ceiling_iters_p95"]
    assert sweep.ceiling_columns(None, None) == dict.fromkeys(sweep.CEILING_FIELDS)


def test_silhouette_band_and_residual():
    hit = np.zeros((7, 7), bool)
    hit[2:5, 2:5] = True                                   # a 3 x 3 block: its ring of 8 and the 4-neighbours outside it
    edge = np.zeros((7, 7), bool)
    edge[2:5, 2:5] = True
    edge[3, 3] = False
    edge[1, 2:5] = edge[5, 2:5] = edge[2:5, 1] = edge[2:5, 5] = True
    assert np.array_equal(scoring.silhouette_band(hit, k=0), edge)
    band = scoring.silhouette_band(hit, k=1)
    assert band[3, 3] and band[1, 1] and band[0, 3] and not band[0, 0] and not band[0, 1]
    assert not scoring.silhouette_band(np.ones((4, 4), bool)).any() and not scoring.silhouette_band(np.zeros((4, 4), bool)).any()

    truth = np.array([[1, 1, 1, 0, 0, 0]], bool)
    mine = np.array([[0, 1, 1, 1, 0, 0]], bool)
    d_truth = np.array([[1.0, 2.0, 3.0, 0.0, 0.0, 0.0]])
    d_mine = np.array([[0.0, 2.5, 2.0, 9.0, 0.0, 0.0]])
    core_out = np.array([[0, 0, 0, 1, 0, 0]], bool)
    r = scoring.residual(mine, d_mine, truth, d_truth, core_out)
    assert list(r) == ["iou", "core_iou", "false_hit", "false_miss", "depth_rmse", "depth_med", "depth_p95", "depth_signed",
                       "n_analytic_hit", "n_method_hit", "n_co_hit"]
    assert r["iou"] == pytest.approx(2 / 4) and r["core_iou"] == pytest.approx(2 / 3)
    assert r["false_hit"] == pytest.approx(1 / 3) and r["false_miss"] == pytest.approx(1 / 3)
    assert r["depth_rmse"] == pytest.approx(np.sqrt((0.25 + 1.0) / 2)) and r["depth_med"] == pytest.approx(0.75)
    assert r["depth_p95"] == pytest.approx(float(np.percentile([0.5, 1.0], 95))) and r["depth_signed"] == pytest.approx(-0.25)
    assert (r["n_analytic_hit"], r["n_method_hit"], r["n_co_hit"]) == (3, 3, 2)
    none = scoring.residual(np.zeros((2, 2), bool), np.zeros((2, 2)), np.zeros((2, 2), bool), np.zeros((2, 2)), np.zeros((2, 2), bool))
    assert none["iou"] == 0.0 and np.isnan(none["depth_med"]) and none["n_co_hit"] == 0
    assert fs.cost({"iters": np.array([[3, 9, 5, 0]]), "hit": np.array([[1, 0, 1, 0]], bool)}) == \
        {"iters_median": 4.0, "iters_p95": pytest.approx(4.9), "iters_max": 5}


# ---- 6. the code object ------------------------------------------------------------------------------------------------------

OBJ = os.path.join(ROOT, "raymarch_algo_compare_amd", "_build", "segment.o")


def test_code_object_no_scratch_no_spills():
    """as test_interval_host does for interval.o"""
    import importlib.util
    assert os.path.exists(OBJ), "segment.o is missing: build the library (make -C raymarch_algo_compare_amd/csrc)"
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    kernels = [k for k in tool.collect([OBJ]) if "_kernel" in k["demangled"]]
    assert sorted(re.search(r"\w+_kernel", k["demangled"]).group(0) for k in kernels) == \
        ["segment_march_kernel", "segment_render_kernel", "segment_sdf_kernel"]
    found = tool.matching_instructions(OBJ, r"\b(scratch|buffer)_")
    for k in kernels:
        assert found.get(k["name"]) == [], (k["demangled"], found.get(k["name"], "not disassembled")[:4])
        assert k["vgpr_spill_count"] == 0, k["demangled"]
        assert k["private_segment_fixed_size"] == 0, k["demangled"]
