"""The affine range without a GPU: csrc/rm_affine.h compiled for the host by g++ (tests/native/affine_check.cpp) against the
reference's own results (tests/golden/affine_*.npz, written by tools/gen_affine_golden.py), its inclusion property against
the pointwise interpreter, the meet against the two ranges it is made of, the march against the surface it must not pass,
the host-only behaviour of the C ABI, and the code object of the kernels (affine.o)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, build_native
from test_segment_host import CATALOGUE_IDS, IDS, PROGRAMS, bits, catalogue_ops, pointwise, random_segments

from raymarch_algo_compare_amd import _native, scoring
from raymarch_algo_compare_amd import affine_range as ar
from raymarch_algo_compare_amd import scene_program as sp

dp = ctypes.POINTER(ctypes.c_double)
vp = ctypes.c_void_p
AFFINE, MEET = _native.RM_RANGE_AFFINE, _native.RM_RANGE_MEET
N_SAMPLES = 33


def load_host_lib():
    """tests/native/affine_check.cpp built by g++, prototypes declared"""
    L = ctypes.CDLL(build_native("affine_check"))
    L.rma_range.argtypes = [vp, ctypes.c_int32, ctypes.c_int, dp, ctypes.c_size_t, dp, vp, ctypes.c_char_p, ctypes.c_int]
    L.rma_interval.argtypes = [vp, ctypes.c_int32, dp, ctypes.c_size_t, dp, ctypes.c_char_p, ctypes.c_int]
    L.rma_march.argtypes = [vp, ctypes.c_int32, ctypes.c_int, vp, dp, dp, ctypes.c_size_t, dp, vp, ctypes.c_char_p, ctypes.c_int]
    L.rma_render.argtypes = [vp, ctypes.c_int32, ctypes.c_int, vp, ctypes.c_double, dp, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                             ctypes.c_int, dp, vp, vp, ctypes.c_char_p, ctypes.c_int]
    L.rma_scene_bound.restype = ctypes.c_double
    return L


@pytest.fixture(scope="module")
def lib():
    return load_host_lib()


@pytest.fixture(scope="module")
def prog_lib():
    L = ctypes.CDLL(build_native("program_check"))
    L.rmp_eval.argtypes = [vp, ctypes.c_int32, dp, ctypes.c_size_t, dp, ctypes.c_char_p, ctypes.c_int]
    return L


def iv_cfg(a):
    """RmIntervalConfig from a fixture's cfg array (t_max, tol, h0, growth, h_max, normal_eps, bound_radius, max_steps)"""
    return _native.interval_config(*(float(x) for x in a[:7]), max_steps=int(a[7]))


def host_range(lib, ops, nops, mode, segs, want_form=True):
    segs = np.ascontiguousarray(segs, np.float64)
    rng = np.empty((len(segs), 2))
    form = np.empty((len(segs), 3)) if want_form else None
    why = ctypes.create_string_buffer(256)
    rc = lib.rma_range(ops, nops, mode, segs.ctypes.data_as(dp), len(segs), rng.ctypes.data_as(dp),
                       None if form is None else form.ctypes.data, why, 256)
    assert rc == 0, why.value
    return rng, form


def host_interval(lib, ops, nops, segs):
    segs = np.ascontiguousarray(segs, np.float64)
    out = np.empty((len(segs), 2))
    why = ctypes.create_string_buffer(256)
    assert lib.rma_interval(ops, nops, segs.ctypes.data_as(dp), len(segs), out.ctypes.data_as(dp), why, 256) == 0, why.value
    return out


def host_march(lib, ops, nops, mode, cfg, o, d):
    o = np.ascontiguousarray(o, np.float64)
    d = np.ascontiguousarray(d, np.float64)
    t, steps = np.empty(len(o)), np.empty(len(o), np.int32)
    why = ctypes.create_string_buffer(256)
    rc = lib.rma_march(ops, nops, mode, ctypes.byref(cfg) if cfg is not None else None, o.ctypes.data_as(dp), d.ctypes.data_as(dp),
                       len(o), t.ctypes.data_as(dp), steps.ctypes.data, why, 256)
    assert rc == 0, why.value
    return t, steps


def host_render(lib, ops, nops, mode, cfg, scene_bound, cam14, W, H, row0=0, rows=None):
    """mode 0: the interval oracle's capture"""
    rows = H if rows is None else rows
    cam = np.ascontiguousarray(cam14, np.float64)
    n = W * rows
    depth, hit, steps = np.empty(n), np.empty(n, np.uint8), np.empty(n, np.int32)
    why = ctypes.create_string_buffer(256)
    rc = lib.rma_render(ops, nops, mode, ctypes.byref(cfg) if cfg is not None else None, scene_bound, cam.ctypes.data_as(dp), W, H,
                        row0, rows, depth.ctypes.data_as(dp), hit.ctypes.data, steps.ctypes.data, why, 256)
    assert rc == 0, why.value
    return depth, hit, steps


# ---- 1. the reference's fixtures, bit for bit ---------------------------------------------------------------------------

def form_cases():
    z = np.load(os.path.join(GOLDEN, "affine_forms.npz"))
    for sid in range(4):
        yield sid, z[f"s{sid}_segs"], z[f"s{sid}_out"]


def frame_cases():
    z = np.load(os.path.join(GOLDEN, "affine_frames.npz"))
    W, H = (int(x) for x in z["shape"])
    for key in sorted(k for k in z.files if k.endswith("_cam")):
        p = key[: -len("cam")]
        sid = int(p[1:p.index("_")])
        yield (p, sid, W, H, z[p + "cam"], z[p + "cfg"], np.unpackbits(z[p + "hit"])[: W * H].astype(bool), z[p + "t"],
               z[p + "steps"], z[p + "score"])


def ray_cases():
    z = np.load(os.path.join(GOLDEN, "affine_rays.npz"))
    for key in sorted(k for k in z.files if k.endswith("_o")):
        p = key[:-1]
        sid = int(p.split("_s")[1].rstrip("_"))
        yield p, sid, z[p + "o"], z[p + "d"], z[p + "cfg"], z[p + "t"], z[p + "steps"]


def check_frame(depth, hit, steps, want_hit, want_t, want_steps, what):
    assert np.array_equal(hit.astype(bool), want_hit), (what, int((hit.astype(bool) != want_hit).sum()))
    assert np.array_equal(bits(depth[want_hit]), want_t), what
    assert np.all(depth[~want_hit] == 0.0), what
    assert np.array_equal(steps, want_steps), (what, np.nonzero(steps != want_steps)[0][:8])


@pytest.mark.parametrize("sid", range(4))
def test_forms_match_reference(lib, sid):
    """x0, x1, e, lo, hi of the reference's COMPONENT_SCENES over its _aff_positions"""
    for s, segs, want in form_cases():
        if s != sid:
            continue
        assert len(segs) == 2000
        ops, nops = catalogue_ops(sid)
        rng, form = host_range(lib, ops, nops, AFFINE, segs)
        got = bits(np.concatenate([form, rng], axis=1))
        assert np.array_equal(got, want), (sid, np.argwhere(got != want)[:8])


@pytest.mark.parametrize("case", [c[0] for c in frame_cases()])
def test_frames_match_reference(lib, case):
    """hit map, t, per-pixel steps; and the IoU of the capture against our interval oracle's host capture, which the
    reference computed against its own interval capture: the recorded value exactly"""
    for p, sid, W, H, cam, cfg, want_hit, want_t, want_steps, score in frame_cases():
        if p != case:
            continue
        ops, nops = catalogue_ops(sid)
        bound = lib.rma_scene_bound(sid)
        depth, hit, steps = host_render(lib, ops, nops, AFFINE, iv_cfg(cfg), bound, cam, W, H)
        check_frame(depth, hit, steps, want_hit, want_t, want_steps, case)
        assert steps.max() <= int(cfg[7])
        gdepth, ghit, _ = host_render(lib, ops, nops, 0, iv_cfg(cfg), bound, cam, W, H)
        ghit2 = ghit.reshape(H, W) > 0
        res = scoring.residual(hit.reshape(H, W) > 0, depth.reshape(H, W), ghit2, gdepth.reshape(H, W),
                               scoring.silhouette_band(ghit2, k=2))
        assert [res["iou"], res["core_iou"]] == score.tolist(), case


def test_patched_frames_pin_the_step_cap():
    """the patched case is worth its name only if max_steps cuts rays short somewhere"""
    assert any(p.endswith("patched_") and want_steps.max() == int(cfg[7])
               for p, sid, W, H, cam, cfg, want_hit, want_t, want_steps, score in frame_cases())


@pytest.mark.parametrize("case", [c[0] for c in ray_cases()])
def test_rays_match_reference(lib, case):
    for p, sid, o, d, cfg, want_t, want_steps in ray_cases():
        if p != case:
            continue
        ops, nops = catalogue_ops(sid)
        t, steps = host_march(lib, ops, nops, AFFINE, iv_cfg(cfg), o, d)
        assert np.array_equal(bits(t), want_t), (case, np.nonzero(bits(t) != want_t)[0][:8])
        assert np.array_equal(steps, want_steps), case


# ---- 2. inclusion, the meet ---------------------------------------------------------------------------------------------

def segment_samples(segs):
    """33 points of each segment, both ends among them: (n, 33, 3)"""
    o, d, t0, t1 = segs[:, 0:3], segs[:, 3:6], segs[:, 6], segs[:, 7]
    tau = t0[:, None] + np.linspace(0.0, 1.0, N_SAMPLES)[None, :] * (t1 - t0)[:, None]
    tau[:, -1] = t1
    return o[:, None, :] + tau[..., None] * d[:, None, :]


def some_segments(idx, n):
    segs = random_segments(np.random.default_rng(6000 + idx), n)
    segs[::9, 3:6] *= 2.5                                  # some unnormalised directions
    segs[::10, 7] = segs[::10, 6]                          # degenerate segments
    return segs


@pytest.mark.parametrize("idx", range(len(PROGRAMS)), ids=IDS)
@pytest.mark.parametrize("mode", [AFFINE, MEET], ids=["affine", "meet"])
def test_inclusion(lib, prog_lib, mode, idx):
    """lo - e <= f(p) <= hi + e, e = 1e-12 (1 + |f|), at 33 samples of random segments (lengths 1e-6 .. the region's
    diagonal): the 14 catalogue programs, the trees of programs_trees.json and DEEP_PROGRAMS"""
    name, expr = PROGRAMS[idx]
    ops, nops = sp.to_ctypes(expr)
    segs = some_segments(idx, 600)
    rng, _ = host_range(lib, ops, nops, mode, segs, want_form=False)
    assert np.all(rng[:, 0] <= rng[:, 1]), name
    f = pointwise(prog_lib, ops, nops, segment_samples(segs).reshape(-1, 3)).reshape(len(segs), N_SAMPLES)
    e = 1e-12 * (1.0 + np.abs(f))
    bad_lo = f < rng[:, :1] - e
    bad_hi = f > rng[:, 1:] + e
    assert not bad_lo.any(), (name, "lower bound violated", np.argwhere(bad_lo)[:4])
    assert not bad_hi.any(), (name, "upper bound violated", np.argwhere(bad_hi)[:4])


@pytest.mark.parametrize("idx", range(len(PROGRAMS)), ids=IDS)
def test_meet_is_the_intersection(lib, idx):
    """bitwise np.maximum of the lower and np.minimum of the upper ends of the affine and the interval range; and the
    range of the form is x0 -+ (|x1| + e)"""
    name, expr = PROGRAMS[idx]
    ops, nops = sp.to_ctypes(expr)
    segs = some_segments(idx, 1000)
    a, form = host_range(lib, ops, nops, AFFINE, segs)
    m, _ = host_range(lib, ops, nops, MEET, segs, want_form=False)
    i = host_interval(lib, ops, nops, segs)
    assert np.array_equal(bits(m[:, 0]), bits(np.maximum(a[:, 0], i[:, 0]))), name
    assert np.array_equal(bits(m[:, 1]), bits(np.minimum(a[:, 1], i[:, 1]))), name
    rad = np.abs(form[:, 1]) + form[:, 2]
    assert np.all(form[:, 2] >= 0.0), name
    assert np.array_equal(bits(a[:, 0]), bits(form[:, 0] - rad)) and np.array_equal(bits(a[:, 1]), bits(form[:, 0] + rad)), name


# ---- 3. never past a surface ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("idx", range(len(PROGRAMS)), ids=IDS)
@pytest.mark.parametrize("mode", [AFFINE, MEET], ids=["affine", "meet"])
def test_march_never_passes_a_surface(lib, prog_lib, mode, idx):
    """rays from a shell around the region, aimed near its centre: the pointwise program at 256 samples of [0, t] of every
    hit and of [0, t_max] of every miss is >= -e, e = 1e-12 (1 + |f|): the cursor only ever crosses segments proven
    empty.  The property presupposes an origin outside the solid (a ray that starts inside hits at t = 0, where f < 0), so
    origins are drawn until they are; no ray may end by the step cap, which says nothing about the rest of the ray."""
    name, expr = PROGRAMS[idx]
    ops, nops = sp.to_ctypes(expr)
    rng = np.random.default_rng(7000 + idx)
    n, t_max = 48, 12.0
    o = rng.normal(size=(8 * n, 3))
    o = o / np.linalg.norm(o, axis=1, keepdims=True) * rng.uniform(4.0, 6.0, size=(len(o), 1))
    o = o[pointwise(prog_lib, ops, nops, o) > 0.0][:n]
    assert len(o) == n, (name, len(o))
    d = -o + rng.normal(scale=1.0, size=o.shape)
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    t, steps = host_march(lib, ops, nops, mode, _native.interval_config(t_max=t_max), o, d)
    assert steps.max() < 20000, (name, "a ray used up max_steps")
    end = np.where(np.isfinite(t), t, t_max)
    tau = np.linspace(0.0, 1.0, 256)[None, :] * end[:, None]
    f = pointwise(prog_lib, ops, nops, (o[:, None, :] + tau[..., None] * d[:, None, :]).reshape(-1, 3)).reshape(n, 256)
    e = 1e-12 * (1.0 + np.abs(f))
    bad = f < -e
    assert not bad.any(), (name, np.argwhere(bad)[:4], f[bad][:4])


# ---- 4. the C ABI without a device ---------------------------------------------------------------------------------------

def test_supported():
    L = _native.load()
    for sid in list(range(20)) + [-1, 20, 1023, 999999]:
        assert L.rm_affine_supported(sid) == L.rm_interval_supported(sid) == (1 if sid in CATALOGUE_IDS else 0), sid
    ops, nops = sp.to_ctypes(sp.op_union(sp.sd_sphere(0.5), sp.sd_box((0.2, 0.3, 0.4))))
    pid = _native.scene_program_create(ops, nops)
    assert L.rm_affine_supported(pid) == 1
    _native.scene_program_destroy(pid)
    assert L.rm_affine_supported(pid) == 0
    assert [ar.has_affine(s) for s in ("Sphere", "Thin Torus", "Mandelbulb", "Menger Sponge", 17, 9)] == \
        [True, True, False, False, True, False]
    assert (_native.RM_RANGE_AFFINE, _native.RM_RANGE_MEET) == (1, 2)
    with pytest.raises(ValueError):
        ar.capture("Sphere", 8, 8, "interval")


def test_header_declares_the_modes():
    with open(os.path.join(ROOT, "include", "rm_hip.h"), encoding="utf-8") as f:
        h = f.read()
    assert re.search(r"#define RM_RANGE_AFFINE 1\b", h) and re.search(r"#define RM_RANGE_MEET 2\b", h)
    for name in ("rm_affine_supported", "rm_affine_range_eval", "rm_affine_march_rays", "rm_affine_render"):
        assert re.search(r"\bint %s\(" % name, h), name
        assert name in _native.EXPORTS, name


def _calls(L, sid, mode, cfg, with_range=True):
    """the three device calls with valid buffers: their return codes (the range call, which reads no configuration, only
    `with_range`)"""
    o = np.zeros(8)
    t = np.empty(4)
    d, h = np.empty(16), np.empty(16, np.uint8)
    desc = _native.make_desc(sid, 0, np.zeros(14), 4, 4)
    ref = ctypes.byref(cfg) if cfg is not None else None
    first = [L.rm_affine_range_eval(sid, mode, o.ctypes.data_as(dp), 1, t.ctypes.data_as(dp), None)] if with_range else []
    return first + [
            L.rm_affine_march_rays(sid, mode, ref, o.ctypes.data_as(dp), o.ctypes.data_as(dp), 1, t.ctypes.data_as(dp), None),
            L.rm_affine_render(ctypes.byref(desc), mode, ref, d.ctypes.data_as(dp), h.ctypes.data, None, None)]


BAD_CONFIGS = [(f, v) for f in ("t_max", "tol", "h0", "growth", "h_max", "normal_eps") for v in (-1.0, float("nan"), float("inf"))] + \
    [("bound_radius", float("nan")), ("growth", 1.0), ("max_steps", -1), ("max_steps", _native.RM_INTERVAL_MAX_STEPS + 1), ("reserved", 1)]


@pytest.mark.parametrize("field,value", BAD_CONFIGS)
def test_bad_config(field, value):
    L = _native.load()
    cfg = _native.RmIntervalConfig()
    setattr(cfg, field, value)
    assert _calls(L, 0, AFFINE, cfg, with_range=False) == [_native.RM_E_BAD_ARG] * 2
    msg = L.rm_last_error().decode()
    assert "RmIntervalConfig" in msg and (field in msg or field == "reserved"), msg


@pytest.mark.parametrize("mode", [0, 3, -1, 99])
def test_bad_mode(mode):
    L = _native.load()
    assert _calls(L, 0, mode, None) == [_native.RM_E_BAD_ARG] * 3
    assert "mode" in L.rm_last_error().decode()


def test_meet_has_no_form():
    L = _native.load()
    segs, rng, form = np.zeros(8), np.empty(2), np.empty(3)
    rc = L.rm_affine_range_eval(0, MEET, segs.ctypes.data_as(dp), 1, rng.ctypes.data_as(dp), form.ctypes.data)
    assert rc == _native.RM_E_BAD_ARG
    assert "out_form" in L.rm_last_error().decode()


def test_error_order_and_no_device():
    """bad scene before bad argument before the device"""
    L = _native.load()
    bad = _native.RmIntervalConfig()
    bad.tol = -1.0
    for sid in (9, 10, 11, 15, 16, 18, 20, -1, 5000):
        assert _calls(L, sid, 7, bad) == [_native.RM_E_BAD_SCENE] * 3, sid
    assert _calls(L, 3, 7, None) == [_native.RM_E_BAD_ARG] * 3
    desc = _native.make_desc(0, 0, np.zeros(14), 4, 4)
    assert L.rm_affine_render(None, AFFINE, None, None, None, None, None) == _native.RM_E_BAD_ARG
    desc.rows = 9                                          # a slice outside the frame: still before the device
    assert L.rm_affine_render(ctypes.byref(desc), AFFINE, None, None, None, None, None) == -3      # RM_E_BAD_DIMS
    # every call that passes the host checks needs a device, n == 0 included: a fresh process that never called rm_init
    code = (
        "import ctypes, numpy as np\n"
        "from raymarch_algo_compare_amd import _native\n"
        "L = _native.load(); dp = ctypes.POINTER(ctypes.c_double)\n"
        "o = np.zeros(8); t = np.empty(4); d = np.empty(16); h = np.empty(16, np.uint8)\n"
        "desc = _native.make_desc(3, 0, np.zeros(14), 4, 4)\n"
        "for mode in (1, 2):\n"
        "    print(L.rm_affine_range_eval(0, mode, o.ctypes.data_as(dp), 1, t.ctypes.data_as(dp), None),"
        " L.rm_affine_march_rays(0, mode, None, o.ctypes.data_as(dp), o.ctypes.data_as(dp), 1, t.ctypes.data_as(dp), None),"
        " L.rm_affine_render(ctypes.byref(desc), mode, None, d.ctypes.data_as(dp), h.ctypes.data, None, None),"
        " L.rm_affine_march_rays(0, mode, None, None, None, 0, None, None))\n")
    env = dict(os.environ, PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, check=True, capture_output=True, text=True).stdout
    assert [int(x) for x in out.split()] == [_native.RM_E_NO_DEVICE] * 8, out


# ---- 5. the code object ------------------------------------------------------------------------------------------------------

OBJ = os.path.join(ROOT, "raymarch_algo_compare_amd", "_build", "affine.o")


def test_code_object_no_scratch_no_spills():
    """as test_segment_host does for segment.o"""
    import importlib.util
    assert os.path.exists(OBJ), "affine.o is missing: build the library (make -C raymarch_algo_compare_amd/csrc)"
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    kernels = [k for k in tool.collect([OBJ]) if "_kernel" in k["demangled"]]
    assert sorted(re.search(r"\w+_kernel", k["demangled"]).group(0) for k in kernels) == \
        ["affine_march_kernel", "affine_range_kernel", "affine_render_kernel"]
    found = tool.matching_instructions(OBJ, r"\b(scratch|buffer)_")
    for k in kernels:
        assert found.get(k["name"]) == [], (k["demangled"], found.get(k["name"], "not disassembled")[:4])
        assert k["vgpr_spill_count"] == 0, k["demangled"]
        assert k["private_segment_fixed_size"] == 0, k["demangled"]
