"""rm_shutdown() then rm_init() on the same device: the library comes back with nothing left over from its first life.
A default frame, a single-launch frame that parks rays, a scene-program frame, explicit rays, the rays of the five sound
tracers, two segment ranges, a capture and its SSIM scores, capture scores and view features against itself, and one
set of intrinsic features give bit-identical arrays and statistics before and after the restart; a program registered
before the shutdown is still registered after it (its device copy is made again).  So do the frames that go through
what the frame engine (csrc/rm_frame.hip) keeps from one frame to the next: two single-launch frames in a row ordered by
tile costs (the second by the first one's), a frame with pass timing on (the same number of passes) and a traced
single-launch frame (the same number of records), whose longest ray ran past the second budget, so that the team kernel
and its side stream were used in both lives."""
import ctypes

import numpy as np
import pytest

import features_cases
from raymarch_algo_compare_amd import _native, features, registry
from raymarch_algo_compare_amd import scene_program as sp
from raymarch_algo_compare_amd.camera import Camera

pytestmark = pytest.mark.gpu

W, H = 96, 64
EXACT_SCENE = 6   # a catalogue scene with an exact form (rm_exact_supported)


def _cam(sid):
    s = registry.SCENES[sid]
    return Camera(s.camera_position or (0.0, 0.0, 5.0), s.camera_target or (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 60.0, W, H).params14()


def _rays(n=192):
    """a fan of rays from (0, 0, 3.5) towards the origin's neighbourhood: hits, grazes and misses"""
    u = np.linspace(-0.6, 0.6, n)
    d = np.stack([u, 0.35 * np.sin(7.0 * u), -np.ones(n)], axis=1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.tile([0.0, 0.0, 3.5], (n, 1)), d


def _round(hip, program):
    """every call once; {name: array or statistics dict}"""
    out = {}
    want = dict(want_t_raw=True, want_final_sdf=True, want_block_var=True, want_evals=True)
    frames = {
        "default": hip.make_desc(10, 0, _cam(10), W, H, full=True),
        "single launch": hip.make_desc(10, 4, _cam(10), W, H, full=True, pipeline=2, suspend_after=(6, 40), tile_order_mode=2),
        "program": hip.make_desc(program, 0, _cam(12), W, H, full=True, lipschitz=registry.SCENES[12].lipschitz or 1.0),
    }
    for name, desc in frames.items():
        r = hip.render(desc, **want)
        for k in ("depth", "iters", "hit", "t_raw", "final_sdf", "block_var", "evals"):
            out[f"{name}: {k}"] = r[k]
        out[f"{name}: stats"] = r["stats"]
    maps = ("depth", "iters", "hit", "t_raw", "final_sdf", "block_var", "evals", "stats")
    L = hip.load()
    # the longest-first tile order: the first frame leaves its tile costs, the second is ordered by them
    ordered = hip.make_desc(10, 4, _cam(10), W, H, full=True, pipeline=2, suspend_after=(6, 40), tile_order_mode=1)
    for turn in ("first", "second"):
        r = hip.render(ordered, **want)
        out.update({f"ordered by costs, {turn}: {k}": r[k] for k in maps})
    # pass timing: a frame of three launches, after two single launches in the same queues
    hip.check(L.rm_set_pass_timing(1))
    try:
        r = hip.render(hip.make_desc(10, 4, _cam(10), W, H, full=True, pipeline=1, suspend_after=(6, 40)), **want)
        n, ms = ctypes.c_int32(0), (ctypes.c_float * 4)()
        hip.check(L.rm_get_pass_ms(None, ctypes.byref(n), ms))
    finally:
        hip.check(L.rm_set_pass_timing(0))
    out.update({f"pass timing: {k}": r[k] for k in maps})
    out["pass timing: passes"] = np.array([n.value])
    # the development trace: one record per ray a team finished (no early hand-over: the rays beyond the second budget)
    hip.check(L.rm_debug_set_trace(1))
    try:
        r = hip.render(hip.make_desc(10, 4, _cam(10), W, H, full=True, pipeline=2, suspend_after=(6, 40), early_handover=-1), **want)
        nrec = ctypes.c_int64(0)
        hip.check(L.rm_debug_get_trace(None, 0, ctypes.byref(nrec), None, None, 0, None))
    finally:
        hip.check(L.rm_debug_set_trace(0))
    out.update({f"traced: {k}": r[k] for k in maps})
    out["traced: records"] = np.array([nrec.value])
    o, d = _rays()
    for k, v in zip(("hit", "t", "iters", "final_sdf"), hip.march_rays(10, 0, o, d)):
        out[f"march_rays: {k}"] = v
    for k, v in zip(("t", "steps", "normals"), hip.interval_march_rays(0, o, d)):
        out[f"interval_march_rays: {k}"] = v
    # the subsystems whose workspace buffers are declared next to their kernels, not where rm_shutdown lives
    for k, v in zip(("t", "normals", "leaf"), hip.exact_march_rays(EXACT_SCENE, o, d)):
        out[f"exact_march_rays: {k}"] = v
    for k, v in zip(("t", "iters", "cursor"), hip.segment_march_rays(0, o, d)):
        out[f"segment_march_rays: {k}"] = v
    for k, v in zip(("t_lo", "t_hi", "status", "steps"), hip.certify_march_rays(0, o, d)):
        out[f"certify_march_rays: {k}"] = v
    for k, v in zip(("t", "steps"), hip.affine_march_rays(0, o, d)):
        out[f"affine_march_rays: {k}"] = v
    segs = np.concatenate([o[::32], d[::32], np.full((6, 1), 0.5), np.linspace(1.0, 4.0, 6)[:, None]], axis=1)
    out["affine_range_eval: range"], out["affine_range_eval: form"] = hip.affine_range_eval(0, segs)
    out["segment_sdf_eval"] = hip.segment_sdf_eval(0, segs)
    cap = hip.capture(frames["default"])
    for k in ("geom", "normal", "depth", "color", "evals", "hit"):
        out[f"capture: {k}"] = cap[k]
    out["capture: stats"] = cap["stats"]
    out["ssim_scores"] = hip.ssim_scores(W, H, cap, [cap])
    out["score_captures"] = _values(hip.score_captures(W, H, cap, [cap])[0])
    out["view_features"] = _values(hip.view_features(_cam(10)[None], [cap])[0])
    _, case = min(features_cases.fixture_cases(), key=lambda c: c[1]["n_lip"] + c[1]["n_chords"] * c[1]["steps"])
    r = features.intrinsic_features_device(case["scene"], [case["set"]], details=True)[0]
    out["intrinsic_features: gmag"], out["intrinsic_features: slab_counts"] = r.pop("gmag"), r.pop("slab_counts")
    out["intrinsic_features"] = _values(r)
    return out


def _values(fields):
    """a result dict's numbers (scalars and small arrays) as one float64 array, for the comparison of bits"""
    return np.concatenate([np.atleast_1d(np.asarray(fields[k], np.float64)) for k in sorted(fields)])


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_the_library_restarts_clean(hip):
    L = hip.load()
    arr, n = sp.to_ctypes(sp.catalogue_expressions()[12])
    program = hip.scene_program_create(arr, n, registry.SCENES[12].lipschitz or 1.0)
    try:
        first = _round(hip, program)
        assert first["single launch: stats"]["total_rays"] == W * H and first["default: stats"]["hit_count"] > 0
        # some ray ran past the second budget: teams finished it, on the stream of the library's own
        assert first["traced: stats"]["iter_max"] > 40 and first["traced: records"][0] > 0
        assert first["pass timing: passes"][0] == 3
        device = _native._device
        L.rm_shutdown()
        _native._device = None                          # what _native.init does on a device switch
        assert L.rm_sdf_eval(0, None, 0, None) == -4    # really down: RM_E_NO_DEVICE
        hip.init(device)                                # ... and up again, for this test and the ones that follow
        second = _round(hip, program)
    finally:
        if _native._device is None:
            hip.init()
        hip.scene_program_destroy(program)
    assert first.keys() == second.keys()
    for name, a in first.items():
        b = second[name]
        if isinstance(a, dict):
            assert a.keys() == b.keys(), name
            for k in a:
                assert np.array_equal(a[k], b[k]), (name, k)
        else:
            assert _same_bits(a, b), name
