"""rm_shutdown() then rm_init() on the same device: the library comes back with nothing left over from its first life.
A default frame, a single-launch frame that parks rays, a scene-program frame, explicit rays and interval rays give
bit-identical arrays and statistics before and after the restart; a program registered before the shutdown is still
registered after it (its device copy is made again)."""
import numpy as np
import pytest

from raymarch_algo_compare_amd import _native, registry
from raymarch_algo_compare_amd import scene_program as sp
from raymarch_algo_compare_amd.camera import Camera

pytestmark = pytest.mark.gpu

W, H = 96, 64


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
    o, d = _rays()
    for k, v in zip(("hit", "t", "iters", "final_sdf"), hip.march_rays(10, 0, o, d)):
        out[f"march_rays: {k}"] = v
    for k, v in zip(("t", "steps", "normals"), hip.interval_march_rays(0, o, d)):
        out[f"interval_march_rays: {k}"] = v
    return out


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_the_library_restarts_clean(hip):
    L = hip.load()
    arr, n = sp.to_ctypes(sp.catalogue_expressions()[12])
    program = hip.scene_program_create(arr, n, registry.SCENES[12].lipschitz or 1.0)
    try:
        first = _round(hip, program)
        assert first["single launch: stats"]["total_rays"] == W * H and first["default: stats"]["hit_count"] > 0
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
