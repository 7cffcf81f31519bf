"""Shared by tests/test_strategy_program_host.py and tests/test_gpu_strategy_program.py: the g++ build of
csrc/rm_strategy_program.h (tests/native/strategy_program_check.cpp), the rays, and the five twins with the compiled
strategy and constructor arguments each is compared with."""
import ctypes

import numpy as np

from conftest import build_native
from raymarch_algo_compare_amd import _native, registry
from raymarch_algo_compare_amd import strategy_program as sp
from raymarch_algo_compare_amd.camera import Camera

# twin key -> (compiled strategy id, non-default constructor arguments of the twin, the same as RmStrategyParams names)
TWINS = {
    "Standard": (0, {}, {}),
    "Relaxed": (1, {"omega": 1.6}, {"omega": 1.6}),
    "Heuristic-Auto-Relaxed": (2, {"omega_max": 1.8, "decay_rate": 0.6}, {"ar_omega_max": 1.8, "ar_decay_rate": 0.6}),
    "Slope-Auto-Relaxed": (3, {"beta": 0.5}, {"beta": 0.5}),
    "Overstep-Bisect": (6, {"min_step_factor": 0.02, "bisection_steps": 9},
                        {"overstep_min_step": 0.02, "overstep_bisection_steps": 9}),
}
HOST_SCENES = [0, 6, 11, 12, 13]      # Sphere, Hollow Cube, Bad Lipschitz Sphere, Pillar Forest, Thin Planes Stack
CONFIGS = [(100, 1e-4, 100.0), (512, 1e-6, 100.0)]


def twin_cases():
    """(name, compiled id, program, RmStrategyParams overrides): every twin with its defaults and, where it has
    constructor arguments, once more with the non-default set"""
    out = []
    dflt = sp.strategy_twins()
    for key, (kid, ctor, prm) in TWINS.items():
        out.append((key, kid, dflt[key], {}))
        if ctor:
            out.append((key + "*", kid, sp.strategy_twins(**{key: ctor})[key], prm))
    return out


def rays(scene_id: int, n: int = 2000, seed: int = 7):
    """About half camera rays of the scene's own camera, half random rays towards the origin's neighbourhood."""
    scene = registry.SCENES[scene_id]
    W, H = 40, 25
    cam = Camera(scene.camera_position or (0.0, 0.0, 5.0), scene.camera_target or (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 60.0, W, H)
    o1, d1 = [], []
    f, r, u = (np.array(v) for v in (cam.forward, cam.right, cam.up))
    for y in range(H):
        for x in range(W):
            sx = ((x + 0.5) / W * 2.0 - 1.0) * cam.half_width
            sy = (1.0 - (y + 0.5) / H * 2.0) * cam.half_height
            o1.append(cam.position)
            d1.append(f + r * sx + u * sy)      # (not normalised: the marchers do that)
    rng = np.random.default_rng(seed + scene_id)
    m = max(n // 2, n - len(o1))
    keep = np.linspace(0, len(o1) - 1, n - m).astype(int)        # (all of them for n = 2000)
    o1, d1 = [o1[k] for k in keep], [d1[k] for k in keep]
    o2 = rng.normal(size=(m, 3)) * 4.0 + np.array([0.0, 1.0, 5.0])
    tgt = rng.normal(size=(m, 3)) * 1.2
    d2 = tgt - o2
    o = np.concatenate([np.asarray(o1, np.float64).reshape(-1, 3), o2])
    d = np.concatenate([np.asarray(d1, np.float64).reshape(-1, 3), d2])
    return np.ascontiguousarray(o), np.ascontiguousarray(d)


_dp = ctypes.POINTER(ctypes.c_double)


def native():
    L = ctypes.CDLL(build_native("strategy_program_check"))
    L.rsp_encode.argtypes = [ctypes.POINTER(_native.RmStrategyOp), ctypes.c_int32, ctypes.c_char_p, ctypes.c_size_t,
                             ctypes.POINTER(ctypes.c_int32)]
    L.rsp_march_rays.argtypes = [ctypes.c_int, ctypes.POINTER(_native.RmStrategyOp), ctypes.c_int32, ctypes.c_int,
                                 ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_int, _dp, _dp, ctypes.c_size_t,
                                 ctypes.POINTER(ctypes.c_uint8), _dp, ctypes.POINTER(ctypes.c_int32), _dp,
                                 ctypes.POINTER(ctypes.c_int32)]
    return L


def host_compiled():
    L = ctypes.CDLL(build_native("host_check"))
    L.rmh_march_rays.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                 ctypes.c_int, _dp, _dp, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint8), _dp,
                                 ctypes.POINTER(ctypes.c_int32), _dp, _dp]
    return L


def _outs(n):
    return np.empty(n, np.uint8), np.empty(n, np.float64), np.empty(n, np.int32), np.empty(n, np.float64)


def _p(a, ty):
    return a.ctypes.data_as(ctypes.POINTER(ty))


def march_program(L, scene, program, cfg, full, o, d):
    """g++ march_one<Scene, StratProgram>: dict like run_host's"""
    n = len(o)
    hit, t, it, fs = _outs(n)
    ev = np.empty(n, np.int32)
    rc = L.rsp_march_rays(scene, program.to_ops(), len(program), cfg[0], cfg[1], cfg[2], 1.0, int(full), _p(o, ctypes.c_double),
                          _p(d, ctypes.c_double), n, _p(hit, ctypes.c_uint8), _p(t, ctypes.c_double), _p(it, ctypes.c_int32),
                          _p(fs, ctypes.c_double), _p(ev, ctypes.c_int32))
    assert rc == 0, rc
    return {"hit": hit, "t": t, "iters": it, "final_sdf": fs, "evals": ev}


PARAM_ORDER18 = ["omega", "ar_omega_min", "ar_omega_max", "ar_smoothing", "ar_growth_rate", "ar_decay_rate", "beta",
                 "overstep_min_step", "hybrid_stuck_step_ratio", "hybrid_min_step", "margin", "ar_omega_init",
                 "overstep_bisection_steps", "hybrid_stuck_threshold", "segment_bisection_steps", "revaa_bisection_steps",
                 "step_scale", "dense_min_step"]
DEFAULTS18 = [1.2, 1.0, 2.0, 0.7, 1.05, 0.7, 0.3, 0.01, 0.001, 0.005, 0.05, 1.2, 16, 5, 8, 8, 1.0, 1e-4]


def march_compiled(L, scene, kid, prm, cfg, full, o, d):
    """g++ march_one<Scene, StratX> (tests/native/host_check.cpp)"""
    n = len(o)
    hit, t, it, fs = _outs(n)
    p18 = np.array([float(prm.get(k, v)) for k, v in zip(PARAM_ORDER18, DEFAULTS18)], np.float64)
    rc = L.rmh_march_rays(scene, kid, cfg[0], cfg[1], cfg[2], 1.0, int(full), _p(o, ctypes.c_double), _p(d, ctypes.c_double), n,
                          _p(hit, ctypes.c_uint8), _p(t, ctypes.c_double), _p(it, ctypes.c_int32), _p(fs, ctypes.c_double),
                          _p(p18, ctypes.c_double))
    assert rc == 0, rc
    return {"hit": hit, "t": t, "iters": it, "final_sdf": fs}


def same_bits(a, b, keys=("hit", "iters", "t", "final_sdf")):
    """names of the arrays that differ in any bit"""
    bad = []
    for k in keys:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        if x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes():
            bad.append(k)
    return bad
