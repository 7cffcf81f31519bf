"""Ray sets for the common-path layout of the team forms (csrc/rm_math_trig.h ONE RARE-PATH TEST PER CALL), used by
tests/test_gpu_common_path.py -- a plain module.  Rays come from tests/short_last_trip_cases.py (crawler_rays,
mixed_rays, by_trip_count) and are classified on the CPU by tests/native/common_path_check.cpp, which marches them
through the evaluation as a team steps it and reports, per ray, the evaluation at which each rare band is first met."""
import ctypes
import functools

import numpy as np

import short_last_trip_cases as C

KINDS = ["acos", "sincos", "do_sin", "atan2_entry", "atan2_form", "acos_taylor", "acos_sqrt", "sincos_r2", "atan2_series",
         "atan2_case_i", "root_guard"]
# what a two-lane wave must be made to meet: each sends the wave to a general body (or to the full pow behind the guard)
RARE = ["acos_taylor", "acos_sqrt", "sincos_r2", "atan2_series", "atan2_case_i", "do_sin", "root_guard"]


@functools.lru_cache(maxsize=None)
def native():
    from conftest import build_native
    lib = ctypes.CDLL(build_native("common_path_check"))
    assert lib.cp_kinds() == len(KINDS)
    lib.cp_march.restype = None
    return lib


def classify(o, d, max_iterations=512, hit_threshold=1e-4, max_distance=100.0):
    """(hit, t, iterations, final_sdf, first): the rays marched by the host build of the team evaluation; first[i, k] is
    the evaluation of ray i that first meets KINDS[k], -1 if none does"""
    o = np.ascontiguousarray(o, np.float64).reshape(-1, 3)
    d = np.ascontiguousarray(d, np.float64).reshape(-1, 3)
    n = len(o)
    hit, t, it, fs = np.empty(n, np.uint8), np.empty(n), np.empty(n, np.int32), np.empty(n)
    first = np.empty((n, len(KINDS)), np.int32)
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    native().cp_march(int(max_iterations), ctypes.c_double(hit_threshold), ctypes.c_double(max_distance), o.ctypes.data_as(dp),
                      d.ctypes.data_as(dp), ctypes.c_size_t(n), hit.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                      t.ctypes.data_as(dp), it.ctypes.data_as(ip), fs.ctypes.data_as(dp), first.ctypes.data_as(ip))
    return hit, t, it, fs, first


@functools.lru_cache(maxsize=None)
def pool():
    """(origins, directions, iterations, first) of every ray the sets are drawn from"""
    by = C.by_trip_count()
    rng = np.random.default_rng(505)
    pts = np.concatenate([by[k][:40] for k in range(1, 9)])
    parts = [C.crawler_rays(64), C.mixed_rays(197, 2197), (pts, rng.normal(0.0, 0.35, pts.shape) - pts)]
    o, d = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    _, _, it, _, first = classify(o, d)
    return o, d, it, first


def lone_rays():
    """[(origin, direction)] for a wave of ONE live lane: the longest ray of the pool"""
    o, d, it, first = pool()
    k = np.argmax(it)
    return [(o[k:k + 1], d[k:k + 1])]


def pair_for(kind):
    """two rays for one team: lane 0 meets `kind` at evaluation e, lane 1 never meets it and is still marching at e, so
    the wave takes the general body there while lane 1 is in the common band.  Returns (origins, directions, e)."""
    o, d, it, first = pool()
    col = first[:, KINDS.index(kind)]
    rare = np.flatnonzero(col >= 0)
    plain = np.flatnonzero(col < 0)
    assert len(rare) and len(plain), (kind, len(rare), len(plain))
    rare = rare[np.argsort(col[rare], kind="stable")]
    for r in rare:
        ok = plain[it[plain] > col[r]]
        if len(ok):
            p = ok[np.argmax(it[ok])]
            return o[[r, p]], d[[r, p]], int(col[r])
    raise AssertionError(f"no pair for {kind}")


def kinds_met(first):
    return {k: int((first[:, i] >= 0).sum()) for i, k in enumerate(KINDS)}
