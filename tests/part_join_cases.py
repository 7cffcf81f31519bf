"""Helpers and argument sets for the Mandelbulb's join per part (csrc/rm_scenes.h THE JOIN PER PART), shared by
tests/test_part_join_host.py and tests/test_gpu_part_join.py -- a plain module.  The host side is
tests/native/part_join_check.cpp."""
import ctypes
import functools

import numpy as np

ULPS = 4096


@functools.lru_cache(maxsize=None)
def native():
    from conftest import build_native
    L = ctypes.CDLL(build_native("part_join_check"))
    L.pj_bail4.restype = None
    L.pj_part_eval.restype = None
    L.pj_sdf.restype = None
    L.pj_band_hi.restype = ctypes.c_double
    return L


def _p(a, t):
    return a.ctypes.data_as(ctypes.POINTER(t))


def bail4(s, sparse):
    """(decision, in the band, rm_pow(s, 0.5) > 4.0, libm pow(s, 0.5) > 4.0) as bool arrays"""
    s = np.ascontiguousarray(s, dtype=np.float64).reshape(-1)
    out = [np.empty(len(s), np.uint8) for _ in range(4)]
    native().pj_bail4(_p(s, ctypes.c_double), ctypes.c_size_t(len(s)), int(sparse), *[_p(o, ctypes.c_uint8) for o in out])
    return [o != 0 for o in out]


def _u64(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _f64(b):
    return np.ascontiguousarray(b, dtype=np.uint64).view(np.float64)


def _nbrs(x, k=3):
    b = int(_u64([x])[0])
    return _f64(np.arange(b - k, b + k + 1, dtype=np.uint64))


SIXTEEN = int(_u64([16.0])[0])


def around_sixteen():
    """every double within ULPS ulps of 16.0, on either side"""
    return _f64(np.arange(SIXTEEN - ULPS, SIXTEEN + ULPS + 1, dtype=np.uint64))


def decision_set():
    """every double within ULPS ulps of 16.0, the band's edges and their neighbours, and the ends of the range"""
    hi = native().pj_band_hi()
    return np.concatenate([around_sixteen(), _nbrs(16.0), _nbrs(hi), [0.0, 2.0 ** -60, 2.0 ** 60, np.inf, np.nan],
                           _nbrs(2.0 ** -60), _nbrs(2.0 ** 60), [-0.0, 5e-324, 1.0, 15.0, 17.0, 1e300]])
