"""The Mandelbulb's join per part on the host (csrc/rm_scenes.h THE JOIN PER PART), no GPU.

1. rm_bail4 (csrc/rm_math_pow.h), the bail-out decision from the squared length, equals `rm_pow(s, 0.5) > 4.0` and libm's
   `pow(s, 0.5) > 4.0` on every double within 4096 ulps of 16.0, at the band's edges and at the ends of the range.
2. An SDF evaluation in the form each wave of a team steps it (tests/native/part_join_check.cpp part_eval; part 1 keeps the
   squared length and takes the root once, behind the loops) ends with r, dr, i and value() bit-equal to
   SceneMandelbulb::sdf's, over the points the ray pools of tests/common_path_cases.py and
   tests/short_last_trip_cases.py evaluate."""
import ctypes
import functools

import numpy as np
import pytest

import common_path_cases as CP
import short_last_trip_cases as C

from part_join_cases import SIXTEEN, _f64, _p, _u64, around_sixteen, bail4, decision_set, native


@pytest.mark.parametrize("sparse", [True, False])
def test_decision_equals_the_roots_compare(sparse):
    s = decision_set()
    dec, band, rm_gt, libm_gt = bail4(s, sparse)
    assert np.array_equal(rm_gt, libm_gt)
    bad = np.flatnonzero(dec != rm_gt)
    assert len(bad) == 0, [(float(s[i]).hex(), bool(dec[i]), bool(rm_gt[i])) for i in bad[:8]]
    # both sides of the decision and of the band are in the set
    assert dec.any() and (~dec).any() and band.any() and (~band).any()
    assert not dec[np.isnan(s)].any() and dec[np.isinf(s)].all() and not dec[s == 0.0].any()


def test_band_is_entered_and_is_what_the_header_says():
    """16 + 1 ulp takes the root itself and answers false; the band is 16 + 1 .. 3 ulp and NaN, nothing else"""
    hi = native().pj_band_hi()
    assert int(_u64([hi])[0]) == SIXTEEN + 4
    one_up = _f64([SIXTEEN + 1])
    for sparse in (True, False):
        dec, band, rm_gt, libm_gt = bail4(one_up, sparse)
        assert band[0] and not dec[0] and not rm_gt[0] and not libm_gt[0]
    s = np.concatenate([around_sixteen(), [0.0, -0.0, 2.0 ** -60, 2.0 ** 60, np.inf, np.nan, -1.0]])
    _, band, _, _ = bail4(s, True)
    b = _u64(s)
    want = ((b > SIXTEEN) & (b < SIXTEEN + 4) & (s > 0)) | np.isnan(s)
    assert np.array_equal(band, want)
    # the two proven sides answer without the root: false up to 16.0, true from hi on
    dec, band, rm_gt, _ = bail4(_f64([SIXTEEN, SIXTEEN + 4, SIXTEEN + 2, SIXTEEN + 3]), True)
    assert list(band) == [False, False, True, True] and list(dec) == [False, True, True, True] and np.array_equal(dec, rm_gt)


# ---- the evaluation in each wave's form -----------------------------------------------------------------------------

def part_eval(part, sparse, pts):
    pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
    n = len(pts)
    r, dr, v = np.empty(n), np.empty(n), np.empty(n)
    it, ended, step = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.uint8)
    d, i32 = ctypes.c_double, ctypes.c_int32
    native().pj_part_eval(int(part), int(sparse), _p(pts, d), ctypes.c_size_t(n), _p(r, d), _p(dr, d), _p(it, i32), _p(v, d),
                          _p(ended, i32), _p(step, ctypes.c_uint8))
    return r, dr, it, v, ended, step


def sdf_eval(pts):
    pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
    n = len(pts)
    r, dr, v, sdf = np.empty(n), np.empty(n), np.empty(n), np.empty(n)
    it = np.empty(n, np.int32)
    d = ctypes.c_double
    native().pj_sdf(_p(pts, d), ctypes.c_size_t(n), _p(r, d), _p(dr, d), _p(it, ctypes.c_int32), _p(v, d), _p(sdf, d))
    return r, dr, it, v, sdf


def _ray_points(o, d, per_ray=40, max_iterations=512, hit_threshold=1e-4, max_distance=100.0):
    """the points the first `per_ray` evaluations of Standard sphere tracing visit on every ray (NumPy on top of the host
    evaluation: for the choice of points only)"""
    o = np.asarray(o, dtype=np.float64).reshape(-1, 3)
    unit = np.asarray(d, dtype=np.float64).reshape(-1, 3)
    unit = unit / np.linalg.norm(unit, axis=1, keepdims=True)
    t = np.zeros(len(o))
    live = np.arange(len(o))
    out = []
    for _ in range(per_ray):
        if not len(live):
            break
        p = o[live] + unit[live] * t[live][:, None]
        out.append(p)
        v = C.full_eval(p)[0]
        t[live] += v
        live = live[(np.abs(v) >= hit_threshold) & (t[live] <= max_distance)]
    return np.concatenate(out)


@functools.lru_cache(maxsize=None)
def pool():
    """evaluation points of the ray pools of tests/common_path_cases.py (crawlers, mixed rays, one ray per trip count) and
    every point set of tests/short_last_trip_cases.py"""
    o, d, _, _ = CP.pool()
    return np.concatenate([_ray_points(o, d), C.all_points()])


@pytest.fixture(scope="module")
def reference():
    return sdf_eval(pool())


def _bits_equal(a, b):
    return np.array_equal(_u64(a), _u64(b))


def test_pool_ends_every_way(reference):
    """ready at begin, bail-out in each of the trips 1..7, and ended by the count"""
    _, _, _, _, ended, _ = part_eval(1, True, pool())
    counts = {k: int((ended == k).sum()) for k in range(0, 9)}
    print("evaluations by the way they ended:", counts)
    assert all(counts[k] >= 20 for k in range(0, 9)), counts
    assert (ended >= 0).all()


@pytest.mark.parametrize("sparse", [True, False])
@pytest.mark.parametrize("part", [0, 1, 2])
def test_part_form_ends_where_sdf_ends(reference, part, sparse):
    r0, dr0, it0, v0, sdf0 = reference
    assert _bits_equal(v0, sdf0)
    r, dr, it, v, ended, step = part_eval(part, sparse, pool())
    assert step.all(), int((step == 0).sum())
    assert _bits_equal(r, r0), int((_u64(r) != _u64(r0)).sum())
    assert _bits_equal(dr, dr0) and np.array_equal(it, it0)
    assert _bits_equal(v, v0), int((_u64(v) != _u64(v0)).sum())
    assert np.array_equal(ended[ended > 0], it[ended > 0]) and (it[ended == 0] == 0).all()
