"""The short last trip of the Mandelbulb evaluation on the host (rm_scenes.h THE SHORT LAST TRIP): SceneMandelbulb::sdf(),
whose eighth trip only updates dr, against the same evaluation run to completion through begin / trip / value with all
eight trips as full passes, and against the oracle -- bit for bit.  No GPU."""
import numpy as np

import short_last_trip_cases as C


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _check(pts):
    from oracle import oracle
    short = C.short_eval(pts)
    full, trips, _ = C.full_eval(pts)
    stepped, stepped_trips = C.stepped_eval(pts)
    assert np.array_equal(_bits(short), _bits(full)), int((_bits(short) != _bits(full)).sum())
    assert np.array_equal(_bits(stepped), _bits(full)) and np.array_equal(stepped_trips, trips)     # e.i still ends at 8
    assert np.array_equal(_bits(short), _bits(oracle.sdf_eval(10, pts)))
    return trips


def test_every_trip_count():
    by = C.by_trip_count()
    for k in range(1, 9):
        assert len(by[k]) >= 200
        assert (_check(by[k]) == k).all(), k


def test_eight_trip_points_near_the_surface():
    pts = C.near_surface()
    assert len(pts) >= 2000
    full, trips, _ = C.full_eval(pts)
    assert (trips == 8).all() and (np.abs(full) < C.SURFACE_EPS).all()
    _check(pts)


def test_last_trip_radius_near_zero_one_and_four():
    """the argument of the pow the short trip keeps, at the ends of its range and around 1 (where log r changes sign)"""
    e = C.edge_points()
    for name, lo, hi in (("zero", 0.0, 1e-2), ("one", 1.0 - 1e-2, 1.0 + 1e-2), ("four", 3.9, 4.0)):
        _, trips, r = C.full_eval(e[name])
        assert (trips == 8).all() and (r >= lo).all() and (r <= hi).all(), (name, float(r.min()), float(r.max()))
        _check(e[name])
    _, _, r0 = C.full_eval(e["zero"])
    assert (r0 == 0.0).any() and (r0 > 0.0).any()
    trips = _check(e["begin"])                  # first r: exactly 1 and 4, their neighbours, and a few ulps around both
    assert (trips == 0).any() and (trips >= 1).any()


def test_crawler_set_has_long_rays():
    """The GPU test's crawler rays, from the oracle's side: rays of >= 200 iterations at every size it runs, for both
    strategies.  A ray that crawls along the Mandelbulb steps from one side of the surface to the other (|d| never falls
    below the threshold), and only the evaluations on the inner side run all eight trips: about every second one.  A
    team's loop runs as many trips as its slowest lane, so what the short last trip sees is the share of a set's STEPS
    in which some live ray takes eight trips: most of them, from 17 rays on."""
    from oracle import oracle
    for n in (1, 17, 64, 197):
        o, d = C.crawler_rays(n)
        for kid in (0, 4):
            it = oracle.march_rays(10, kid, o, d)[2]
            assert (it >= 200).any(), (n, kid, int(it.max()))
        its, trips = C.trace_standard(o, d)
        steps = (trips >= 0).any(axis=0)
        eight = (trips == 8).any(axis=0)
        print(n, "eight-trip evaluations", float((trips == 8).sum() / its.sum()), "eight-trip steps", float(eight.sum() / steps.sum()))
        assert (trips == 8).sum() >= 0.45 * its.sum(), n
        assert eight.sum() >= 0.5 * steps.sum(), n             # one ray alone: every second step
        assert n == 1 or eight.sum() >= 0.9 * steps.sum(), n   # a team's view from 17 rays on


def test_mixed_set_mixes_trip_counts_in_a_wave():
    o, _ = C.mixed_rays(64, 5)
    assert set(C.full_eval(o)[1].tolist()) == set(range(1, 9))
