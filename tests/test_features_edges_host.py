"""The edge cases of the discovery features (tests/features_edge_cases.py) without a GPU: every case through the host build of
csrc/rm_features.h (tests/native/features_check.cpp) over the CPU oracle's point evaluation, against the NumPy expectations
the case module states -- and the conditions the cases rest on, asserted over the oracle.  This is what shows that the
cases are right and that the reference's expressions alone meet them; tests/test_gpu_features_edges.py gives the device
the same cases and the same assertions.

The host build's radix select is a plain sort (features_check.cpp), so the select cases prove the cases here and the
kernel there."""
import ctypes

import numpy as np
import pytest

import features_cases as C
import features_edge_cases as E
from oracle import oracle
from raymarch_algo_compare_amd import _native, features


@pytest.fixture(scope="module")
def host():
    return C.Host()


@pytest.fixture(scope="module")
def run_intrinsic(host):
    def run(scene_id, sets):
        return host.intrinsic(sets, oracle.sdf_eval(scene_id, host.points(sets)))
    return run


@pytest.fixture(scope="module")
def run_view(host):
    def run(captures, cameras):
        return [host.view(cap, cam.params14()) for cap, cam in zip(captures, cameras)]
    return run


# ---- the conditions of the cases ------------------------------------------------------------------------------------------------

def test_run_cases_give_the_intended_inside_flags():
    E.check_run_conditions(oracle.sdf_eval)
    sets, flags = E.mixed_batch()
    assert E.MIXED_CHORDS >= 70 and len(sets) == E.MIXED_SETS
    for s, f in zip(sets, flags):
        for c in range(E.MIXED_CHORDS):
            a, b = s["chords"][c, :3], s["chords"][c, 3:]
            assert np.array_equal(oracle.sdf_eval(E.SPHERE, a[None, :] + s["ts"][:, None] * (b - a)[None, :]) < 0.0, f[c]), c
        kinds = {tuple(c) for c in s["chords"]}
        assert len(kinds) == 4 and len(np.unique(s["seglen"])) == E.MIXED_CHORDS


def test_median_cases_have_the_structure_they_claim():
    E.check_median_conditions()


def test_p99_cases_have_the_structure_they_claim():
    E.check_p99_conditions(oracle.sdf_eval)


# ---- the cases through the host build ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("steps", E.RUN_STEPS)
def test_runs(run_intrinsic, steps):
    E.check_runs(run_intrinsic, steps)


def test_every_chord_s_block_sits_at_its_own_offset(run_intrinsic):
    E.check_mixed_batch(run_intrinsic)


@pytest.mark.parametrize("n", E.MEDIAN_N)
def test_median(run_intrinsic, n):
    E.check_median(run_intrinsic, n)


def test_median_with_two_slots_per_chord(run_intrinsic):
    for n in (3, 101, 257):
        E.check_median(run_intrinsic, n, steps=3)


@pytest.mark.parametrize("scene", E.P99_SCENES)
@pytest.mark.parametrize("n", E.P99_N)
def test_p99(run_intrinsic, scene, n):
    E.check_lip_sets(run_intrinsic, scene, E.p99_case(scene, n, oracle.sdf_eval))


@pytest.mark.parametrize("scene", E.LEFT_OUT_SCENES)
def test_p99_with_points_left_out(run_intrinsic, scene):
    for n in E.LEFT_OUT_N:
        E.check_lip_sets(run_intrinsic, scene, E.left_out_case(scene, n, oracle.sdf_eval))


@pytest.mark.parametrize("w,h", E.VIEW_SHAPES)
def test_view_masks(run_view, host, w, h):
    E.check_views(run_view, host, E.view_mask_cases(w, h))


def test_view_values(run_view, host):
    cases = E.view_value_cases()
    for shape in sorted({c[1]["hit"].shape for c in cases}):
        E.check_views(run_view, host, [c for c in cases if c[1]["hit"].shape == shape])


def test_view_non_finite_depth(run_view, host):
    """a box axis with a NaN hit coordinate is NaN in both corners wherever the pixel sits; NumPy's min / max say the same"""
    E.check_views(run_view, host, E.view_depth_cases())


def test_evals_count_by_hand(host):
    """feat_evals_count: NaN and negatives 0, above 2^24 2^24, truncation between; a count keeps every bit"""
    cam = C.camera(4, 2)
    for v, count in ((np.nan, 0), (-1.0, 0), (-1e-30, 0), (0.0, 0), (0.99, 0), (1.0, 1), (2.5, 2), (16777215.0, 16777215), (16777216.0, 16777216),
                     (16777218.0, 16777216), (3e38, 16777216), (np.inf, 16777216), (-np.inf, 0)):
        cap = C.capture_of(np.ones((2, 4), bool), 1)
        cap["evals"][:] = v
        got = host.view(cap, cam.params14())
        assert got["sum_evals"] == 8 * count and got["hardness_mean"] == float(count) and got["hardness_cv"] == 0.0, (v, got)
        with np.errstate(all="ignore"):
            want = features.view_features_numpy(cap, cam)
        assert (want["sum_evals"], want["hardness_mean"], want["hardness_cv"]) == (8 * count, float(count), 0.0), (v, want)


def test_hit_bytes_other_than_one(host):
    """the ABI's "non-zero = hit": bytes 2 and 255 count as 1 does"""
    cap, cam = C.capture_of((np.arange(33 * 9).reshape(9, 33) * 7) % 3 != 0, 31), C.camera(33, 9)
    want = host.view(cap, cam.params14())
    maps, keep = _native.view_maps(cap, 33, 9)
    raw = np.where(keep[3] != 0, np.where(np.arange(33 * 9).reshape(9, 33) % 2 == 0, 2, 255), 0).astype(np.uint8)
    res = _native.RmViewFeatures()
    cam14 = np.ascontiguousarray(cam.params14(), np.float64)
    assert host.L.rmft_view(33, 9, cam14.ctypes.data_as(C.dp), maps.depth, maps.normal, maps.evals, raw.ctypes.data_as(C.u8p), ctypes.byref(res)) == 0
    got = {k: getattr(res, k) for k, _ in _native.RmViewFeatures._fields_[:9]}
    got["box_lo"], got["box_hi"] = np.array(res.box_lo[:]), np.array(res.box_hi[:])
    assert {2, 255} <= set(raw.ravel().tolist()) and want["n_hit"] == int((raw != 0).sum())
    C.same_view(got, want, "hit bytes 2 and 255")


def test_many_views_are_distinct():
    caps, cams = E.many_views(130)
    assert len({c["hit"].tobytes() + c["depth"].tobytes() for c in caps}) == 130
    assert len({cam.params14().tobytes() for cam in cams}) == 130
