"""The edge cases of the discovery features (tests/features_edge_cases.py) on the MI355X: the kernels of csrc/rm_features.hip
that no host build runs -- feat_chord_kernel's ballots, carries across chunks and LDS slots at every chord_steps of the host
list, feat_select_kernel's radix select at every rank edge with ties, single-byte and top-byte keys and kScoreNoKey slots,
the view kernels at tile-multiple frames, 65 and 130 views, hit bytes other than 1 -- with the assertions of
tests/test_features_edges_host.py: intrinsic results and gmag bit for bit against NumPy over the oracle's values, view
features bit for bit against the host build and against NumPy by check_view_against_numpy's rule.  The two definitions the
header adds (a NaN hit coordinate makes its box axis NaN wherever the pixel sits; evals are counts in [0, 2^24]) are pinned
between the host build and the device here."""
import ctypes

import numpy as np
import pytest

import features_cases as C
import features_edge_cases as E
from oracle import oracle
from raymarch_algo_compare_amd import _native, features

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host():
    return C.Host()


@pytest.fixture(scope="module")
def run_intrinsic(hip):
    def run(scene_id, sets):
        return [(r, r["gmag"], r["slab_counts"]) for r in features.intrinsic_features_device(scene_id, sets, details=True)]
    return run


@pytest.fixture(scope="module")
def run_view(hip):
    def run(captures, cameras):
        return _native.view_features(np.stack([cam.params14() for cam in cameras]), captures)
    return run


# ---- intrinsic ------------------------------------------------------------------------------------------------------------------

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


def test_a_refused_seglen_reaches_no_kernel(hip):
    s = dict(E.mixed_batch()[0][0])
    for i, v in ((0, np.nan), (74, -1.0)):
        seglen = s["seglen"].copy()
        seglen[i] = v
        with pytest.raises(_native.RmError) as e:
            features.intrinsic_features_device(E.SPHERE, [dict(s, seglen=seglen)])
        assert e.value.code == _native.RM_E_BAD_ARG and f"seglen[{i}]" in str(e.value)
    seglen = s["seglen"].copy()
    seglen[3] = np.inf                                        # a length: every run of chord 3 is +inf long
    r = features.intrinsic_features_device(E.SPHERE, [dict(s, seglen=seglen)], details=True)[0]
    assert np.array_equal(r["slab_counts"], E.expected_runs(E.mixed_batch()[1][0], seglen)[0])
    assert C.bits(r["slab_median"])[0] == E.expected_runs(E.mixed_batch()[1][0], seglen)[1]


# ---- view -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", E.VIEW_SHAPES)
def test_view_masks(run_view, host, w, h):
    E.check_views(run_view, host, E.view_mask_cases(w, h))


def test_view_values(run_view, host):
    cases = E.view_value_cases()
    for shape in sorted({c[1]["hit"].shape for c in cases}):
        E.check_views(run_view, host, [c for c in cases if c[1]["hit"].shape == shape])


def test_view_non_finite_depth(run_view, host):
    """a box axis with a NaN hit coordinate is NaN in both corners wherever the pixel sits -- lane 0, where a fold by halves
    that keeps its left operand on a false comparison kept the NaN, and every other lane, where it dropped it"""
    E.check_views(run_view, host, E.view_depth_cases())


def test_many_views(run_view, host):
    """view_finish_kernel handles one view per thread of 64-thread workgroups: 64, 65 and 130 views, each equal to the same
    view alone and to the host build"""
    caps, cams = E.many_views(130)
    alone = [run_view([cap], [cam])[0] for cap, cam in zip(caps, cams)]
    for v, (cap, cam) in enumerate(zip(caps, cams)):
        C.same_view(alone[v], host.view(cap, cam.params14()), f"view {v} alone")
    assert len({(a["n_hit"], a["sum_evals"], a["box_lo"].tobytes()) for a in alone}) == 130
    for n in (64, 65, 130):
        batch = run_view(caps[:n], cams[:n])
        assert len(batch) == n
        for v in range(n):
            C.same_view(batch[v], alone[v], f"view {v} of {n}")


def test_hit_bytes_other_than_one(hip, host):
    """the ABI's "non-zero = hit" through a raw rm_view_features call: bytes 2 and 255 count as 1 does"""
    cap, cam = C.capture_of((np.arange(33 * 9).reshape(9, 33) * 7) % 3 != 0, 31), C.camera(33, 9)
    want = _native.view_features(cam.params14()[None], [cap])[0]
    maps, keep = _native.view_maps(cap, 33, 9)
    raw = np.where(keep[3] != 0, np.where(np.arange(33 * 9).reshape(9, 33) % 2 == 0, 2, 255), 0).astype(np.uint8)
    assert {2, 255} <= set(raw.ravel().tolist()) and want["n_hit"] == int((raw != 0).sum())
    maps.hit = raw.ctypes.data
    res = _native.RmViewFeatures()
    cam14 = np.ascontiguousarray(cam.params14(), np.float64)
    _native.check(hip.load().rm_view_features(33, 9, 1, cam14.ctypes.data_as(C.dp), ctypes.byref(maps), ctypes.byref(res), None))
    got = {k: getattr(res, k) for k, _ in _native.RmViewFeatures._fields_[:9]}
    got["box_lo"], got["box_hi"] = np.array(res.box_lo[:]), np.array(res.box_hi[:])
    C.same_view(got, want, "hit bytes 2 and 255")
    C.same_view(got, host.view(cap, cam.params14()), "hit bytes 2 and 255, host")
