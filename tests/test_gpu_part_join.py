"""The Mandelbulb's join per part on the GPU (csrc/rm_scenes.h THE JOIN PER PART: the atan2 wave of a team decides bail-out
from the squared length and takes the root once per evaluation): rm_march_rays(team=True) and a single-launch frame of
the Mandelbulb / Standard against the oracle, bit for bit on iterations, hit, raw t and final_sdf; a launch-per-pass
frame, whose resume_team_kernel keeps its join and must agree; and rm_bail4 itself on the device, band included
(rm_debug_bail4_eval, csrc/rm_math_check.hip) -- no constructible ray reaches the band.  At most 3 teams per call."""
import numpy as np
import pytest

import common_path_cases as P
import short_last_trip_cases as C
import part_join_cases as HOST

pytestmark = pytest.mark.gpu

W, H = 64, 48
_ref = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _check_rays(hip, o, d, what):
    from oracle import oracle
    assert len(o) <= 3 * 64
    rh, rt, ri, rf = oracle.march_rays(10, 0, o, d)
    hit, t, it, fs = hip.march_rays(10, 0, o, d, team=True)
    assert np.array_equal(it, ri) and np.array_equal(hit, rh), (what, int((it != ri).sum()))
    assert np.array_equal(_bits(t), _bits(rt)) and np.array_equal(_bits(fs), _bits(rf)), what
    return ri


def test_one_live_crawler(hip):
    """sparse loops with one live lane: the tail of a frame, the case the join per part is built for"""
    (o, d), = P.lone_rays()
    it = _check_rays(hip, o, d, "one lane")
    assert it[0] >= 200, int(it[0])


@pytest.mark.parametrize("n_live", [16, 17, 64])
def test_sparse_flag_on_and_off(hip, n_live):
    """16 lanes: the flag is on; 17 and 64 mixed lanes: the full loops.  Every set mixes the trip counts 1..8 in its
    first evaluations, so lanes leave the part-1 wave's loop at every trip, and holds rays that march on for long."""
    o, d = C.mixed_rays(n_live, 3000 + n_live)
    assert len(set(C.full_eval(o)[1].tolist())) >= 6
    it = _check_rays(hip, o, d, n_live)
    assert it.max() >= 50, int(it.max())


def _frame_ref():
    if "f" not in _ref:
        from oracle import oracle
        _ref["f"] = oracle.render(10, 0, C.frame_camera(W, H), W, H)
    return _ref["f"]


@pytest.mark.parametrize("pipeline", [2, 1])
def test_frames(hip, pipeline):
    """pipeline = 2: the single launch (pipeline_team_kernel, the new join); pipeline = 1: the parked rays are finished by
    resume_team_kernel, which did not change"""
    ref = _frame_ref()
    desc = hip.make_desc(10, 0, C.frame_camera(W, H), W, H, full=True, pipeline=pipeline, suspend_after=(2, 6))
    out = hip.render(desc, want_t_raw=True, want_final_sdf=True)
    assert np.array_equal(out["iters"], ref.iters) and np.array_equal(out["hit"], ref.hit), pipeline
    assert np.array_equal(_bits(out["t_raw"]), _bits(ref.t)) and np.array_equal(_bits(out["final_sdf"]), _bits(ref.final_sdf)), pipeline


MASKS = {"all": (1 << 64) - 1, "lane0": 1, "two": (1 << 9) | (1 << 50), "16": 0x1111111111111111}


@pytest.mark.parametrize("sparse", [True, False])
@pytest.mark.parametrize("mask_name", list(MASKS))
def test_decision_on_the_device_equals_the_host(hip, mask_name, sparse):
    """rm_bail4 and rm_bail4_band on the device against the host build, which tests/test_part_join_host.py holds to
    rm_pow and to libm: every double within 4096 ulps of 16.0, the band's edges, the ends of the range.  The elements go
    to the waves in order, so waves all below 16, all above the band, and straddling it (the wave-uniform test is taken by
    some lanes and not by others) all occur; with one and two live lanes the band lanes are alone in their waves."""
    s = HOST.decision_set()
    if MASKS[mask_name] != (1 << 64) - 1:                       # few lanes per wave: keep the launch small
        s = np.concatenate([HOST._f64(np.arange(HOST.SIXTEEN - 40, HOST.SIXTEEN + 41, dtype=np.uint64)), s[-40:]])
    dec, band = hip.debug_bail4_eval(s, sparse, lane_mask=MASKS[mask_name])
    ref_dec, ref_band, rm_gt, libm_gt = HOST.bail4(s, sparse)
    assert band.sum() >= 3 and np.array_equal(band, ref_band)
    bad = np.flatnonzero(dec != ref_dec)
    assert len(bad) == 0, [(float(s[i]).hex(), bool(dec[i])) for i in bad[:8]]
    assert np.array_equal(dec, rm_gt) and np.array_equal(dec, libm_gt)
    one_up = np.flatnonzero(_bits(s) == HOST.SIXTEEN + 1)
    assert len(one_up) and band[one_up].all() and not dec[one_up].any()
