"""The common-path layout of the team forms on the GPU (csrc/rm_math_trig.h ONE RARE-PATH TEST PER CALL; the sparse flag
and the join from registers of csrc/rm_kernels.h team_trip): rm_march_rays(team=True) and a single-launch frame of the
Mandelbulb / Standard against the oracle, bit for bit: iterations, hit, raw t, final_sdf; and a launch-per-pass frame,
whose resume_team_kernel keeps the forms it had and must give the same frame.

Which body a wave takes depends on the lanes it holds, so the waves are laid out on the CPU (tests/common_path_cases.py,
from the host build of the team evaluation): one live lane; two live lanes of which one meets a rare band at a known
evaluation while the other, still marching, never meets it; 16 live lanes (the sparse flag is on), 17 and 64 (off).
That the sets do what they are chosen for is asserted here on the CPU side, so the test cannot pass by never leaving
the common path.  At most 3 teams per call."""
import numpy as np
import pytest

import common_path_cases as P
import short_last_trip_cases as C

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


def test_the_host_classification_marches_as_the_oracle_does():
    """what the sets are chosen by: the host build of the team evaluation gives the oracle's rays bit for bit, and the
    pool meets every band the sets are drawn for (and none is off the plain path of atan2: no such ray exists here)"""
    from oracle import oracle
    o, d, it, first = P.pool()
    rh, rt, ri, rf = oracle.march_rays(10, 0, o, d)
    h, t, i2, fs, _ = P.classify(o, d)
    assert np.array_equal(i2, ri) and np.array_equal(h, rh)
    assert np.array_equal(_bits(t), _bits(rt)) and np.array_equal(_bits(fs), _bits(rf))
    met = P.kinds_met(first)
    assert all(met[k] > 0 for k in P.RARE), met
    assert met["atan2_entry"] == 0, met


def test_one_live_lane(hip):
    for o, d in P.lone_rays():
        _, _, it, _, first = P.classify(o, d)
        assert it[0] >= 200, int(it[0])                       # a long ray alone in its team: the frame's critical case
        _check_rays(hip, o, d, "one lane")


@pytest.mark.parametrize("kind", P.RARE)
def test_two_live_lanes_one_in_a_rare_band(hip, kind):
    o, d, e = P.pair_for(kind)
    _, _, it, _, first = P.classify(o, d)
    k = P.KINDS.index(kind)
    assert first[0, k] == e and first[1, k] < 0 and it[1] > e, (kind, first[:, k], it)
    _check_rays(hip, o, d, kind)


@pytest.mark.parametrize("n_live", [16, 17, 64])
@pytest.mark.parametrize("rays", ["mixed", "crawler"])
def test_sparse_flag_on_and_off(hip, rays, n_live):
    o, d = C.mixed_rays(n_live, 3000 + n_live) if rays == "mixed" else C.crawler_rays(n_live)
    first = P.classify(o, d)[4]
    assert P.kinds_met(first)["root_guard"] > 0                # some root fails its guard: with the flag on the full pow stands in
    _check_rays(hip, o, d, (rays, n_live))


def _frame_ref():
    if "f" not in _ref:
        from oracle import oracle
        cam = C.frame_camera(W, H)
        o, dirs = C.frame_rays(cam, W, H)
        first = P.classify(np.broadcast_to(o, (W * H, 3)), dirs.reshape(-1, 3))[4]
        _ref["f"] = (oracle.render(10, 0, cam, W, H), P.kinds_met(first))
    return _ref["f"]


@pytest.mark.parametrize("pipeline", [2, 1])
def test_frames(hip, pipeline):
    """pipeline = 2: the single launch (pipeline_team_kernel); pipeline = 1: the parked rays are finished by
    resume_team_kernel.  The frame's rays meet every rare band (CPU)."""
    ref, met = _frame_ref()
    assert all(met[k] > 0 for k in P.RARE), met
    desc = hip.make_desc(10, 0, C.frame_camera(W, H), W, H, full=True, pipeline=pipeline, suspend_after=(2, 6))
    out = hip.render(desc, want_t_raw=True, want_final_sdf=True)
    assert np.array_equal(out["iters"], ref.iters) and np.array_equal(out["hit"], ref.hit), pipeline
    assert np.array_equal(_bits(out["t_raw"]), _bits(ref.t)) and np.array_equal(_bits(out["final_sdf"]), _bits(ref.final_sdf)), pipeline
