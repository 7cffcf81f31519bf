"""The short last trip of the Mandelbulb evaluation on the GPU (rm_scenes.h THE SHORT LAST TRIP; team_trips of
rm_kernels.h): every kernel that takes it -- the ray marchers with and without teams, the single launch in its three
forms, a batch, the launch-per-pass schedule's team pass, the point evaluation -- against the oracle: raw t and final_sdf
as 64-bit patterns, iterations and hits."""
import numpy as np
import pytest

import short_last_trip_cases as C

pytestmark = pytest.mark.gpu

W, H = 96, 64
_ref = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _frame_ref(kid):
    """the oracle's 96x64 frame of the default view: computed once, shared, never modified"""
    if kid not in _ref:
        from oracle import oracle
        _ref[kid] = oracle.render(10, kid, C.frame_camera(W, H), W, H)
    return _ref[kid]


def _same_frame(out, ref, what):
    assert np.array_equal(out["iters"], ref.iters) and np.array_equal(out["hit"], ref.hit), what
    assert np.array_equal(_bits(out["t_raw"]), _bits(ref.t)), what
    assert np.array_equal(_bits(out["final_sdf"]), _bits(ref.final_sdf)), what


@pytest.mark.parametrize("n_live", [1, 17, 64, 197])
@pytest.mark.parametrize("kid", [0, 4])
@pytest.mark.parametrize("rays", ["mixed", "crawler"])
def test_march_rays(hip, rays, kid, n_live):
    from oracle import oracle
    o, d = C.mixed_rays(n_live, 2000 + n_live) if rays == "mixed" else C.crawler_rays(n_live)
    rh, rt, ri, rf = oracle.march_rays(10, kid, o, d)
    if rays == "crawler":
        assert (ri >= 200).any(), int(ri.max())
    for team in (True, False):
        hit, t, it, fs = hip.march_rays(10, kid, o, d, team=team)
        assert np.array_equal(it, ri) and np.array_equal(hit, rh), (team, int((it != ri).sum()))
        assert np.array_equal(_bits(t), _bits(rt)) and np.array_equal(_bits(fs), _bits(rf)), team


@pytest.mark.parametrize("form", [1, 2, 3])
@pytest.mark.parametrize("suspend_after", [(2, 6), (2, 9)])
def test_single_launch_frames(hip, suspend_after, form):
    extra = dict(keep_busy=-1) if form == 3 else {}
    for kid in (0, 4):
        desc = hip.make_desc(10, kid, C.frame_camera(W, H), W, H, full=True, pipeline=2, suspend_after=suspend_after,
                             pipeline_form=form, **extra)
        _same_frame(hip.render(desc, want_t_raw=True, want_final_sdf=True), _frame_ref(kid), (kid, suspend_after, form))


def test_batch_of_two_views(hip):
    """rm_render_batch: the default view and the macro view (camera at z = 1.9) in one launch.  A batch returns no fp64
    maps (RmOutputs of rm_render_batch_outputs: depth, iterations, hits), so raw t is compared as the fp32 depth the
    reference derives from it (types.py:93), bit for bit; final_sdf cannot be compared here."""
    from oracle import oracle
    from raymarch_algo_compare_amd.camera import Camera
    cams = np.stack([C.frame_camera(W, H), Camera((0.0, 0.0, 1.9), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 60.0, W, H).params14()])
    shape = hip.make_desc(10, 0, cams[0], W, H, pipeline=2, suspend_after=(2, 6))
    out = hip.render_batch(shape, cams)
    for f in range(2):
        ref = _frame_ref(0) if f == 0 else oracle.render(10, 0, cams[1], W, H)
        assert np.array_equal(out["iters"][f], ref.iters) and np.array_equal(out["hit"][f], ref.hit), f
        depth = np.where(ref.hit > 0, ref.t, 0.0).astype(np.float32)
        assert out["depth"][f].tobytes() == depth.tobytes(), f


@pytest.mark.parametrize("resume_mode", [0, 3])
def test_launch_per_pass_team_pass(hip, resume_mode):
    """pipeline = 1: the parked rays are finished by resume_team_kernel"""
    desc = hip.make_desc(10, 0, C.frame_camera(W, H), W, H, full=True, pipeline=1, suspend_after=(2, 6), resume_mode=resume_mode)
    _same_frame(hip.render(desc, want_t_raw=True, want_final_sdf=True), _frame_ref(0), resume_mode)


def test_sdf_eval_on_the_host_tests_points(hip):
    from oracle import oracle
    pts = C.all_points()
    assert np.array_equal(_bits(hip.sdf_eval(10, pts)), _bits(oracle.sdf_eval(10, pts)))
