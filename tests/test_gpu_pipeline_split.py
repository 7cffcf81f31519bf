"""The split form of the single launch (RmFrameDesc.pipeline_form = 2, csrc/rm_pipeline.h): the producers and the teams
of one frame as two kernels side by side -- pipeline_producer_kernel on the caller's stream, pipeline_team_kernel on the
library's own -- fed by the same queue and control block as the fused pipeline_kernel (pipeline_form = 1).  Which kernel
marches a ray, and whether the two overlap at all, is a matter of timing; the results are not: split = fused bit for bit,
and both equal the reference-generated goldens."""
import ctypes

import numpy as np
import pytest

from conftest import golden_frames
from test_gpu_parity import _check, _render

pytestmark = pytest.mark.gpu

STANDARD, ENHANCED, OVERSTEP_BISECT = 0, 4, 6      # Overstep-Bisect: the early hand-over is off by default
MAPS = ("depth", "iters", "hit", "t_raw", "final_sdf")
# default budgets (16 / 48 trips, 7/16 of the grid as teams), and tiny ones: nearly every ray goes through queue 1
SCHEDULES = (dict(), dict(suspend_after=(3, 11)), dict(suspend_after=(6, 40), team_grid=5, tile_rows=1))


def _same(a, b):
    """every map and the whole statistics record of two renders, bit for bit"""
    for k in MAPS:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k
    sa, sb = a["stats"], b["stats"]
    assert {k: v for k, v in sa.items() if k != "iter_hist"} == {k: v for k, v in sb.items() if k != "iter_hist"}
    assert (sa["iter_hist"] == sb["iter_hist"]).all()


_frames = {}


def _frame_192x108():
    """a 192x108 Mandelbulb frame description in the goldens' format (no golden of this size: fused is the reference)"""
    if "g" not in _frames:
        from raymarch_algo_compare_amd import registry
        from raymarch_algo_compare_amd.camera import Camera
        sc = registry.SCENES[10]
        W, H = 192, 108
        _frames["g"] = {"W": W, "H": H, "row0": 0, "rows": H, "max_iterations": 512, "hit_threshold": 1e-4, "max_distance": 100.0,
                        "lipschitz": 1.0, "cam": Camera(sc.camera_position, sc.camera_target, (0.0, 1.0, 0.0), 60.0, W, H).params14()}
    return _frames["g"]


def _fused(hip, tag, g, kid, sched):
    """the fused frame of (size, strategy, schedule): rendered once, shared, never modified"""
    key = (tag, kid, tuple(sorted(sched.items())))
    if key not in _frames:
        _frames[key] = _render(hip, g, 10, kid, True, pipeline=2, pipeline_form=1, **sched)
    return _frames[key]


@pytest.mark.parametrize("kid", [STANDARD, ENHANCED, OVERSTEP_BISECT])
def test_split_equals_fused_and_the_goldens_64x48(hip, kid):
    g = golden_frames("64x48").get(10, kid)
    for sched in SCHEDULES:
        fused = _fused(hip, "64x48", g, kid, sched)
        assert _check(fused, g, 10) == (0, 0), sched
        split = _render(hip, g, 10, kid, True, pipeline=2, pipeline_form=2, **sched)
        assert _check(split, g, 10) == (0, 0), sched
        _same(split, fused)


@pytest.mark.parametrize("kid", [STANDARD, ENHANCED, OVERSTEP_BISECT])
def test_split_equals_fused_192x108(hip, kid):
    g = _frame_192x108()
    for sched in SCHEDULES:
        _same(_render(hip, g, 10, kid, True, pipeline=2, pipeline_form=2, **sched), _fused(hip, "192x108", g, kid, sched))


def test_back_to_back_frames_on_one_workspace(hip):
    """three split frames, a fused one, a split one: generation tags, control-block reset and the statistics fold"""
    g = _frame_192x108()
    sched = dict(suspend_after=(3, 11))
    ref = _fused(hip, "192x108", g, STANDARD, sched)
    for form in (2, 2, 2, 1, 2):
        _same(_render(hip, g, 10, STANDARD, True, pipeline=2, pipeline_form=form, **sched), ref)


def test_serialised_kernels_give_the_same_frame(hip):
    """pipeline_form = 3: producers, then teams, on the caller's stream -- what is left of the split form when the device
    does not run the two kernels side by side.  The frame returns (an error word of the queue protocol would raise)."""
    for tag, g in (("64x48", golden_frames("64x48").get(10, STANDARD)), ("192x108", _frame_192x108())):
        for sched in SCHEDULES:
            out = _render(hip, g, 10, STANDARD, True, pipeline=2, pipeline_form=3, keep_busy=-1, **sched)
            _same(out, _fused(hip, tag, g, STANDARD, sched))


def test_more_teams_than_tiles(hip):
    """64x48 in one-row tiles is 48 tiles, in 64x4 tiles 12: 300 team workgroups asked for (the plan caps them at half
    the resident grid), three producer workgroups at most"""
    g = golden_frames("64x48").get(10, STANDARD)
    for sched in (dict(team_grid=300), dict(team_grid=300, tile_rows=1, suspend_after=(2, 5))):
        split = _render(hip, g, 10, STANDARD, True, pipeline=2, pipeline_form=2, **sched)
        assert _check(split, g, 10) == (0, 0), sched
        _same(split, _fused(hip, "64x48", g, STANDARD, sched))


def test_batch_of_frames_split(hip):
    """rm_render_batch takes the split form when asked: the parked ray's frame rides on its queue entry"""
    g = golden_frames("64x48").get(10, STANDARD)
    cams = np.stack([g["cam"], g["cam"]])
    cfgs = [dict(max_iterations=512), dict(max_iterations=300)]
    outs = []
    for form in (1, 2):
        shape = hip.make_desc(10, STANDARD, g["cam"], g["W"], g["H"], pipeline=2, suspend_after=(3, 11), team_grid=2, pipeline_form=form)
        outs.append(hip.render_batch(shape, cams, cfgs))
    for k in ("iters", "hit", "depth"):
        assert outs[0][k].tobytes() == outs[1][k].tobytes(), k
    assert (outs[1]["iters"][0] == g["iters"]).all() and (outs[1]["hit"][0] == g["hit"]).all()


def test_split_is_refused_outside_its_schedule(hip):
    """late teams and the queue-0 stage keep the fused kernel: asking for the split form there is an argument error"""
    g = golden_frames("64x48").get(10, STANDARD)
    for sched in (dict(late_teams=3, team_grid=1), dict(queue_first=1), dict(resume_mode=1)):
        with pytest.raises(hip.RmError):
            _render(hip, g, 10, STANDARD, True, pipeline=2, pipeline_form=2, suspend_after=(3, 11), **sched)
        assert _check(_render(hip, g, 10, STANDARD, True, pipeline=2, suspend_after=(3, 11), **sched), g, 10) == (0, 0)


def test_pass_marks_of_a_split_frame(hip):
    """rm_get_pass_ms still splits the frame at the marks its waves leave: four non-negative spans"""
    g = _frame_192x108()
    L = hip.load()
    hip.check(L.rm_set_pass_timing(1))
    try:
        _render(hip, g, 10, STANDARD, False, pipeline=2, pipeline_form=2, suspend_after=(8, 40))
        n, ms = ctypes.c_int32(0), (ctypes.c_float * 4)()
        hip.check(L.rm_get_pass_ms(None, ctypes.byref(n), ms))
        assert n.value == 4 and all(ms[i] >= 0.0 for i in range(4)) and sum(ms) > 0.0
    finally:
        hip.check(L.rm_set_pass_timing(0))
