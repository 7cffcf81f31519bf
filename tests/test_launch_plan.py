"""The launch policy of a frame (csrc/rm_launch_plan.h) on the CPU, with faked device facts: 256 compute units and an
occupancy of 2 workgroups per CU unless a case says otherwise.  Schedules never change results, so the parity suites
pass whatever the plan picks; these cases pin the documented decisions instead.  Each names the comment (in
rm_launch_plan.h unless said otherwise) or the DESIGN.md figure it pins."""
import ctypes

import pytest

from conftest import build_native
from raymarch_algo_compare_amd import _native

MANDELBULB, GRAZING, THIN_PLANES, SPHERE_CLOUD, BUMPY = 10, 1, 13, 14, 15
STANDARD, ENHANCED, OVERSTEP, SKIPPING, REVAA, HYBRID, SEGMENT = 0, 4, 6, 7, 8, 9, 10
PROGRAM = 1024                      # RM_SCENE_PROGRAM_BASE: the first scene-program id
CUS = 256
RESIDENT = CUS * 2                  # the single launch's resident grid at 2 workgroups per CU

_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(build_native("plan_check"))
        _lib.rmplan_fields.restype = ctypes.c_char_p
        _lib.rmplan.restype = None
    return _lib


def plan(scene, strategy, width=1920, height=1080, *, batch=0, configs=None, occ=2, occ_batch=None, occ_pipeline=None,
         has_teams=None, has_resume_team=None, entry_bytes=224, max_iterations=512, has_split=None, occ_producers=None,
         occ_teams=None, **desc):
    """The plan of one descriptor as a dict (refuse: the plan refuses it).  The split form's two kernels exist where teams
    do and reach the fused kernel's occupancy unless a case says otherwise."""
    L = lib()
    d = _native.make_desc(scene, strategy, [0.0] * 14, width, height, max_iterations=max_iterations, **desc)
    teams = scene in (MANDELBULB, SPHERE_CLOUD, BUMPY) if has_teams is None else has_teams
    names = ["refuse"] + [n for n in L.rmplan_fields().decode().split(",") if n]
    out = (ctypes.c_int64 * len(names))()
    asked = (ctypes.c_int * 4)()
    cfg = None
    if configs is not None:
        cfg = (_native.RmMarchConfig * len(configs))()
        for c, it in zip(cfg, configs):
            c.max_iterations = it
    L.rmplan(ctypes.byref(d), batch, cfg, CUS, occ, occ if occ_batch is None else occ_batch,
             occ if occ_pipeline is None else occ_pipeline, int(teams), int(teams if has_resume_team is None else has_resume_team),
             entry_bytes, out, asked, int(teams if has_split is None else has_split),
             (occ if occ_pipeline is None else occ_pipeline) if occ_producers is None else occ_producers,
             (occ if occ_pipeline is None else occ_pipeline) if occ_teams is None else occ_teams)
    p = dict(zip(names, out))
    p["park"] = (p.pop("park[0]"), p.pop("park[1]"))
    p["pass_team"] = (p.pop("pass_team[0]"), p.pop("pass_team[1]"))
    p["asked"] = tuple(asked[:2])
    p["asked_split"] = tuple(asked[2:])      # the split form's producers / teams
    return p


def share16(p):
    """Team workgroups as sixteenths of the resident grid."""
    assert p["team_wgs"] * 16 % RESIDENT == 0, p["team_wgs"]
    return p["team_wgs"] * 16 // RESIDENT


# ---- the single launch (Mandelbulb) --------------------------------------------------------------------------------------

def test_mandelbulb_1080p_standard_is_one_launch():
    # pipeline_mode ("the single launch is 4-27 % faster"), suspend_levels ("struck from their tile at 16 trips ... handed
    # to the teams at 48"), the team share table ("1920x1080 ... 192: 9.4"), KEEP BUSY (burst 256), EARLY HAND-OVER (at the strike)
    p = plan(MANDELBULB, STANDARD)
    assert p["refuse"] == 0 and p["mode"] == 2 and p["single"] == 1
    assert p["park"] == (16, 48)
    assert (p["tile_h"], p["tiles_x"], p["tiles_y"]) == (4, 30, 270)
    assert share16(p) == 6
    assert p["keep_busy"] == 256 and p["early_handover"] == p["park"][0] == 16
    assert p["suspend_after2"] == 48 and p["q0_detach"] == 1 and p["early_exit_wgs"] == 0
    # grid = static teams + producers (every other resident workgroup; DESIGN.md section 6 "b threading")
    assert p["producer_waves"] == (RESIDENT - p["team_wgs"]) * 4
    assert p["pipeline_grid"] == RESIDENT == p["late_team_first"]
    assert p["fused_reduce"] == 0 and p["queue_entry_bytes"] == 224
    assert p["asked"] == (0, 1)           # the pipeline's occupancy only: no render grid is sized


def test_mandelbulb_1080p_with_previous_costs():
    # "with the previous frame's tile costs ... 24 / 56 with 7/16 of the grid as teams"; "64x1 tiles ... 1080p 9.6 -> 8.5 ms"
    p = plan(MANDELBULB, STANDARD, tile_order_mode=1)
    assert p["park"] == (24, 56)
    assert (p["tile_h"], p["tiles_y"]) == (1, 1080)
    assert share16(p) == 7
    assert p["tile_order"] == 1 and p["static_order"] == 2      # no costs yet: centre-out


def test_segment_budgets():
    # "larger frames, and Segment whose trips evaluate twice, at 32 / 64"
    assert plan(MANDELBULB, SEGMENT)["park"] == (32, 64)


@pytest.mark.parametrize("strategy, share, share_ordered", [(OVERSTEP, 3, 4), (HYBRID, 3, 4), (SKIPPING, 6, 4)])
def test_strategies_whose_rays_end_early(strategy, share, share_ordered):
    # EARLY HAND-OVER "the three whose rays end early or whose loop index restarts lose 1-2 % ...: off there";
    # team share "Overstep-Bisect 2.95 / 3.03 / 3.32 ms and Adaptive-Hybrid 4.67 / 4.69 / 4.71 at 96 / 128 / 192 teams"
    p = plan(MANDELBULB, strategy)
    assert p["single"] == 1 and p["early_handover"] == 0
    assert share16(p) == share
    assert share16(plan(MANDELBULB, strategy, tile_order_mode=1)) == share_ordered


def test_720p_enhanced_share():
    # "1280x720 wants 128-160 teams, not 224 -- Enhanced 17.6 -> 15.6 ms in the sum at 128"
    assert share16(plan(MANDELBULB, ENHANCED, 1280, 720)) == 4
    assert share16(plan(MANDELBULB, STANDARD, 1280, 720)) == 5


def test_8k_does_not_suspend():
    # pipeline_mode "at 7680x4320 the frame is throughput-bound"; suspend_levels "7680x4320: 50 ms without, 53-58 with"
    p = plan(MANDELBULB, STANDARD, 7680, 4320)
    assert p["mode"] == 1 and p["park"] == (0, 0) and p["single"] == 0
    assert p["fused_reduce"] == 1


def test_4k_budgets():
    # "larger frames ... at 32 / 64"; team share "3840x2160 ... 96: 15.1"
    p = plan(MANDELBULB, STANDARD, 3840, 2160)
    assert p["mode"] == 2 and p["park"] == (32, 64)
    assert share16(p) == 3


@pytest.mark.parametrize("width, height, budgets", [(1920, 1080, (32, 128)), (3840, 2160, (48, 192))])
def test_one_launch_per_pass_budgets(width, height, budgets):
    # suspend_levels "1080p: 15.2 -> 11.1 ms at 32 / 128 trips; 3840x2160 ... at 48 / 192"; "Segment and RevAA evaluate the
    # SDF twice per loop trip: half the trip budgets"
    p = plan(MANDELBULB, STANDARD, width, height, pipeline=1)
    assert p["mode"] == 1 and p["single"] == 0 and p["park"] == budgets
    for strategy in (SEGMENT, REVAA):
        assert plan(MANDELBULB, strategy, width, height, pipeline=1)["park"] == (budgets[0] // 2, budgets[1] // 2)
    # the passes: one resume workgroup per CU, team passes followed by as many fillers (KEEP BUSY)
    assert p["render_grid"] == RESIDENT and p["resume_grid"] == CUS and p["resume_refill_min"] == 16
    assert p["pass_team"] == (0, 1) and p["pass_keep_busy"] == 256 and p["team_pass_grid"] == 2 * CUS
    assert p["fused_reduce"] == 0


def test_per_pass_knobs():
    p = plan(MANDELBULB, STANDARD, pipeline=1, resume_mode=3, keep_busy=-1, resume_grid=7)
    assert p["pass_team"] == (1, 1) and p["pass_keep_busy"] == 0 and p["team_pass_grid"] == p["resume_grid"] == 7
    p = plan(MANDELBULB, STANDARD, pipeline=1, resume_mode=1)
    assert p["pass_team"] == (0, 0) and p["pass_keep_busy"] == 0


# ---- one launch per pass: the other scenes ------------------------------------------------------------------------------

@pytest.mark.parametrize("scene", [GRAZING, THIN_PLANES])
def test_plane_scenes_park_at_128(scene):
    # "Parking at 128 trips ... 20-45 % faster for every strategy but Skipping-Spheres"
    for strategy in (STANDARD, SEGMENT, HYBRID):
        p = plan(scene, strategy)
        assert p["park"] == (128, 0) and p["mode"] == 1 and p["pass_team"] == (0, 0)
    assert plan(scene, SKIPPING)["park"] == (0, 0)


@pytest.mark.parametrize("scene", [SPHERE_CLOUD, BUMPY])
def test_sphere_unions_park_at_16(scene):
    # "parked at 16 trips and finished by TEAMS ... Not for Adaptive-Hybrid"; Segment / RevAA half; suspend_levels' strat_ok
    assert plan(scene, STANDARD)["park"] == (16, 0)
    assert plan(scene, SEGMENT)["park"] == (8, 0)
    assert plan(scene, REVAA)["park"] == (8, 0)
    for strategy in (SKIPPING, OVERSTEP, HYBRID):
        assert plan(scene, strategy)["park"] == (0, 0)
    p = plan(scene, STANDARD)
    assert p["pass_team"][0] == 1 and p["team_pass_grid"] == 2 * CUS       # one resume pass: the team form


def test_no_parking_elsewhere():
    for scene in (0, 2, 3, 12, 16, 19):
        assert plan(scene, STANDARD)["park"] == (0, 0)
    assert plan(SPHERE_CLOUD, STANDARD, max_iterations=128)["park"] == (0, 0)        # budgets of 128 and below


def test_refill_default():
    # "the scenes whose rays are short ... measured better at 16"
    for scene in range(20):
        assert plan(scene, STANDARD)["refill_min"] == (16 if scene in (0, 2, 3, 4, 6, 18, 19) else 8), scene
    assert plan(0, STANDARD, refill_min=5)["refill_min"] == 5
    assert plan(1, STANDARD, refill_min=65)["refill_min"] == 8


def test_interleave():
    # "one trip per turn pays where the trip count varies (Mandelbulb)"
    assert plan(MANDELBULB, STANDARD)["interleave"] == 1
    assert plan(SPHERE_CLOUD, STANDARD)["interleave"] == 0
    assert plan(MANDELBULB, STANDARD, eval_mode=1)["interleave"] == 0
    assert plan(SPHERE_CLOUD, STANDARD, eval_mode=2)["interleave"] == 1


# ---- tile order -----------------------------------------------------------------------------------------------------------

def test_tile_order_per_scene():
    # default_tile_order: plane scenes natural (3); Thin Torus, Near Miss, Pillar Forest middle rows first (4); centre-out (2)
    want = {1: 3, 13: 3, 3: 4, 5: 4, 12: 4}
    for scene in range(20):
        p = plan(scene, STANDARD)
        assert p["tile_order"] == p["static_order"] == want.get(scene, 2), scene
    assert plan(PROGRAM, STANDARD)["tile_order"] == 2
    assert plan(0, STANDARD, tile_order_mode=3)["tile_order"] == 3


def test_tile_order_of_batches():
    # "Mandelbulb sweeps: centre-out within every frame"; other batches natural
    assert plan(MANDELBULB, STANDARD, 384, 384, batch=4)["tile_order"] == 2
    for scene in (0, 1, 3, 14):
        assert plan(scene, STANDARD, 384, 384, batch=4)["tile_order"] == 3
    assert plan(3, STANDARD, 384, 384, batch=1)["tile_order"] == 4            # a batch of one orders like a frame


# ---- scene programs -------------------------------------------------------------------------------------------------------

def test_scene_programs_run_one_launch_per_pass():
    # pipeline_mode "a scene program has no single-launch form"
    p = plan(PROGRAM, STANDARD, pipeline=2, suspend_after=(16, 64), has_teams=False)
    assert p["mode"] == 1 and p["single"] == 0 and p["park"] == (16, 64) and p["resume_grid"] == CUS
    assert plan(PROGRAM, STANDARD, has_teams=False)["park"] == (0, 0)


# ---- grids ----------------------------------------------------------------------------------------------------------------

def test_render_grid():
    # grid_per_cu: min(CUs * min(per_cu, 3), ceil(tiles / 4)); "three workgroups per CU at most ... measured 10-16 % slower with four"
    assert plan(0, STANDARD)["render_grid"] == CUS * 2
    assert plan(0, STANDARD, occ=5)["render_grid"] == CUS * 3
    assert plan(0, STANDARD, occ=1)["render_grid"] == CUS
    assert plan(0, STANDARD, occ=0)["render_grid"] == CUS * 2          # occupancy unknown: 2
    assert plan(0, STANDARD, 96, 64)["render_grid"] == 8               # 2 x 16 tiles
    assert plan(0, STANDARD, grid_waves=100)["render_grid"] == 25
    assert plan(0, STANDARD, 96, 64, grid_waves=100)["render_grid"] == 8
    assert plan(0, STANDARD, 64, 4)["render_grid"] == 1
    assert plan(0, STANDARD)["asked"] == (1, 0)
    assert plan(0, STANDARD, grid_waves=100)["asked"] == (0, 0)


def test_batch_grid_and_policy():
    # the batch is one launch: its grid is sized for all tiles with the batch kernel's occupancy
    p = plan(0, STANDARD, 128, 64, batch=16, occ=3, occ_batch=1)
    assert p["render_grid"] == min(CUS, 16 * 2 * 16 // 4)
    assert plan(0, STANDARD, 128, 64, batch=64, occ=3, occ_batch=1)["render_grid"] == CUS
    # "the launch-wide scheduling policy looks at the largest budget of a batch"
    p = plan(SPHERE_CLOUD, STANDARD, 384, 384, batch=3, configs=[128, 512, 512], max_iterations=128)
    assert p["march_frame"] == 1 and p["park"] == (16, 0)
    p = plan(SPHERE_CLOUD, STANDARD, 384, 384, batch=2, configs=[128, 64], max_iterations=512)
    assert p["march_frame"] == 0 and p["park"] == (0, 0)
    # sweeps: "64 x 384^2 viewpoints 29.0 ms" at 4/16 of the grid as teams
    p = plan(MANDELBULB, STANDARD, 384, 384, batch=64)
    assert p["single"] == 1 and share16(p) == 4


def test_single_launch_grid_knobs():
    # an explicit grid_waves sizes the producers; team_grid the teams (capped at half the resident grid)
    p = plan(MANDELBULB, STANDARD, grid_waves=40, team_grid=40)
    assert p["team_wgs"] == 40 and p["producer_waves"] == 40 and p["pipeline_grid"] == 50
    assert plan(MANDELBULB, STANDARD, team_grid=700)["team_wgs"] == RESIDENT // 2
    assert plan(MANDELBULB, STANDARD, occ_pipeline=0)["pipeline_grid"] == RESIDENT      # occupancy unknown: 2 per CU


# ---- explicit knobs, fused reduce, refusals -------------------------------------------------------------------------------

def test_explicit_knobs_override_the_defaults():
    p = plan(MANDELBULB, STANDARD, suspend_after=(20, 90), keep_busy=64, early_handover=30, early_trips=6, exit_backlog=9,
             queue_first=2, queue_refill_min=4, queue_retry=3, team_retry=2, team_steal=2)
    assert p["park"] == (20, 90) and p["keep_busy"] == 64 and p["early_trips"] == 6 and p["exit_backlog"] == 9
    assert p["q0_detach"] == 0 and p["early_handover"] == 0          # queue_first 2: no detach, so no hand-over
    assert (p["q0_first"], p["q0_refill_min"], p["q0_retry"], p["team_retry"], p["team_steal"]) == (0, 4, 3, 2, 0)
    p = plan(MANDELBULB, STANDARD, keep_busy=-1, early_handover=-1)
    assert p["keep_busy"] == 0 and p["early_handover"] == 0
    p = plan(MANDELBULB, STANDARD, early_handover=30)
    assert p["early_handover"] == 30
    # late teams: no keep-busy (they need the producers' places); never with an explicit grid
    p = plan(MANDELBULB, STANDARD, late_teams=64)
    assert p["early_exit_wgs"] == 64 and p["keep_busy"] == 0 and p["pipeline_grid"] == RESIDENT + 64
    assert plan(MANDELBULB, STANDARD, late_teams=64, grid_waves=400)["early_exit_wgs"] == 0
    # off switches
    assert plan(MANDELBULB, STANDARD, suspend_after=(-1, 0))["park"] == (0, 0)
    assert plan(MANDELBULB, STANDARD, suspend_after=(0, -1))["park"] == (16, 0)
    p = plan(MANDELBULB, STANDARD, resume_mode=1)
    assert p["single"] == 1 and p["team_wgs"] == 0 and p["suspend_after2"] == 0 and p["keep_busy"] == 0


def test_fused_reduce_only_for_one_frame_without_parking():
    assert plan(0, STANDARD)["fused_reduce"] == 1
    assert plan(0, STANDARD, batch=1)["fused_reduce"] == 1
    assert plan(0, STANDARD, batch=2)["fused_reduce"] == 0
    assert plan(GRAZING, STANDARD)["fused_reduce"] == 0
    assert plan(0, STANDARD, rows=0)["fused_reduce"] == 0


def test_one_row_tiles_exist_for_the_team_single_launch_only():
    p = plan(MANDELBULB, STANDARD, tile_rows=1)
    assert p["refuse"] == 0 and p["tile_h"] == 1 and p["tiles_y"] == 1080
    assert plan(MANDELBULB, STANDARD, tile_rows=1, pipeline=1)["refuse"] == 1
    assert plan(0, STANDARD, tile_rows=1)["refuse"] == 1
    # the single launch of a scene without teams keeps 64x4 tiles
    p = plan(MANDELBULB, STANDARD, tile_order_mode=1, has_teams=False)
    assert p["single"] == 1 and p["tile_h"] == 4 and p["team_wgs"] == 0


# ---- how the single launch is performed (single_launch_form) --------------------------------------------------------------

def test_default_single_launch_is_split():
    # "bench.py 270.5-272.5 Mrays/s with the fused kernel, 278.0-278.7 split"
    p = plan(MANDELBULB, STANDARD)
    assert p["form"] == 2 and p["refuse"] == 0
    assert p["asked"] == (0, 1) and p["asked_split"] == (1, 1)      # the fused occupancy is the one that sized the grid


@pytest.mark.parametrize("strategy", [SKIPPING, HYBRID])
def test_strategies_that_keep_the_fused_kernel(strategy):
    # "Skipping-Spheres and Adaptive-Hybrid keep the fused kernel"
    p = plan(MANDELBULB, strategy)
    assert p["single"] == 1 and p["form"] == 1 and p["asked_split"] == (0, 0)


def test_batches_keep_the_fused_kernel():
    p = plan(MANDELBULB, STANDARD, 384, 384, batch=4)
    assert p["single"] == 1 and p["form"] == 1 and p["asked_split"] == (0, 0)


@pytest.mark.parametrize("occ_pipeline, split, form", [(2, (2, 2), 2), (2, (1, 2), 1), (2, (2, 1), 1), (3, (3, 2), 1), (3, (2, 3), 1),
                                                       (5, (3, 3), 2), (2, (0, 0), 1), (0, (2, 2), 1)])
def test_split_needs_the_fused_grids_occupancy(occ_pipeline, split, form):
    # "only where each of the two kernels reaches at least the workgroups per compute unit the plan's grid counts on"
    # (grid_per_cu: three at most); an unknown occupancy keeps the fused kernel
    p = plan(MANDELBULB, STANDARD, occ_pipeline=occ_pipeline, occ_producers=split[0], occ_teams=split[1])
    assert p["form"] == form and p["refuse"] == 0


def test_no_split_where_the_schedule_is_not_covered():
    # "detach mode, every team resident from the start"; a scene without the two kernels
    assert plan(MANDELBULB, STANDARD, queue_first=2)["form"] == 1
    assert plan(MANDELBULB, STANDARD, late_teams=64)["form"] == 1
    assert plan(MANDELBULB, STANDARD, resume_mode=1)["form"] == 1            # no teams
    assert plan(MANDELBULB, STANDARD, has_split=False)["form"] == 1
    for kw in (dict(queue_first=2), dict(late_teams=64), dict(has_split=False)):
        assert plan(MANDELBULB, STANDARD, **kw)["asked_split"] == (0, 0)


def test_explicit_forms():
    for form in (1, 2, 3):
        p = plan(MANDELBULB, STANDARD, pipeline_form=form, occ_producers=1, occ_teams=1)      # no occupancy test
        assert p["form"] == form and p["refuse"] == 0 and p["asked_split"] == (0, 0)
    # an explicit form holds for the strategies and the batches the library would keep fused
    assert plan(MANDELBULB, SKIPPING, pipeline_form=2)["form"] == 2
    assert plan(MANDELBULB, STANDARD, 384, 384, batch=4, pipeline_form=2)["form"] == 2
    # "the split form exists for single launches with teams in detach mode without late teams"
    for form in (2, 3):
        assert plan(MANDELBULB, STANDARD, pipeline_form=form, late_teams=64)["refuse"] == 1
        assert plan(MANDELBULB, STANDARD, pipeline_form=form, queue_first=2)["refuse"] == 1
        assert plan(MANDELBULB, STANDARD, pipeline_form=form, has_split=False)["refuse"] == 1
    assert plan(MANDELBULB, STANDARD, pipeline_form=1, late_teams=64)["refuse"] == 0


def test_no_occupancy_is_asked_of_the_split_kernels_outside_a_single_launch():
    for p in (plan(0, STANDARD), plan(0, STANDARD, grid_waves=100), plan(MANDELBULB, STANDARD, pipeline=1),
              plan(MANDELBULB, STANDARD, 7680, 4320), plan(SPHERE_CLOUD, STANDARD), plan(0, STANDARD, pipeline_form=2),
              plan(MANDELBULB, STANDARD, 384, 384, batch=4, pipeline=1)):
        assert p["single"] == 0 and p["form"] == 0 and p["refuse"] == 0
        assert p["asked"][1] == 0 and p["asked_split"] == (0, 0)


# ---- the parked-ray queues' clear (queue_step) ----------------------------------------------------------------------------

def queue_step(prev, writer, stride, need, cap_before, cap_after=None):
    """(bytes to clear, (stride, writer, used) to remember) for the previous key (stride, writer, used)"""
    out = (ctypes.c_uint64 * 4)()
    u64 = ctypes.c_uint64
    lib().rmplan_queue(prev[0], prev[1], u64(prev[2]), writer, stride, u64(need), u64(cap_before),
                       u64(cap_before if cap_after is None else cap_after), out)
    return out[0], (out[1], out[2], out[3])


@pytest.mark.parametrize("writer", [1, 2])
def test_a_fresh_or_grown_queue_is_cleared_as_far_as_needed(writer):
    # "fresh memory: no word of it may look like a published entry of a later launch"
    assert queue_step((0, 0, 0), writer, 224, 1000, 0, 1000) == (1000, (224, writer, 1000))
    # grown: what the old buffer held is gone with it
    assert queue_step((224, 2, 4000), writer, 224, 5000, 4000, 5000) == (5000, (224, writer, 5000))
    assert queue_step((160, 1, 4000), writer, 224, 5000, 4000, 8192) == (5000, (224, writer, 5000))


def test_the_same_single_launch_layout_clears_nothing():
    assert queue_step((224, 2, 3000), 2, 224, 2000, 4000) == (0, (224, 2, 3000))
    assert queue_step((224, 2, 3000), 2, 224, 4000, 4000) == (0, (224, 2, 4000))


@pytest.mark.parametrize("prev", [(224, 1, 3000), (224, 3, 3000), (160, 2, 3000), (160, 1, 3000)])
def test_a_single_launch_after_another_writer_clears_what_that_one_used(prev):
    # "another layout wrote here: stale payload words now sit at this launch's `ready` offsets"
    assert queue_step(prev, 2, 224, 2000, 4000) == (3000, (224, 2, 2000))
    assert queue_step(prev, 2, 224, 3500, 4000) == (3000, (224, 2, 3500))
    assert queue_step((prev[0], prev[1], 9000), 2, 224, 2000, 4000) == (4000, (224, 2, 2000))     # min(used, cap)
    assert queue_step((prev[0], prev[1], 0), 2, 224, 2000, 4000) == (0, (224, 2, 2000))           # nothing was touched


@pytest.mark.parametrize("prev", [(224, 2, 3000), (160, 2, 3000), (224, 3, 3000), (224, 1, 3000), (0, 0, 0)])
def test_a_pass_per_launch_frame_never_clears_but_records_itself(prev):
    assert queue_step(prev, 1, 192, 2000, 4000) == (0, (192, 1, max(prev[2], 2000)))


def test_used_is_the_running_maximum():
    key = (0, 0, 0)
    seen = []
    for writer, stride, need in [(2, 224, 1000), (2, 224, 3000), (2, 224, 500), (1, 224, 3500), (1, 160, 100)]:
        _, key = queue_step(key, writer, stride, need, 4000)
        seen.append(key[2])
    assert seen == [1000, 3000, 3000, 3500, 3500]
    # the unknown writer of rm_debug_poison_queues touches the whole buffer; the next single launch clears all of it
    clear, key = queue_step(key, 3, key[0], 4000, 4000)
    assert clear == 0 and key == (160, 3, 4000)
    assert queue_step(key, 2, 160, 100, 4000) == (4000, (160, 2, 100))


# ---- filler workgroups of rm_march_rays_team, tile-order cache keys -------------------------------------------------------

def test_team_fillers():
    # "filler workgroups (two per compute unit in all)"
    L = lib()
    L.rmplan_fillers.argtypes = [ctypes.c_int, ctypes.c_int64]
    assert L.rmplan_fillers(CUS, 1) == 2 * CUS - 1
    assert L.rmplan_fillers(CUS, 2 * CUS) == 0
    assert L.rmplan_fillers(CUS, 2 * CUS + 1) == 0              # never negative
    assert L.rmplan_fillers(CUS, 1 << 40) == 0
    assert L.rmplan_fillers(CUS, 0) == 2 * CUS


def test_tile_order_cache_keys():
    d = _native.make_desc(MANDELBULB, ENHANCED, [0.0] * 14, 1920, 1080)
    d.row0, d.rows, d.band_rows, d.band_stride, d.band_offset = 8, 540, 4, 2, 1
    dyn, stat = (ctypes.c_int64 * 10)(), (ctypes.c_int64 * 12)()
    lib().rmplan_keys(ctypes.byref(d), 1, 3, 4, dyn, stat)
    assert list(dyn) == [MANDELBULB, ENHANCED, 1920, 1080, 8, 540, 4, 2, 1, 1]
    # "pure geometry: the same permutation for every scene and strategy", per frame count and order
    assert list(stat) == [0, 0, 1920, 1080, 8, 540, 4, 2, 1, 1, 3, 4]
