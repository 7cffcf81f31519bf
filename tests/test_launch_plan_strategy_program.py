"""The launch plan of a frame with a strategy program (csrc/rm_launch_plan.h, plan_strategy_program), through the g++
harness of tests/test_launch_plan.py: always one plain render pass, exactly where a compiled strategy would park rays,
use teams or run the single launch."""
import pytest

from test_launch_plan import plan

PROGRAM = 1024          # RM_STRATEGY_PROGRAM_BASE
MANDELBULB, GRAZING, SPHERE_CLOUD, PILLARS = 10, 1, 14, 12


def _plain(p, tiles_y):
    assert not p["refuse"]
    assert p["mode"] == 1 and p["single"] == 0 and p["park"] == (0, 0)
    assert p["interleave"] == 0 and p["tile_h"] == 4 and p["tiles_y"] == tiles_y
    assert p["team_wgs"] == 0 and p["pipeline_grid"] == 0 and p["pass_team"] == (0, 0) and p["queue_entry_bytes"] == 0
    assert p["tile_order"] == p["static_order"] and p["render_grid"] > 0


@pytest.mark.parametrize("strategy", [PROGRAM, PROGRAM + 7, 2 ** 31 - 1])
def test_mandelbulb_1080p_is_one_plain_pass(strategy):
    assert plan(MANDELBULB, 0)["single"] == 1                      # what the compiled Standard does here
    p = plan(MANDELBULB, strategy)
    _plain(p, 270)
    assert p["fused_reduce"] == 1 and p["static_order"] == 2


def test_scenes_that_park_with_a_compiled_strategy():
    for scene, order in ((GRAZING, 3), (SPHERE_CLOUD, 2), (PILLARS, 4)):
        if scene != PILLARS:
            assert plan(scene, 0)["park"][0] > 0
        p = plan(scene, PROGRAM)
        _plain(p, 270)
        assert p["static_order"] == order


def test_a_batch_is_one_plain_pass():
    p = plan(MANDELBULB, PROGRAM, 384, 384, batch=16)
    _plain(p, 96)
    assert p["batch"] == 1 and p["nframes"] == 16 and p["fused_reduce"] == 0


def test_scheduling_fields_of_the_descriptor_are_ignored():
    p = plan(MANDELBULB, PROGRAM, pipeline=2, suspend_after=(8, 32), eval_mode=2, tile_order_mode=1, tile_rows=1, resume_mode=3)
    _plain(p, 270)


def test_ids_below_the_base_plan_as_before():
    assert plan(MANDELBULB, 12)["single"] == 1
