"""The gfx950 kernels against what the REFERENCE computes away from the default MarchConfig, camera and frame shape:
tests/golden/frames_config_<family>.npz and rays_config.npz (families as in tests/test_config_golden.py), compared
with the fixtures directly -- no oracle in between.  Bit for bit: iterations, hits, the hashes of the raw fp64 t and
final_sdf, the fp32 depth map (hashed, as the reference's RayMarchStats builds it) and RmStats.

Cases that reach the last, saturating bin of RmStats.iter_hist (543; iterations above 542 are folded into it): family
C's histogram cases at budgets 543, 544 and 2048 and its thresholds 0 and 1e-9 at budget 700 (nothing converges that
far, the budget runs out), and family E's draws with budgets 700 and 2048."""
import numpy as np
import pytest

import config_cases as cc
from conftest import sha_f64

pytestmark = pytest.mark.gpu

HIST_BINS = 544
# long-ray suspension with budgets far below the library's: passes with one wavefront per 64 parked rays, passes with
# wavefront teams, and the single launch with a team grid -- schedules only, every one must give the same frame
SCHEDULES = (dict(suspend_after=(-1, -1)),
             dict(suspend_after=(2, 5), pipeline=1, resume_mode=1),
             dict(suspend_after=(3, 7), pipeline=1, resume_mode=2),
             dict(suspend_after=(2, 6), pipeline=2, team_grid=3))


def _desc(hip, c, full=True, **kw):
    return hip.make_desc(c["sid"], c["kid"], c["cam"], c["W"], c["H"], c["row0"], c["rows"], c["max_iterations"],
                         c["hit_threshold"], c["max_distance"], c["lipschitz"], full, params=c["prm"], **kw)


def _check_stats(c, st, what):
    it = c["iters"].reshape(-1)
    want = np.bincount(np.minimum(it, HIST_BINS - 1), minlength=HIST_BINS)
    assert st["total_rays"] == it.size and st["hit_count"] == int(c["hit"].sum()) and st["sum_iters"] == int(it.sum()), what
    assert st["iter_min"] == int(it.min()) and st["iter_max"] == int(it.max()), what
    assert len(st["iter_hist"]) == HIST_BINS and (st["iter_hist"] == want).all(), what


def _check_full(c, out, what):
    assert (out["iters"] == c["iters"]).all(), what
    assert (out["hit"] == c["hit"]).all(), what
    assert cc.first_bad_ray(c, out["t_raw"]) is None, (what, "first ray with another t", cc.first_bad_ray(c, out["t_raw"]))
    assert sha_f64(out["t_raw"]) == c["sha_t"] and sha_f64(out["final_sdf"]) == c["sha_fs"], what
    _check_lean(c, out, what)


def _check_lean(c, out, what):
    import hashlib
    assert (out["iters"] == c["iters"]).all() and (out["hit"] == c["hit"]).all(), what
    assert out["depth"].dtype == np.float32
    assert hashlib.sha256(np.ascontiguousarray(out["depth"]).astype("<f4").tobytes()).digest() == c["sha_depth32"], what
    _check_stats(c, out["stats"], what)


@pytest.mark.parametrize("fam", cc.FAMILIES)
def test_frames_match_reference(hip, fam):
    """rm_render of every case, with raw outputs (full = 1) and on the product path (full = 0)."""
    for c in cc.family(fam):
        _check_full(c, hip.render(_desc(hip, c), want_t_raw=True, want_final_sdf=True), ("full", cc.label(c)))
        _check_lean(c, hip.render(_desc(hip, c, full=False)), ("lean", cc.label(c)))


def test_last_histogram_bin_saturates(hip):
    """Frames whose iterations pass 542: the counts above are folded into bin 543, and iter_max is not clamped."""
    top = [c for c in cc.all_cases() if c["iters"].max() >= HIST_BINS - 1]
    assert len(top) >= 40 and any(c["iters"].max() > 2000 for c in top)
    assert {542, 543, 544} <= {int(c["iters"].max()) for c in cc.family("C")}          # both sides of the clamp
    for c in top:
        out = hip.render(_desc(hip, c, full=False))
        over = int((c["iters"] >= HIST_BINS - 1).sum())
        assert over > 0 and int(out["stats"]["iter_hist"][HIST_BINS - 1]) == over, cc.label(c)
        assert int(out["stats"]["iter_hist"].sum()) == c["iters"].size and out["stats"]["iter_max"] == int(c["iters"].max()), cc.label(c)


@pytest.mark.parametrize("fam", cc.FAMILIES)
def test_parked_rays_carry_their_configuration(hip, fam):
    """Every Mandelbulb case and one case in five of the others with suspension off, in passes with tiny suspension budgets
    and in the single launch with a team grid: a parked ray is resumed with its frame's budget, threshold, far plane and
    parameters -- budgets below the suspension budget included (family B)."""
    picked = [c for i, c in enumerate(cc.family(fam)) if c["sid"] == 10 or i % 5 == 0]
    assert any(c["sid"] == 10 for c in picked)
    for c in picked:
        for sched in SCHEDULES:
            _check_full(c, hip.render(_desc(hip, c, **sched), want_t_raw=True, want_final_sdf=True), (sched, cc.label(c)))
        _check_lean(c, hip.render(_desc(hip, c, full=False, **SCHEDULES[3])), ("lean", SCHEDULES[3], cc.label(c)))


def test_sweep_batches_match_reference(hip):
    """Family A as the sweep issues it: one rm_render_batch per (scene, strategy, viewpoint), one frame and one
    RmMarchConfig per level."""
    groups = {}
    for c in cc.family("A"):
        groups.setdefault(c["tag"].rsplit("/", 1)[0], []).append(c)
    assert len(groups) == 99
    for name, cases in groups.items():
        c0 = cases[0]
        assert all((c["sid"], c["kid"], c["W"], c["H"]) == (c0["sid"], c0["kid"], c0["W"], c0["H"]) for c in cases)
        for full in (True, False):
            cfgs = [dict(max_iterations=c["max_iterations"], hit_threshold=c["hit_threshold"], max_distance=c["max_distance"],
                         lipschitz=c["lipschitz"], full=full) for c in cases]
            out = hip.render_batch(hip.make_desc(c0["sid"], c0["kid"], c0["cam"], c0["W"], c0["H"]),
                                   np.stack([c["cam"] for c in cases]), cfgs)
            for i, c in enumerate(cases):
                one = {"iters": out["iters"][i], "hit": out["hit"][i], "depth": out["depth"][i], "stats": out["stats"][i]}
                _check_lean(c, one, (name, full, cc.label(c)))


def test_explicit_rays_match_reference(hip):
    """rm_march_rays, and rm_march_rays_team for the Mandelbulb pairs: the device normalises the stored directions itself."""
    pairs = cc.ray_pairs()
    assert sum(1 for p in pairs if p["sid"] == 10) >= 3
    for p in pairs:
        for team in ((False, True) if p["sid"] == 10 else (False,)):
            hit, t, it, fs = hip.march_rays(p["sid"], p["kid"], p["o"], p["d"], p["max_iterations"], p["hit_threshold"],
                                            p["max_distance"], p["lipschitz"], team=team, params=p["prm"])
            bad = np.nonzero((it != p["iters"]) | (hit != p["hit"]) | (t.view(np.uint64) != p["t_bits"])
                             | (fs.view(np.uint64) != p["fs_bits"]))[0]
            assert len(bad) == 0, (p["n"], p["sid"], p["kid"], team, "first bad ray", int(bad[0]), p["d"][bad[0]].tolist())
