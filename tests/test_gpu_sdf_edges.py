"""The 20 scene SDFs at their edge points on the MI355X, against the REFERENCE's own values (tests/golden/sdf_edges.npz,
rays_edges.npz; layout and recipes in tests/sdf_edge_cases.py) -- bit for bit, NaN as one class, no oracle in between.

What only the device has, and no host build can show: the dense libm forms skip bands by wave ballot, rm_pow_half<true>
changes form at 16 live lanes, amdgcn lowers division and sqrt its own way at huge and tiny magnitudes, the ISA peephole,
and the team form of the union scenes and of the Mandelbulb.  So every scene is evaluated under wave layouts laid out on
purpose -- the path a lane takes depends on its neighbours, the value must not: fixture order, a permutation, prefixes of 1,
63, 64 and 65 points, a wave of 64 copies of an edge point, and the edge point alone among 63 ordinary points in lanes 0,
13, 31, 32, 63.  Then the same values through scene programs, the reference's marches from edge points (the team form
included), and frames from cameras that stand on an edge point.

Where the reference raises (tests/test_sdf_edges_host.py) nothing is pinned; what the device returns there is printed, and
it must not depend on the layout either."""
import numpy as np
import pytest

import sdf_edge_cases as ec

from raymarch_algo_compare_amd import _native
from raymarch_algo_compare_amd import scene_program as sp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def E():
    return ec.edges()


@pytest.fixture
def programs():
    """program ids made through this fixture are destroyed at teardown"""
    made = []

    def make(expr):
        ops, n = sp.to_ctypes(expr)
        made.append(_native.scene_program_create(ops, n))
        return made[-1]
    yield make
    for pid in made:
        try:
            _native.scene_program_destroy(pid)
        except _native.RmError:
            pass


def _classes(v):
    return f"NaN {int(np.isnan(v).sum())}, +inf {int((v == np.inf).sum())}, -inf {int((v == -np.inf).sum())}, finite {int(np.isfinite(v).sum())}"


# ---- rm_sdf_eval under every layout ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("sid", range(ec.NSCENES))
def test_sdf_eval_equals_the_reference_under_every_layout(hip, E, sid):
    n = len(E.pts)
    whole = hip.sdf_eval(sid, E.pts)
    report = ec.mismatches(E, sid, whole)
    assert not report, "fixture order\n" + report
    perm = ec.permutation(n)
    got = hip.sdf_eval(sid, E.pts[perm])
    report = ec.mismatches(E, sid, got, idx=perm)
    assert not report, "permuted\n" + report
    # ... and at the points nothing pins (the reference raised, or the sincos cut) the value is the same in both layouts
    assert ec.same_bits(got, whole[perm]), ("a value depends on the layout", int((ec.bits(got) != ec.bits(whole[perm])).sum()))
    for k in ec.PREFIXES:
        got = hip.sdf_eval(sid, E.pts[:k])
        report = ec.mismatches(E, sid, got, idx=np.arange(k))
        assert not report and ec.same_bits(got, whole[:k]), f"prefix of {k}\n" + report
    idx = ec.chosen(E, sid)
    pts, rep, lanes = ec.wave_of_copies(E, idx)
    report = ec.mismatches(E, sid, hip.sdf_eval(sid, pts), idx=rep, lanes=lanes)
    assert not report, "a wave of 64 copies\n" + report
    pts, pos, idx, lanes = ec.alone_in_wave(E, sid, idx)
    report = ec.mismatches(E, sid, hip.sdf_eval(sid, pts)[pos], idx=idx, lanes=lanes)
    assert not report, "alone among 63 ordinary points\n" + report
    unpinned = ~E.pinned(sid)
    if unpinned.any():
        print(f"scene {sid}: reference raised at {int(E.raised[sid].sum())} points, beyond the sincos cut {int(E.unclaimed[sid].sum())}; "
              f"the device returns {_classes(whole[unpinned])}")


def test_unpinned_points_on_the_device(hip, E):
    """Capped Torus where the reference goes complex and Gyroid beyond the sincos cut: NaN (include/rm_hip.h).  At the
    overflow points of Cylinder and Pillar Forest: what libm's pow makes of the square, +inf, i.e. the oracle's value (which
    tests/test_sdf_edges_host.py holds to the header build there)."""
    from oracle import oracle
    got = hip.sdf_eval(17, E.pts[E.raised[17]])
    assert np.isnan(got).all(), _classes(got)
    got = hip.sdf_eval(16, E.pts[E.unclaimed[16]])
    assert np.isnan(got).all(), _classes(got)
    for sid in (4, 12):
        pts = E.pts[E.raised[sid]]
        got, want = hip.sdf_eval(sid, pts), oracle.sdf_eval(sid, pts)
        print(f"scene {sid}, {len(pts)} overflow points of the reference: the device returns {_classes(got)}")
        bad = np.flatnonzero(ec.bits(got) != ec.bits(want))
        assert not len(bad), (sid, len(bad), pts[bad[0]].tolist(), float(got[bad[0]]), float(want[bad[0]]))
    assert (hip.sdf_eval(4, E.pts[E.raised[4]]) == np.inf).all()


# ---- the same values through scene programs --------------------------------------------------------------------------------

def test_programs_equal_the_reference(hip, E, programs):
    exprs = {**sp.catalogue_expressions(), **sp.catalogue_twins()}
    assert sorted(exprs) == sorted(ec.RESTATED + ec.TWINS)
    perm = ec.permutation(len(E.pts))
    for sid in sorted(exprs):
        pid = programs(exprs[sid])
        whole = hip.sdf_eval(pid, E.pts)
        report = ec.mismatches(E, sid, whole)
        assert not report, f"program of scene {sid}\n" + report
        got = hip.sdf_eval(pid, E.pts[perm])
        assert ec.same_bits(got, whole[perm]), (sid, "a value depends on the layout")
        if sid in (16, 17):
            assert np.isnan(whole[~E.pinned(sid)]).all(), sid
        if (~E.pinned(sid)).any():              # where nothing is pinned the program is the built-in scene still
            assert ec.same_bits(whole[~E.pinned(sid)], hip.sdf_eval(sid, E.pts[~E.pinned(sid)])), sid


# ---- the reference's marches from edge points ---------------------------------------------------------------------------------

def _localise(sid, kid, b, lip, got, R):
    """test_sdf_edges_host.py pins oracle.march_rays to the hash the device missed: the first ray that differs from it"""
    from oracle import oracle
    want = oracle.march_rays(sid, kid, R["o"], R["d"], max_iterations=b, lipschitz=lip)
    assert ec.cell_hash(want[0], want[2], want[1], want[3]) == R["sha"][sid, kid, R["budgets"].index(b)].tobytes()
    bad = np.flatnonzero((got[0] != want[0]) | (got[2] != want[2]) | (ec.bits(got[1]) != ec.bits(want[1])) | (ec.bits(got[3]) != ec.bits(want[3])))
    k = int(bad[0])
    return (f"{len(bad)} rays differ; ray {k} (lane {k % 64}) origin {R['o'][k].tolist()} direction {R['d'][k].tolist()}: hit {int(got[0][k])} / "
            f"{int(want[0][k])}, iterations {int(got[2][k])} / {int(want[2][k])}, t {float(got[1][k])!r} / {float(want[1][k])!r}, "
            f"final_sdf {float(got[3][k])!r} / {float(want[3][k])!r} (device / reference)")


@pytest.mark.parametrize("sid", range(ec.NSCENES))
def test_marches_equal_the_reference(hip, sid):
    R = ec.rays()
    for kid in range(ec.NSTRATEGIES):
        lip = float(R["lip"][sid, kid])
        for bi, b in enumerate(R["budgets"]):
            for team in ((False, True) if sid in ec.TEAM_SCENES else (False,)):
                got = hip.march_rays(sid, kid, R["o"], R["d"], max_iterations=b, lipschitz=lip, team=team)
                if ec.cell_hash(got[0], got[2], got[1], got[3]) != R["sha"][sid, kid, bi].tobytes():
                    pytest.fail(f"scene {sid}, strategy {kid}, budget {b}, team {team}: " + _localise(sid, kid, b, lip, got, R))


# ---- frames from a camera standing on an edge point ------------------------------------------------------------------------

W, H = 16, 12
# (what the camera stands on, position, target, scenes): every ray of the frame starts at the edge point, so the first
# evaluation of all 192 lanes is the edge itself and the second leaves it in 192 directions
CAMERAS = [("the origin", (0.0, 0.0, 0.0), (0.0, 0.0, -1.0), (0, 9, 10, 14, 15, 16, 18)),
           ("a Mandelbulb pole", (0.0, -0.0, 1.1), (0.0, 0.0, 0.0), (10,)),
           ("a Sphere Cloud centre", (0.4253, 1.3505, 0.9373), (0.0, 0.0, 0.0), (14, 10)),
           ("a Menger jump plane", (2.0 / 3.0, 0.2, 1.5), (0.0, 0.0, 0.0), (9, 10)),
           ("a lattice tie", (0.5, 1.5, -2.5), (0.0, 0.0, 0.0), (18, 15))]
# suspend_after = (1, 1): every ray still marching after one trip is parked.  In passes the one resume pass is then the
# team pass of a team scene.  A single launch has teams only for suspend_after[1] > suspend_after[0] (csrc/rm_launch_plan.h:
# otherwise the second level is dropped, and the split form, which is a team kernel of its own, is refused), so the fused
# and the split single launch also run at (1, 2): struck after one trip, handed to the teams after two.
PARKED, TEAMS = dict(suspend_after=(1, 1)), dict(suspend_after=(1, 2))
SCHEDULES = [("passes", dict(pipeline=1, **PARKED), False), ("single launch", dict(pipeline=2, **PARKED), False),
             ("single launch with teams", dict(pipeline=2, pipeline_form=1, **TEAMS), True),
             ("split", dict(pipeline=2, pipeline_form=2, **TEAMS), True)]      # the last two: scenes with a team form


@pytest.mark.parametrize("cam", range(len(CAMERAS)))
def test_frames_from_an_edge_point_equal_the_oracle(hip, cam):
    from oracle import oracle
    from raymarch_algo_compare_amd.camera import Camera
    what, pos, tgt, scenes = CAMERAS[cam]
    c14 = Camera(pos, tgt, (0.0, 1.0, 0.0), 60.0, W, H).params14()
    for sid in scenes:
        for kid in (0, 6):
            for b in (1, 2, 8):
                ref = oracle.render(sid, kid, c14, W, H, max_iterations=b)
                for name, sched, team_only in SCHEDULES:
                    if team_only and sid not in ec.TEAM_SCENES:
                        continue
                    out = hip.render(hip.make_desc(sid, kid, c14, W, H, max_iterations=b, full=True, **sched), want_t_raw=True, want_final_sdf=True)
                    tag = (what, sid, kid, b, name)
                    assert (out["iters"] == ref.iters).all() and (out["hit"] == ref.hit).all(), tag
                    assert ec.same_bits(out["t_raw"], ref.t) and ec.same_bits(out["final_sdf"], ref.final_sdf), tag
                    st = out["stats"]
                    assert (st["total_rays"], st["hit_count"], st["sum_iters"]) == (W * H, int(ref.hit.sum()), int(ref.iters.sum())), tag
                    assert (st["iter_min"], st["iter_max"]) == (int(ref.iters.min()), int(ref.iters.max())), tag
