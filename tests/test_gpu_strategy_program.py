"""Strategy programs on a real MI355X: the interpreter's kernels (csrc/rm_strategy_tu.hip) against the compiled
strategies their twins restate -- frames, rays, batches, capture -- against the NumPy machine for a strategy no
catalogue entry has, the evaluation budget, edges, lifetime and the registry."""
import numpy as np
import pytest

import strategy_program_cases as cases
from oracle import oracle
from raymarch_algo_compare_amd import _native, registry
from raymarch_algo_compare_amd import scene_program as scp
from raymarch_algo_compare_amd import strategy_program as sp
from raymarch_algo_compare_amd.camera import Camera
from raymarch_algo_compare_amd.config import MarchConfig, RenderConfig

pytestmark = pytest.mark.gpu

FRAME_SCENES = [0, 6, 10, 11, 12, 13]
W, H = 64, 48


def _cam(scene_id, w=W, h=H):
    s = registry.get_scene_by_id(scene_id)
    pos = (s.camera_position if s is not None else None) or (0.0, 0.0, 5.0)
    tgt = (s.camera_target if s is not None else None) or (0.0, 0.0, 0.0)
    return Camera(pos, tgt, (0.0, 1.0, 0.0), 60.0, w, h).params14()


@pytest.fixture(scope="module")
def twins(hip):
    """[(name, compiled id, program id, RmStrategyParams overrides)], destroyed at the end of the module"""
    made = [(name, kid, hip.strategy_program_create(prog.to_ops(), len(prog)), prm) for name, kid, prog, prm in cases.twin_cases()]
    yield made
    for _, _, pid, _ in made:
        hip.strategy_program_destroy(pid)


@pytest.fixture(scope="module")
def user_scene(hip):
    expr = scp.op_smooth_union(scp.sd_box((1, 1, 1)), scp.op_translate((1.2, 0.3, 0), scp.sd_sphere(0.8)), 0.3)
    info = scp.register_scene("Strategy Program Test Blob", expr)
    yield info.id
    scp.unregister_scene("Strategy Program Test Blob")


@pytest.fixture(scope="module")
def ext_scene(hip):
    """a scene program with an op beyond primitives.py: rendered by the kernels of strat_progext.o"""
    expr = scp.op_union(scp.op_scale(scp.sd_box((1, 1, 1)), 0.7), scp.op_translate((1.4, 0.2, 0), scp.sd_sphere(0.6)))
    info = scp.register_scene("Strategy Program Test Scaled Box", expr)
    yield info.id
    scp.unregister_scene("Strategy Program Test Scaled Box")


def _frame(hip, scene_id, kid, cam, w, h, full, prm, max_iterations=512):
    desc = hip.make_desc(scene_id, kid, cam, w, h, 0, None, max_iterations, 1e-4, 100.0, 1.0, full, params=prm or None)
    return hip.render(desc, want_t_raw=True, want_final_sdf=bool(full), want_evals=True)


def _same(a, b, what, full=True):
    for k in ("iters", "hit", "depth", "evals"):
        assert np.array_equal(a[k], b[k]), (what, k)
    for k in ("t_raw",) + (("final_sdf",) if full else ()):
        assert np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)), (what, k)
    for k, v in a["stats"].items():
        assert np.array_equal(v, b["stats"][k]), (what, "stats", k)


@pytest.mark.parametrize("scene", FRAME_SCENES + ["user", "ext"])
def test_twin_frames_equal_compiled_kernels(hip, twins, user_scene, ext_scene, scene):
    sid = {"user": user_scene, "ext": ext_scene}.get(scene, scene)
    cam = _cam(sid)
    for name, kid, pid, prm in twins:
        for full in (True, False):
            _same(_frame(hip, sid, pid, cam, W, H, full, None), _frame(hip, sid, kid, cam, W, H, full, prm), (scene, name, full), full)


@pytest.mark.parametrize("scene", FRAME_SCENES + ["user", "ext"])
def test_twin_rays_equal_compiled_kernels(hip, twins, user_scene, ext_scene, scene):
    sid = {"user": user_scene, "ext": ext_scene}.get(scene, scene)
    o, d = cases.rays(scene if isinstance(scene, int) else 0, 3000)
    for name, kid, pid, prm in twins:
        a = hip.march_rays(sid, pid, o, d)
        b = hip.march_rays(sid, kid, o, d, params=prm or None)
        keys = ("hit", "t", "iters", "final_sdf")
        assert cases.same_bits(dict(zip(keys, a)), dict(zip(keys, b))) == [], (scene, name)


def test_batch_equals_single_frames(hip, twins):
    w, h = 32, 24
    cams = np.stack([Camera((x, 0.5, 5.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 60.0, w, h).params14() for x in (-2.0, 0.0, 1.5, 3.0)])
    cfgs = [{"max_iterations": m, "hit_threshold": e, "full": True} for m, e in ((512, 1e-4), (100, 1e-4), (64, 1e-6), (7, 1e-3))]
    for name, kid, pid, prm in twins:
        if prm:
            continue
        b = hip.render_batch(hip.make_desc(6, pid, cams[0], w, h, full=True), cams, cfgs, want_evals=True)
        for f in range(4):
            desc = hip.make_desc(6, pid, cams[f], w, h, 0, None, cfgs[f]["max_iterations"], cfgs[f]["hit_threshold"], 100.0, 1.0, True)
            one = hip.render(desc, want_evals=True)
            for k in ("iters", "hit", "depth", "evals"):
                assert np.array_equal(b[k][f], one[k]), (name, f, k)
            assert b["stats"][f]["sum_iters"] == one["stats"]["sum_iters"]


def test_capture_equals_compiled_twin(hip, twins):
    name, kid, pid, prm = twins[-2]      # Overstep-Bisect, defaults
    assert kid == 6 and not prm
    cam = _cam(6)
    a = hip.capture(hip.make_desc(6, pid, cam, W, H, full=True))
    b = hip.capture(hip.make_desc(6, kid, cam, W, H, full=True))
    for k in ("geom", "normal", "depth", "color", "evals", "hit"):
        if k in a and isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k], equal_nan=True), k


@pytest.mark.parametrize("scene", [0, 12])
def test_new_strategy_equals_run_host(hip, scene):
    prog = sp.understep_relax()
    pid = hip.strategy_program_create(prog.to_ops(), len(prog))
    try:
        o, d = cases.rays(scene, 2000)
        a = hip.march_rays(scene, pid, o, d)
    finally:
        hip.strategy_program_destroy(pid)
    b = sp.run_host(prog, lambda p: oracle.sdf_eval(scene, p), o, d, {"max_iterations": 512}, full=True)
    keys = ("hit", "t", "iters", "final_sdf")
    assert cases.same_bits(dict(zip(keys, a)), b) == []
    assert a[0].any() and not a[0].all()


def test_budget_force_finishes_every_ray(hip):
    prog = sp.budget_probe(10)
    pid = hip.strategy_program_create(prog.to_ops(), len(prog))
    try:
        out = _frame(hip, 0, pid, _cam(0, 16, 12), 16, 12, True, None, max_iterations=4)
    finally:
        hip.strategy_program_destroy(pid)
    assert not out["hit"].any()
    assert (out["evals"] == sp.budget(4)).all() and (out["iters"] == sp.budget(4)).all()
    assert out["stats"]["sum_evals"] == 16 * 12 * sp.budget(4)


def test_edges(hip, twins):
    name, kid, pid, prm = twins[0]
    for w, h, mi in ((1, 1, 512), (65, 5, 512), (64, 48, 0)):
        cam = _cam(0, w, h)
        _same(_frame(hip, 0, pid, cam, w, h, True, None, mi), _frame(hip, 0, kid, cam, w, h, True, None, mi), (w, h, mi))
    ob = [t for t in twins if t[1] == 6 and not t[3]][0]
    cam = _cam(6)
    for mi in (0, 16):      # Overstep-Bisect: an init block that finishes the ray / goes straight to the bisection's exit
        _same(_frame(hip, 6, ob[2], cam, W, H, True, None, mi), _frame(hip, 6, 6, cam, W, H, True, None, mi), ("ob", mi))


def test_lifetime(hip):
    cam = _cam(2)
    before = _frame(hip, 2, 4, cam, W, H, True, None)
    pa, pb = sp.twin_standard(), sp.twin_relaxed()
    a = hip.strategy_program_create(pa.to_ops(), len(pa))
    b = hip.strategy_program_create(pb.to_ops(), len(pb))
    try:
        fa, fb = _frame(hip, 2, a, cam, W, H, True, None), _frame(hip, 2, b, cam, W, H, True, None)
        _same(fa, _frame(hip, 2, 0, cam, W, H, True, None), "a")
        _same(fb, _frame(hip, 2, 1, cam, W, H, True, None), "b")
        _same(_frame(hip, 2, a, cam, W, H, True, None), fa, "a again")
        o, d = cases.rays(2, 64)
        with pytest.raises(hip.RmError) as e:
            hip.march_rays(2, a, o, d, team=True)
        assert e.value.code == hip.RM_E_BAD_STRATEGY and "team" in str(e.value)
        with pytest.raises(hip.RmError) as e:
            hip.march_rays(10, a, o, d, team=True)
        assert e.value.code == hip.RM_E_BAD_STRATEGY
    finally:
        hip.strategy_program_destroy(a)
        hip.strategy_program_destroy(b)
    for call in (lambda: _frame(hip, 2, a, cam, W, H, True, None), lambda: hip.march_rays(2, a, *cases.rays(2, 8))):
        with pytest.raises(hip.RmError) as e:
            call()
        assert e.value.code == hip.RM_E_BAD_STRATEGY and "does not exist" in str(e.value)
    for bad in (13, 1023):
        with pytest.raises(hip.RmError) as e:
            _frame(hip, 2, bad, cam, W, H, True, None)
        assert e.value.code == hip.RM_E_BAD_STRATEGY and f"strategy_id {bad} out of range" in str(e.value)
    _same(_frame(hip, 2, 4, cam, W, H, True, None), before, "compiled strategy after programs came and went")


def test_registry_resolves_a_registered_strategy(hip):
    from raymarch_algo_compare_amd.main import run_once
    from raymarch_algo_compare_amd.sweep import run_sweep
    info = sp.register_strategy("Understep-Relax", sp.understep_relax())
    twin = sp.register_strategy("Plain-Twin", sp.twin_standard())
    try:
        assert registry.get_strategy_by_name("understep-relax").id == info.id >= _native.RM_STRATEGY_PROGRAM_BASE
        assert "Understep-Relax" not in registry.list_strategies() and len(registry.list_strategies()) == 11
        with pytest.raises(ValueError):
            sp.register_strategy("Understep-Relax", sp.understep_relax())
        with pytest.raises(ValueError):
            sp.register_strategy("Standard", sp.understep_relax())
        st = run_once(RenderConfig(width=W, height=H), MarchConfig(), "Cube", "Understep-Relax")
        direct = _frame(hip, 2, info.id, _cam(2), W, H, True, None)
        assert st.hit_count == int(direct["hit"].sum()) and st.iteration_max == int(direct["iters"].max())
        assert st.iteration_mean == pytest.approx(float(direct["iters"].mean()), rel=1e-12)
        rows = run_sweep(["Sphere"], ["Understep-Relax"], "budget", 32, 24, budgets=[64])
        ref = run_sweep(["Sphere"], ["Plain-Twin"], "budget", 32, 24, budgets=[64])
        std = run_sweep(["Sphere"], ["Standard"], "budget", 32, 24, budgets=[64])
        assert rows and all(r["strategy"] == "Understep-Relax" for r in rows)
        assert len(ref) == len(std)
        for r, s in zip(ref, std):
            for k in ("viewpoint", "iters_mean", "iters_max", "evals_mean", "evals_max", "hit_rate", "divergence_proxy"):
                assert r[k] == s[k], k
    finally:
        sp.unregister_strategy("Understep-Relax")
        sp.unregister_strategy("Plain-Twin")
    assert registry.get_strategy_by_name("Understep-Relax") is None
