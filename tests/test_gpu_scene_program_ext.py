"""The four scene-program ops beyond primitives.py and the five catalogue twins on the MI355X: the device against the host
build (tests/native/program_ext_check.cpp) bit for bit in all four evaluations, on the inputs of
tests/test_scene_program_ext_host.py; a twin's frames against its catalogue scene's; the Bad Lipschitz twin against the
unit sphere in the oracle; no tunnelling of the oracle on the other four twins; the sweep's --oracle-twins.

Every program made here is destroyed by the fixture that made it."""
import numpy as np
import pytest

import program_ext_cases as cases
from program_ext_cases import bits

from raymarch_algo_compare_amd import _native, registry, sweep
from raymarch_algo_compare_amd import scene_program as sp
from raymarch_algo_compare_amd.camera import Camera

pytestmark = pytest.mark.gpu

PROGRAMS = cases.programs()
W, H = 48, 36


@pytest.fixture(scope="module")
def host():
    return cases.Host()


@pytest.fixture
def programs(hip):
    """program ids made through this fixture are destroyed at teardown"""
    made = []

    def make(expr, lipschitz=1.0):
        ops, n = sp.to_ctypes(expr)
        made.append(_native.scene_program_create(ops, n, lipschitz))
        return made[-1]
    yield make
    for pid in made:
        try:
            _native.scene_program_destroy(pid)
        except _native.RmError:
            pass


def _camera(scene):
    return Camera(scene.camera_position or (0.0, 0.0, 5.0), scene.camera_target or (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 60.0,
                  W, H).params14()


def _same(a, b, what):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    bad = np.argwhere(bits(a) != bits(b))
    assert bad.size == 0, (what, len(bad), bad[:4], a[tuple(bad[0])], b[tuple(bad[0])])


# ---- 1. the device equals the host build ----------------------------------------------------------------------------

@pytest.mark.parametrize("idx", range(len(PROGRAMS)), ids=cases.NAMES)
def test_device_equals_host_in_all_four_evaluations(host, programs, idx):
    name, expr, off = PROGRAMS[idx]
    pid = programs(expr)
    pts = np.concatenate([cases.special_points(off), np.random.default_rng(0).uniform(-3.5, 3.5, size=(2000, 3))])
    _same(_native.sdf_eval(pid, pts), host.point(expr, pts), (name, "rm_sdf_eval"))
    lo, hi = cases.boxes(100 + idx, off)
    dlo, dhi = _native.interval_sdf_eval(pid, lo, hi)
    _same(np.stack([dlo, dhi], axis=1), host.interval(expr, lo, hi), (name, "rm_interval_sdf_eval"))
    segs = cases.segments(300 + idx)
    dual, box = host.dual(expr, segs)
    dev = _native.segment_sdf_eval(pid, segs)
    _same(dev, dual, (name, "rm_segment_sdf_eval"))
    _same(dev[:, :2], box, (name, "rm_segment_sdf_eval val against the interval range"))
    for mode in (_native.RM_RANGE_AFFINE, _native.RM_RANGE_MEET):
        rng, _ = _native.affine_range_eval(pid, segs, mode, want_form=False)
        _same(rng, host.affine(expr, mode, segs), (name, "rm_affine_range_eval", mode))


# ---- 2. a twin's frames are its catalogue scene's ------------------------------------------------------------------------

@pytest.mark.parametrize("sid", cases.TWIN_IDS)
def test_twin_frames_equal_the_catalogue_frames(programs, sid):
    scene = registry.SCENES[sid]
    pid = programs(sp.catalogue_twins()[sid], scene.lipschitz)
    cam = _camera(scene)
    mixed = False                                          # (Standard overshoots every ray of Bad Lipschitz Sphere: no hit)
    for key in ("Standard", "Segment", "Overstep-Bisect"):
        kid = registry.STRATEGIES[key]
        want = _native.render(_native.make_desc(sid, kid, cam, W, H, full=True, lipschitz=scene.lipschitz), want_t_raw=True,
                              want_final_sdf=True)
        got = _native.render(_native.make_desc(pid, kid, cam, W, H, full=True, lipschitz=scene.lipschitz), want_t_raw=True,
                             want_final_sdf=True)
        assert np.array_equal(got["iters"], want["iters"]), (scene.name, key, int((got["iters"] != want["iters"]).sum()))
        assert np.array_equal(got["hit"], want["hit"]), (scene.name, key)
        _same(got["t_raw"], want["t_raw"], (scene.name, key, "t"))
        _same(got["final_sdf"], want["final_sdf"], (scene.name, key, "final_sdf"))
        mixed = mixed or 0 < int(want["hit"].sum()) < W * H
    assert mixed, (scene.name, "no frame with hits and misses")


# ---- 3. the Bad Lipschitz twin ------------------------------------------------------------------------------------------

def test_bad_lipschitz_twin_in_the_oracle_and_the_segment_tracer(programs):
    """Scaling by 2 is exact and changes no sign test: the oracle's frame of the twin is the unit sphere's.  The segment
    tracer, whose derivative range scales with the value, hits the same pixels."""
    scene = registry.SCENES[11]
    pid = programs(sp.catalogue_twins()[11], scene.lipschitz)
    cam = _camera(scene)
    cfg = _native.interval_config(bound_radius=1.05)
    twin = _native.interval_render(pid, cam, W, H, cfg, want_normal=False)
    unit = _native.interval_render(0, cam, W, H, cfg, want_normal=False)
    assert np.array_equal(twin["hit"], unit["hit"]) and np.array_equal(twin["steps"], unit["steps"])
    _same(twin["depth"], unit["depth"], "depth")
    assert 0.05 <= twin["hit"].mean() <= 0.95
    seg = _native.segment_render(pid, cam, W, H, _native.segment_config(bound_radius=1.05, l_global=2.0))
    assert np.array_equal(seg["hit"], twin["hit"])


# ---- 4. the oracle does not tunnel ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("sid", [9, 15, 16, 18])
def test_oracle_of_the_twin_is_sound_against_the_point_samples(programs, sid, capsys):
    """2048 equally spaced samples of every ray in [0, min(t_hit, t_max)): each is > 0 -- before an oracle hit and along an
    oracle miss.  The frame has hits and misses.  The IoU against the catalogue scene's Dense-March capture is printed (a
    finding: DESIGN.md section 3, "Program extensions")."""
    from raymarch_algo_compare_amd.runner import ray_directions
    scene = registry.SCENES[sid]
    pid = programs(sp.catalogue_twins()[sid], scene.lipschitz)
    cam14 = _camera(scene)
    t_max = 100.0                                          # the oracle's default
    out = _native.interval_render(pid, cam14, W, H, want_normal=False)
    hit = out["hit"].astype(bool).ravel()
    rate = float(hit.mean())
    assert 0.05 <= rate <= 0.95, (scene.name, rate)
    cam = Camera(scene.camera_position or (0.0, 0.0, 5.0), scene.camera_target or (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 60.0, W, H)
    rd = np.asarray(ray_directions(cam), dtype=np.float64).reshape(-1, 3)
    ro = np.asarray(cam14[:3], dtype=np.float64)
    end = np.where(hit, np.minimum(out["depth"].ravel(), t_max), t_max)
    t = end[:, None] * (np.arange(2048) / 2048.0)[None, :]
    f = _native.sdf_eval(pid, (ro[None, None, :] + t[..., None] * rd[:, None, :]).reshape(-1, 3)).reshape(t.shape)
    bad = np.argwhere(~(f > 0.0))
    assert bad.size == 0, (scene.name, len(bad), bad[:4], f[tuple(bad[0])], t[tuple(bad[0])])
    dense = _native.render(_native.make_desc(sid, registry.SHADER_ONLY_STRATEGIES["Dense-March"], cam14, W, H))
    dh = dense["hit"].astype(bool).ravel()
    union = int((dh | hit).sum())
    with capsys.disabled():
        print(f"\noracle of the {scene.name} twin, {W}x{H}: hit rate {rate:.4f}, IoU against Dense-March "
              f"{int((dh & hit).sum()) / max(union, 1):.4f} (dense hits {int(dh.sum())}, oracle hits {int(hit.sum())})")


# ---- 5. the sweep -------------------------------------------------------------------------------------------------------

def test_sweep_scores_box_lattice_against_its_twin(hip):
    name = sp.twin_name("Box Lattice")
    try:
        rows = sweep.run_sweep(["Box Lattice"], ["Standard"], "budget", W, H, budgets=[32, 256], oracle="interval",
                               ceiling="segment", oracle_twins=True)
        assert rows and all(r["scene"] == "Box Lattice" for r in rows)
        for r in rows:
            for k in sweep.ORACLE_FIELDS + sweep.CEILING_FIELDS:
                assert r[k] is not None and np.isfinite(r[k]), (k, r[k])
        assert all(0.0 < r["oracle_iou"] <= 1.0 for r in rows) and all(r["ceiling_iou"] > 0.9 for r in rows)
        assert registry.find_program_scene(name) is not None
    finally:
        if registry.find_program_scene(name) is not None:
            sp.unregister_scene(name)
    plain = sweep.run_sweep(["Box Lattice"], ["Standard"], "budget", W, H, budgets=[32, 256], oracle="interval", ceiling="segment")
    assert len(plain) == len(rows)
    assert all(r[k] is None for r in plain for k in sweep.ORACLE_FIELDS + sweep.CEILING_FIELDS)
    assert registry.find_program_scene(name) is None
    drop = set(sweep.ORACLE_FIELDS + sweep.CEILING_FIELDS + ["ms_per_frame"])
    assert [{k: v for k, v in r.items() if k not in drop} for r in rows] == \
        [{k: v for k, v in r.items() if k not in drop} for r in plain]
