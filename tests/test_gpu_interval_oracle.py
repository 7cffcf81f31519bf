"""The interval first-hit oracle on the MI355X: rm_interval_* against the reference's own results (tests/golden/
interval_*.npz), against the host build of csrc/rm_interval.h (tests/native/interval_check.cpp), no tunnelling against
the pointwise SDF, the closed forms of analytic.py, the lifecycle of program ids, and the sweep's oracle columns.

Every program made here is destroyed by the fixture that made it, so the other suites see the catalogue scenes only."""
import ctypes
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from test_interval_host import (CATALOGUE_IDS, DEEP_PROGRAMS, _cfg, bits, check_frame, frame_cases, host_eval, host_march, host_render,
                                load_host_lib, ray_cases)

from raymarch_algo_compare_amd import _native, analytic, registry, scoring, sweep
from raymarch_algo_compare_amd import interval_oracle as io
from raymarch_algo_compare_amd import scene_program as sp
from raymarch_algo_compare_amd.camera import Camera
from raymarch_algo_compare_amd.viewpoints import viewpoints_for

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host():
    return load_host_lib()


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


# ---- 1. the reference's fixtures, bit for bit ---------------------------------------------------------------------------

def test_render_matches_reference():
    n = 0
    for p, sid, W, H, cam, cfg, want_hit, want_t, n_sha, n_bits in frame_cases():
        out = _native.interval_render(sid, cam, W, H, _cfg(cfg))
        check_frame(out["depth"].ravel(), out["hit"].ravel(), out["normal"].reshape(-1, 3), want_hit, want_t, n_sha, n_bits, p)
        n += 1
    assert n == 12


def test_march_rays_matches_reference():
    n = 0
    for p, sid, o, d, cfg, want_t, want_n in ray_cases():
        t, steps, nrm = _native.interval_march_rays(sid, o, d, _cfg(cfg))
        assert np.array_equal(bits(t), want_t), (p, np.nonzero(bits(t) != want_t)[0][:8])
        assert np.array_equal(bits(nrm), want_n), p
        n += 1
    assert n == 10


# ---- 2. the device against the host build ------------------------------------------------------------------------------

def _trees(k=6):
    with open(os.path.join(GOLDEN, "programs_trees.json"), encoding="utf-8") as f:
        trees = json.load(f)["trees"]
    return [sp.expr_from_json(t) for t in trees[:k]] + [e for _, e in DEEP_PROGRAMS]


def _compare(host, sid_dev, expr, scene_bound, cam14, W, H, what):
    ops, n = sp.to_ctypes(expr)
    depth, hit, nrm, steps = host_render(host, ops, n, _native.interval_config(), scene_bound, cam14, W, H)
    out = _native.interval_render(sid_dev, cam14, W, H)
    assert np.array_equal(out["hit"].ravel(), hit), what
    assert np.array_equal(bits(out["depth"].ravel()), bits(depth)), what
    assert np.array_equal(bits(out["normal"].reshape(-1, 3)), bits(nrm)), what
    assert np.array_equal(out["steps"].ravel(), steps), what


@pytest.mark.parametrize("sid", CATALOGUE_IDS)
def test_device_equals_host_catalogue(host, sid):
    ex = sp.catalogue_expressions()[sid]
    for vp in viewpoints_for(registry.SCENES[sid]):
        cam = Camera(vp.position, vp.target, vp.up, 60.0, 96, 72).params14()
        _compare(host, sid, ex, host.rmi_scene_bound(sid), cam, 96, 72, (sid, vp.name))


def test_device_equals_host_programs(host, programs):
    cam = Camera((0.3, 1.2, 5.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 60.0, 96, 72).params14()
    for i, expr in enumerate(_trees()):
        pid = programs(expr)
        _compare(host, pid, expr, -1.0, cam, 96, 72, f"tree {i}")
        # explicit rays, unnormalised directions included
        rng = np.random.default_rng(i)
        o = rng.uniform(-4, 4, size=(300, 3))
        d = -o + rng.normal(size=o.shape)
        ops, n = sp.to_ctypes(expr)
        t_h, s_h, n_h = host_march(host, ops, n, _native.interval_config(), o, d)
        t_d, s_d, n_d = _native.interval_march_rays(pid, o, d)
        assert np.array_equal(bits(t_d), bits(t_h)) and np.array_equal(s_d, s_h) and np.array_equal(bits(n_d), bits(n_h)), i


def test_sdf_eval_equals_host(host):
    rng = np.random.default_rng(5)
    c = rng.uniform(-3, 3, size=(4000, 3))
    e = 10.0 ** rng.uniform(-6, 0, size=(4000, 3))
    for sid in CATALOGUE_IDS:
        ops, n = sp.to_ctypes(sp.catalogue_expressions()[sid])
        lo_h, hi_h = host_eval(host, ops, n, c - e, c + e)
        lo_d, hi_d = io.interval_sdf(sid, c - e, c + e)
        assert np.array_equal(bits(lo_d), bits(lo_h)) and np.array_equal(bits(hi_d), bits(hi_h)), sid


# ---- 3. no tunnelling ---------------------------------------------------------------------------------------------------

def _strategy_overshoot(sid, cam, o_t):
    """pixels where a strategy's frame hits beyond the oracle's first hit, or misses where the oracle hits"""
    out = {}
    for key in ("Standard", "Relaxed"):
        kid = registry.STRATEGIES[key]
        r = _native.render(_native.make_desc(sid, kid, cam.params14(), cam.width, cam.height, full=True), want_t_raw=True)
        h = r["hit"] > 0
        ok = np.isfinite(o_t)
        out[key] = int((ok & (~h | (r["t_raw"] > o_t + 1e-3))).sum())
    return out


@pytest.mark.parametrize("sid", CATALOGUE_IDS)
def test_no_tunnelling(sid):
    scene = registry.SCENES[sid]
    vp = viewpoints_for(scene)[0]
    cam = Camera(vp.position, vp.target, vp.up, 60.0, 64, 48)
    o, d = analytic.camera_rays(cam)
    d = d.reshape(-1, 3)
    o = np.broadcast_to(o, d.shape)
    t, steps, _ = _native.interval_march_rays(sid, o, d, want_normals=False)
    capped = steps >= 20000
    assert int(capped.sum()) == 0, f"{scene.name}: {int(capped.sum())} rays used up max_steps"
    end = np.where(np.isfinite(t), t, io.DEFAULT_T_MAX)
    K = 2048
    s = np.arange(K) / K                                  # evenly spaced on [0, end)
    worst = np.inf
    for a in range(0, len(d), 256):
        b = min(a + 256, len(d))
        pts = o[a:b, None, :] + (end[a:b, None] * s[None, :])[..., None] * d[a:b, None, :]
        f = _native.sdf_eval(sid, pts.reshape(-1, 3))
        worst = min(worst, float(f.min()))
    assert worst >= -1e-12, f"{scene.name}: the SDF is {worst} before the oracle's first hit"
    if sid in (3, 13):
        print(f"{scene.name}: pixels past the oracle's first hit {_strategy_overshoot(sid, cam, np.where(np.isfinite(t), t, np.inf).reshape(48, 64))}")


# ---- 4. the closed forms ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["Sphere", "Cube", "Thin Torus", "Grazing Plane"])
def test_against_closed_forms(name):
    scene = registry.get_scene_by_name(name)
    rc = scene.suggested_camera()
    pos, tgt = (rc.camera_position, rc.camera_target) if rc else ((0.0, 0.0, 5.0), (0.0, 0.0, 0.0))
    cam = Camera(pos, tgt, (0.0, 1.0, 0.0), 60.0, 160, 120)
    a_depth, a_hit, _ = analytic.analytic_depth(name, cam)
    o, d = analytic.camera_rays(cam)
    t = io.first_hit(o, d.reshape(-1, 3), scene).reshape(120, 160)
    o_hit = np.isfinite(t)
    want = a_hit & (a_depth <= io.DEFAULT_T_MAX)
    assert not (want & ~o_hit).any(), f"{name}: {int((want & ~o_hit).sum())} analytic hits the oracle misses"
    both = want & o_hit
    assert np.all(t[both] <= a_depth[both] + 1e-9), name
    P = o[None, :] + t[o_hit][:, None] * d[o_hit]
    f = _native.sdf_eval(scene.id, P)
    assert np.all(np.abs(f) <= 16 * io.DEFAULT_TOL), (name, float(np.abs(f).max()))


# ---- 5. lifecycle and timing --------------------------------------------------------------------------------------------

def test_lifecycle_and_timing(programs):
    pid = programs(sp.op_subtract(sp.sd_box((1.0, 1.0, 1.0)), sp.sd_sphere(1.3)))
    cam = Camera((2.0, 2.0, 4.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 60.0, 64, 48).params14()
    a = _native.interval_render(pid, cam, 64, 48, repeats=3, warmup=1)
    b = _native.interval_render(6, cam, 64, 48)                       # Hollow Cube: the same program
    assert np.array_equal(a["hit"], b["hit"]) and np.array_equal(bits(a["depth"]), bits(b["depth"]))
    tm = a["timing"]
    assert tm["repeats"] == 3 and len(tm["ms_each"]) == 3 and all(x > 0 for x in tm["ms_each"])
    assert tm["ms_min"] <= tm["ms_median"] <= tm["ms_max"]
    _native.scene_program_destroy(pid)
    for call in (lambda: _native.interval_render(pid, cam, 64, 48), lambda: _native.interval_march_rays(pid, [[0, 0, 5]], [[0, 0, -1]]),
                 lambda: _native.interval_sdf_eval(pid, [[0, 0, 0]], [[0, 0, 0]])):
        with pytest.raises(_native.RmError) as e:
            call()
        assert e.value.code == _native.RM_E_BAD_SCENE
    mandelbulb = registry.get_scene_by_name("Mandelbulb").id
    with pytest.raises(_native.RmError) as e:
        _native.interval_render(mandelbulb, cam, 64, 48)
    assert e.value.code == _native.RM_E_BAD_SCENE
    assert io.interval_capture("Mandelbulb", Camera((0, 0, 3), (0, 0, 0), (0, 1, 0), 60.0, 8, 8)) is None


def test_capture_rows_and_dtypes():
    cam = Camera((0.0, 0.0, 5.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 60.0, 40, 30)
    cap = io.interval_capture("Sphere", cam)
    assert cap["depth"].dtype == np.float64 and cap["hit"].dtype == bool and cap["normal"].dtype == np.float64
    assert cap["depth"].shape == (30, 40) and cap["normal"].shape == (30, 40, 3) and cap["steps"].dtype == np.int32
    # a row slice is the same rows of the whole frame
    part = _native.interval_render(0, cam.params14(), 40, 30, row0=7, rows=11)
    assert np.array_equal(bits(part["depth"]), bits(cap["depth"][7:18]))


# ---- 6. the sweep's oracle columns --------------------------------------------------------------------------------------

def test_sweep_oracle_columns(tmp_path):
    W = H = 48
    rows = sweep.run_sweep(["Thin Torus", "Menger"], ["Standard", "Relaxed"], "budget", W, H, budgets=[16, 64],
                           oracle="interval", out_path=str(tmp_path / "s.csv"))
    assert len(rows) > 0
    oracle = {}
    for r in rows:
        scene = registry.get_scene_by_name(r["scene"])
        if scene.name.startswith("Menger"):
            assert all(r[k] is None for k in sweep.ORACLE_FIELDS), r
            continue
        vp = next(v for v in viewpoints_for(scene) if v.name == r["viewpoint"])
        cam = Camera(vp.position, vp.target, vp.up, 60.0, W, H)
        if vp.name not in oracle:
            oracle[vp.name] = io.interval_capture(scene, cam)
        strat = registry.get_strategy_by_name(r["strategy"])
        # the sweep's frames are rm_render_batch frames: fp32 depth, as rm_render's `depth`
        out = _native.render(_native.make_desc(scene.id, strat.id, cam.params14(), W, H, max_iterations=r["max_iterations"],
                                               hit_threshold=r["hit_threshold"]))
        hit = out["hit"] > 0
        s = scoring.score_capture({"hit": hit, "depth": out["depth"], "normal": np.zeros((H, W, 3))},
                                  oracle[vp.name], compute_ssim=False)
        want = {"oracle_iou": s["hit"]["iou"], "oracle_false_hit": s["hit"]["false_hit_rate"],
                "oracle_false_miss": s["hit"]["false_miss_rate"], "oracle_depth_mae": s["depth"]["mae"],
                "oracle_depth_rmse": s["depth"]["rmse"], "oracle_depth_p95": s["depth"]["p95"]}
        for k, v in want.items():
            assert r[k] == pytest.approx(v, nan_ok=True), (r["strategy"], r["viewpoint"], k)
        assert 0.0 <= r["oracle_iou"] <= 1.0 and 0.0 <= r["oracle_false_hit"] <= 1.0 and 0.0 <= r["oracle_false_miss"] <= 1.0
        assert r["oracle_depth_mae"] >= 0.0 and r["oracle_depth_rmse"] >= r["oracle_depth_mae"] - 1e-15
    text = (tmp_path / "s.csv").read_text().splitlines()
    assert text[0].split(",")[-len(sweep.ORACLE_FIELDS):] == sweep.ORACLE_FIELDS
    plain = sweep.run_sweep(["Thin Torus"], ["Standard"], "budget", W, H, budgets=[16])
    assert set(plain[0]) == set(sweep.ROW_FIELDS)
