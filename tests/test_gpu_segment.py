"""The sound segment tracer on the MI355X: rm_segment_* against the reference's own results (tests/golden/segment_*.npz),
against the host build of csrc/rm_segment.h (tests/native/segment_check.cpp), never past a surface against the pointwise
SDF, the hit mask of the interval oracle, the lifecycle of program ids, and the sweep's ceiling columns.

Every launch is bounded by its budget (at most RM_SEGMENT_MAX_STEPS trips per ray).  Every program made here is destroyed
by the fixture that made it, so the other suites see the catalogue scenes only."""
import ctypes
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from test_interval_host import DEEP_PROGRAMS
from test_segment_host import (CATALOGUE_IDS, bits, check_frame, dsdf_cases, frame_cases, host_eval, host_march, host_render,
                               load_host_lib, random_segments, ray_cases, seg_cfg)

from raymarch_algo_compare_amd import _native, analytic, registry, scoring, sweep
from raymarch_algo_compare_amd import faithful_segment as fs
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


# ---- 7. the reference's fixtures, bit for bit ---------------------------------------------------------------------------

def test_render_matches_reference():
    n = 0
    for p, sid, W, H, cam, cfg, want_hit, want_t, want_iters in frame_cases():
        out = _native.segment_render(sid, cam, W, H, seg_cfg(cfg))
        check_frame(out["depth"].ravel(), out["hit"].ravel(), out["iters"].ravel(), out["cursor"].ravel(), want_hit, want_t,
                    want_iters, p)
        n += 1
    assert n == 8


def test_march_rays_matches_reference():
    n = 0
    for p, sid, o, d, cfg, want_t, want_iters in ray_cases():
        t, iters, _ = _native.segment_march_rays(sid, o, d, seg_cfg(cfg))
        assert np.array_equal(bits(t), want_t), (p, np.nonzero(bits(t) != want_t)[0][:8])
        assert np.array_equal(iters, want_iters), p
        n += 1
    assert n == 10


def test_sdf_eval_matches_reference():
    for sid, segs, want in dsdf_cases():
        got = bits(_native.segment_sdf_eval(sid, segs))
        assert np.array_equal(got, want), (sid, np.argwhere(got != want)[:8])
        r = fs.segment_sdf(sid, segs[:, 0:3], segs[:, 3:6], segs[:, 6], segs[:, 7])
        assert np.array_equal(bits(r["der_hi"]), want[:, 3])


# ---- 8. the device against the host build ------------------------------------------------------------------------------

def _trees(k=6):
    with open(os.path.join(GOLDEN, "programs_trees.json"), encoding="utf-8") as f:
        trees = json.load(f)["trees"]
    return [sp.expr_from_json(t) for t in trees[:k]] + [e for _, e in DEEP_PROGRAMS]


def _compare(host, sid_dev, expr, scene_bound, cam14, W, H, what):
    ops, n = sp.to_ctypes(expr)
    depth, hit, iters, cursor = host_render(host, ops, n, _native.segment_config(), scene_bound, cam14, W, H)
    out = _native.segment_render(sid_dev, cam14, W, H)
    assert np.array_equal(out["hit"].ravel(), hit), what
    assert np.array_equal(bits(out["depth"].ravel()), bits(depth)), what
    assert np.array_equal(out["iters"].ravel(), iters), what
    assert np.array_equal(bits(out["cursor"].ravel()), bits(cursor)), what


@pytest.mark.parametrize("sid", CATALOGUE_IDS)
def test_device_equals_host_catalogue(host, sid):
    ex = sp.catalogue_expressions()[sid]
    for vp in viewpoints_for(registry.SCENES[sid]):
        cam = Camera(vp.position, vp.target, vp.up, 60.0, 96, 72).params14()
        _compare(host, sid, ex, host.rms_scene_bound(sid), cam, 96, 72, (sid, vp.name))


def test_device_equals_host_programs(host, programs):
    for i, expr in enumerate(_trees()):
        pid = programs(expr)
        rng = np.random.default_rng(i)
        o = rng.uniform(-4, 4, size=(300, 3))
        d = -o + rng.normal(size=o.shape)                  # unnormalised directions included
        d[::2] /= np.linalg.norm(d[::2], axis=1, keepdims=True)
        ops, n = sp.to_ctypes(expr)
        t_h, i_h, c_h = host_march(host, ops, n, _native.segment_config(), o, d)
        t_d, i_d, c_d = _native.segment_march_rays(pid, o, d)
        assert np.array_equal(bits(t_d), bits(t_h)) and np.array_equal(i_d, i_h) and np.array_equal(bits(c_d), bits(c_h)), i
        segs = random_segments(rng, 2000)
        assert np.array_equal(bits(_native.segment_sdf_eval(pid, segs)), bits(host_eval(host, ops, n, segs))), i


def test_sdf_eval_equals_host(host):
    segs = random_segments(np.random.default_rng(5), 4000)
    segs[::9, 3:6] *= 2.5
    for sid in CATALOGUE_IDS:
        ops, n = sp.to_ctypes(sp.catalogue_expressions()[sid])
        dev = _native.segment_sdf_eval(sid, segs)
        assert np.array_equal(bits(dev), bits(host_eval(host, ops, n, segs))), sid


# ---- 9. never past a surface ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sid", CATALOGUE_IDS)
def test_never_past_a_surface(sid):
    """Every ray of the first viewpoint at 64 x 48: the pointwise SDF at 2048 evenly spaced points of [0, min(cursor, t_max))
    is >= -1e-12 (test_no_tunnelling's bound), and every hit has |f| < tol at t, f being the value the tracer itself reads
    (the interval program at the point).  Rays that used up the budget are counted and printed, not capped: their cursor
    passes the same check.  On the reference's four scenes there is none (true of the reference itself).
    On the host build of the same header (budget 4096) no ray of any of the 14 scenes uses up the budget; DESIGN.md
    section 3, "Segment ceiling"."""
    scene = registry.SCENES[sid]
    vp = viewpoints_for(scene)[0]
    cam = Camera(vp.position, vp.target, vp.up, 60.0, 64, 48)
    o, d = analytic.camera_rays(cam)
    d = d.reshape(-1, 3)
    o = np.broadcast_to(o, d.shape)
    t, iters, cursor = _native.segment_march_rays(sid, o, d)
    hit = np.isfinite(t)
    spent = ~hit & (iters >= 4096)
    print(f"{scene.name}: hits {int(hit.sum())} of {len(t)}, iters median {np.median(iters[hit]) if hit.any() else 0:.0f} "
          f"max {int(iters.max())}, rays that used up the budget {int(spent.sum())}")
    if sid < 4:
        assert int(spent.sum()) == 0, f"{scene.name}: {int(spent.sum())} rays used up the budget"
    assert np.array_equal(cursor[hit], t[hit])
    end = np.minimum(cursor, fs.DEFAULT_T_MAX)
    K = 2048
    s = np.arange(K) / K                                  # evenly spaced on [0, end)
    worst = np.inf
    for a in range(0, len(d), 256):
        b = min(a + 256, len(d))
        pts = o[a:b, None, :] + (end[a:b, None] * s[None, :])[..., None] * d[a:b, None, :]
        worst = min(worst, float(_native.sdf_eval(sid, pts.reshape(-1, 3)).min()))
    print(f"{scene.name}: least pointwise SDF before the cursor {worst:.3e}")
    assert worst >= -1e-12, f"{scene.name}: the SDF is {worst} before the tracer's cursor"
    P = o[hit] + t[hit][:, None] * d[hit]
    f, _ = io.interval_sdf(sid, P, P)
    assert np.all(np.abs(f) < fs.DEFAULT_TOL), (scene.name, float(np.abs(f).max()))


# ---- 10. against the interval oracle -------------------------------------------------------------------------------------

@pytest.mark.parametrize("sid", CATALOGUE_IDS)
def test_against_the_interval_oracle(sid):
    """Scenes 0-3 at the fixtures' cameras: the tracer's hit mask IS the oracle's (IoU exactly 1, as the reference's own
    tracer against its own oracle).  All 14: the hit rays' steps next to the oracle's are printed."""
    scene = registry.SCENES[sid]
    rc = scene.suggested_camera()
    pos, tgt = (rc.camera_position, rc.camera_target) if rc else ((0.0, 0.0, 5.0), (0.0, 0.0, 0.0))
    cam = Camera(pos, tgt, (0.0, 1.0, 0.0), 60.0, 96, 72)
    if sid < 4:
        want = [c for c in frame_cases() if c[0] == f"s{sid}_default_"][0]
        assert np.array_equal(cam.params14(), want[4]), "not the fixture's camera"
    cap = fs.faithful_capture(scene, cam)
    gold = io.interval_capture(scene, cam)
    res = scoring.residual(cap["hit"], cap["depth"], gold["hit"], gold["depth"], scoring.silhouette_band(gold["hit"], k=2))
    c = fs.cost(cap)
    both = cap["hit"] & gold["hit"]
    print(f"{scene.name}: IoU {res['iou']:.4f} core {res['core_iou']:.4f} depth med {res['depth_med']:.2e}; steps to a hit: "
          f"segment median {c['iters_median']:.0f} p95 {c['iters_p95']:.0f} max {c['iters_max']}, "
          f"oracle median {np.median(gold['steps'][both]) if both.any() else 0:.0f} max {int(gold['steps'][both].max()) if both.any() else 0}")
    assert cap["depth"].dtype == np.float64 and cap["hit"].dtype == bool and cap["iters"].dtype == np.int32
    assert cap["depth"].shape == cap["cursor"].shape == (72, 96)
    if sid < 4:
        assert res["iou"] == 1.0, (scene.name, res)


# ---- 11. rows, lifecycle, timing, the sweep ------------------------------------------------------------------------------

def test_rows_lifecycle_and_timing(programs):
    cam = Camera((2.0, 2.0, 4.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 60.0, 64, 48).params14()
    whole = _native.segment_render(6, cam, 64, 48)
    part = _native.segment_render(6, cam, 64, 48, row0=7, rows=11)
    for k in ("depth", "cursor"):
        assert np.array_equal(bits(part[k]), bits(whole[k][7:18])), k
    assert np.array_equal(part["hit"], whole["hit"][7:18]) and np.array_equal(part["iters"], whole["iters"][7:18])
    pid = programs(sp.op_subtract(sp.sd_box((1.0, 1.0, 1.0)), sp.sd_sphere(1.3)))       # Hollow Cube's program
    a = _native.segment_render(pid, cam, 64, 48, repeats=3, warmup=1)
    assert np.array_equal(a["hit"], whole["hit"]) and np.array_equal(bits(a["depth"]), bits(whole["depth"]))
    tm = a["timing"]
    assert tm["repeats"] == 3 and len(tm["ms_each"]) == 3 and all(x > 0 for x in tm["ms_each"])
    assert tm["ms_min"] <= tm["ms_median"] <= tm["ms_max"]
    _native.scene_program_destroy(pid)
    seg = np.array([[0, 0, 5, 0, 0, -1, 0.0, 1.0]])
    for call in (lambda: _native.segment_render(pid, cam, 64, 48), lambda: _native.segment_march_rays(pid, [[0, 0, 5]], [[0, 0, -1]]),
                 lambda: _native.segment_sdf_eval(pid, seg)):
        with pytest.raises(_native.RmError) as e:
            call()
        assert e.value.code == _native.RM_E_BAD_SCENE
    mandelbulb = registry.get_scene_by_name("Mandelbulb").id
    with pytest.raises(_native.RmError) as e:
        _native.segment_render(mandelbulb, cam, 64, 48)
    assert e.value.code == _native.RM_E_BAD_SCENE
    assert fs.faithful_capture("Mandelbulb", Camera((0, 0, 3), (0, 0, 0), (0, 1, 0), 60.0, 8, 8)) is None
    t, iters = fs.segment_trace([0.0, 0.0, 5.0], [[0.0, 0.0, -1.0]], "Sphere", t_max=10.0)
    assert abs(t[0] - 4.0) < 1e-4 and 1 <= iters[0] <= 8


def test_sweep_ceiling_columns(tmp_path):
    W = H = 48
    rows = sweep.run_sweep(["Thin Torus", "Menger"], ["Standard"], "budget", W, H, budgets=[16, 64], ceiling="segment",
                           out_path=str(tmp_path / "s.csv"))
    assert len(rows) > 0
    seen = 0
    for r in rows:
        assert set(r) == set(sweep.ROW_FIELDS + sweep.CEILING_FIELDS)
        scene = registry.get_scene_by_name(r["scene"])
        if scene.name.startswith("Menger"):
            assert all(r[k] is None for k in sweep.CEILING_FIELDS), r
            continue
        vp = next(v for v in viewpoints_for(scene) if v.name == r["viewpoint"])
        cam = Camera(vp.position, vp.target, vp.up, 60.0, W, H)
        cap, gold = fs.faithful_capture(scene, cam), io.interval_capture(scene, cam)
        res = scoring.residual(cap["hit"], cap["depth"], gold["hit"], gold["depth"], scoring.silhouette_band(gold["hit"], k=2))
        it = cap["iters"][cap["hit"]]
        want = {"ceiling_iou": res["iou"], "ceiling_depth_med": res["depth_med"],
                "ceiling_iters_median": float(np.median(it)) if it.size else 0.0,
                "ceiling_iters_p95": float(np.percentile(it, 95)) if it.size else 0.0}
        for k, v in want.items():
            assert r[k] == pytest.approx(v, nan_ok=True), (r["viewpoint"], k)
        seen += 1
    assert seen > 0
    text = (tmp_path / "s.csv").read_text().splitlines()
    assert text[0].split(",")[-len(sweep.CEILING_FIELDS):] == sweep.CEILING_FIELDS
    both = sweep.run_sweep(["Thin Torus"], ["Standard"], "budget", W, H, budgets=[16], oracle="interval", ceiling="segment")
    assert list(both[0]) == sweep.ROW_FIELDS + sweep.ORACLE_FIELDS + sweep.CEILING_FIELDS
    plain = sweep.run_sweep(["Thin Torus"], ["Standard"], "budget", W, H, budgets=[16])
    assert set(plain[0]) == set(sweep.ROW_FIELDS)
