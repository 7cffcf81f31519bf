"""The exact first hit on a real MI355X: the kernels of csrc/rm_exact.hip against the g++ build of the same header
(tests/native/exact_check.cpp) bit for bit, exact_capture against interval_capture on the device, the trust gate
(oracle_validation) and the sweep's oracle columns.

Every program made here is destroyed by the fixture that made it, so the other suites see the catalogue scenes only."""
import numpy as np
import pytest

import exact_cases as ec

from raymarch_algo_compare_amd import _native, oracle_validation, registry, scoring, sweep
from raymarch_algo_compare_amd import exact_oracle as xo
from raymarch_algo_compare_amd import interval_oracle as io
from raymarch_algo_compare_amd import scene_program as sp
from raymarch_algo_compare_amd.camera import Camera
from raymarch_algo_compare_amd.viewpoints import viewpoints_for

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture
def programs(hip):
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


def same_frame(dev, host):
    assert np.array_equal(dev["hit"] > 0, host["hit"])
    assert np.array_equal(bits(dev["depth"]), bits(host["depth"]))
    assert np.array_equal(bits(dev["normal"]), bits(host["normal"]))
    assert np.array_equal(dev["leaf"], host["leaf"])


# ---- 1. the device equals the host build, bit for bit ------------------------------------------------------------------------

@pytest.mark.parametrize("sid", ec.EXACT_IDS)
def test_device_equals_host(hip, programs, sid):
    """depth, hit, normal and leaf of all eleven scenes (the twins of 11 and 15 as programs; Thin Torus at 128x96)"""
    W, H = ec.frame_size(sid)
    cam = ec.default_camera(W, H).params14()
    scene = programs(ec.expression(sid)) if sid in ec.TWIN_IDS else sid
    dev = _native.exact_render(scene, cam, W, H, _native.exact_config(t_max=ec.T_MAX))
    host = ec.host_frame(sid)
    assert host["hit"].any() and not host["hit"].all()
    same_frame(dev, host)


def test_device_equals_host_on_a_user_program(hip, programs):
    """box, cylinder, capsule, torus, subtract and onion over a sphere in one program; a band equals the same rows of the frame"""
    W, H = 64, 48
    cam = Camera((2.2, 1.6, 3.4), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 60.0, W, H).params14()
    pid = programs(ec.mixed_program())
    cfg = _native.exact_config(t_max=ec.T_MAX)
    dev = _native.exact_render(pid, cam, W, H, cfg)
    host = ec.host_render(ec.mixed_program(), cam, W, H)
    assert len(np.unique(host["leaf"][host["hit"]])) >= 5          # the frame sees most of the leaves
    same_frame(dev, host)
    band = _native.exact_render(pid, cam, W, H, cfg, row0=5, rows=7)
    for k in ("depth", "normal"):
        assert np.array_equal(bits(band[k]), bits(dev[k][5:12])), k
    assert np.array_equal(band["hit"], dev["hit"][5:12]) and np.array_equal(band["leaf"], dev["leaf"][5:12])


@pytest.mark.parametrize("sid", [14, 15])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_explicit_rays_equal_host(hip, programs, sid, n):
    """Sphere Cloud (24 leaves) and the Bumpy Sphere twin (31 leaves, the longest walk); directions not normalised"""
    rng = np.random.default_rng(1000 * sid + n)
    o = rng.normal(size=(n, 3)) * 0.3 + (0.0, 0.0, 6.0)
    d = (rng.normal(size=(n, 3)) * 0.25 + (0.0, 0.0, -1.0)) * rng.uniform(0.5, 2.0, size=(n, 1))
    scene = programs(ec.expression(sid)) if sid in ec.TWIN_IDS else sid
    t, nrm, leaf = _native.exact_march_rays(scene, o, d)
    ht, hn, hl = ec.host_march(ec.expression(sid), o, d)
    assert np.array_equal(bits(t), bits(ht)) and np.array_equal(bits(nrm), bits(hn)) and np.array_equal(leaf, hl)
    if n >= 63:
        assert np.isfinite(ht).any() and np.isinf(ht).any()
    t2, none, _ = _native.exact_march_rays(scene, o, d, want_normals=False)
    assert none is None and np.array_equal(bits(t2), bits(ht))


def test_hits_misses_and_inside_eyes_in_one_wave(hip):
    """64 rays on Hollow Cube: from outside (hits and misses), from inside the removed sphere and from inside the shell"""
    rng = np.random.default_rng(7)
    o = np.concatenate([np.tile((0.0, 0.0, 5.0), (24, 1)), np.zeros((20, 3)), np.tile((0.95, 0.95, 0.95), (20, 1))])
    d = np.concatenate([rng.normal(size=(24, 3)) * 0.25 + (0.0, 0.0, -1.0), rng.normal(size=(40, 3))])
    perm = rng.permutation(64)
    o, d = o[perm], d[perm]
    t, nrm, leaf = _native.exact_march_rays(6, o, d)
    ht, hn, hl = ec.host_march(ec.expression(6), o, d)
    assert np.isinf(ht).any() and np.isfinite(ht).any() and set(np.unique(hl)) == {-1, 0, 1}
    assert np.array_equal(bits(t), bits(ht)) and np.array_equal(bits(nrm), bits(hn)) and np.array_equal(leaf, hl)
    assert np.array_equal(bits(xo.first_hit(o, d, 6)), bits(ht))


# ---- 2. against the interval oracle on the device ------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["Hollow Cube (CSG)", "Onion Shell"])
def test_exact_capture_against_interval_capture(hip, name):
    """the four conditions of the host test (tests/test_exact_host.py), both captures from the device"""
    cam = ec.default_camera(64, 48)
    ex, iv = xo.exact_capture(name, cam), io.interval_capture(name, cam, bound_radius=-1.0)
    assert ex["hit"].dtype == bool and ex["depth"].dtype == np.float64 and ex["leaf"].dtype == np.int32
    assert ex["depth"].shape == (48, 64) and ex["normal"].shape == (48, 64, 3)
    assert not (ex["hit"] & ~iv["hit"]).any()
    only = iv["hit"] & ~ex["hit"]
    assert not (only & ~scoring.silhouette_band(ex["hit"], 2)).any()
    both = ex["hit"] & iv["hit"]
    te, ti = ex["depth"][both], iv["depth"][both]
    assert both.any() and (ti <= te + 1e-12 * (1.0 + te)).all()
    assert (te - ti).max() <= 4.0 * ec.INTERVAL_LAG_MEASURED
    assert xo.exact_capture("Metaballs", cam) is None


# ---- 3. the trust gate ----------------------------------------------------------------------------------------------------------

def test_oracle_validation_reports_the_three_tables(hip):
    rep = oracle_validation.validate(["Sphere", "Hollow Cube (CSG)", "Metaballs"], width=48, height=36)
    assert rep["resolution"] == [48, 36] and sorted(rep["scenes"]) == ["Hollow Cube (CSG)", "Sphere"]
    for name, s in rep["scenes"].items():
        assert sorted(s["comparisons"]) == sorted(oracle_validation.COMPARISONS)
        assert 0.0 < s["exact_hit_rate"] < 1.0 and 0.0 < s["interval_hit_rate"] < 1.0 and 0.0 < s["silhouette_band_frac"] < 1.0
        for table in s["comparisons"].values():
            assert np.isfinite(table["iou"]) and np.isfinite(table["core_iou"]) and 0.0 <= table["iou"] <= 1.0
        gate = s["comparisons"]["interval_vs_exact"]
        # soundness: no exact hit is missed and the interval depth is the earlier one (at this size the band may cover
        # every hit pixel, so core_iou says nothing)
        assert gate["false_miss"] == 0.0 and gate["depth_med"] <= 4.0 * ec.INTERVAL_LAG_MEASURED and gate["depth_signed"] < 0.0
    dev = oracle_validation.validate(["Sphere"], width=48, height=36, device_score=True)["scenes"]["Sphere"]["comparisons"]
    host = rep["scenes"]["Sphere"]["comparisons"]
    for k in ("interval_vs_exact", "dense_vs_exact"):
        assert dev[k]["iou"] == host[k]["iou"] and dev[k]["n_co_hit"] == host[k]["n_co_hit"]
        assert dev[k]["depth_med"] == pytest.approx(host[k]["depth_med"], rel=1e-6)


# ---- 4. the sweep's oracle columns ------------------------------------------------------------------------------------------------

def test_sweep_fills_the_oracle_columns_from_the_exact_capture(hip):
    W = H = 48
    rows = sweep.run_sweep(["Sphere"], ["Standard"], "budget", W, H, budgets=[64], oracle="exact")
    scene = registry.get_scene_by_name("Sphere")
    assert len(rows) == len(viewpoints_for(scene)) == 2
    for r in rows:
        vp = next(v for v in viewpoints_for(scene) if v.name == r["viewpoint"])
        cam = Camera(vp.position, vp.target, vp.up, 60.0, W, H)
        out = _native.render(_native.make_desc(scene.id, registry.get_strategy_by_name("Standard").id, cam.params14(), W, H,
                                               max_iterations=r["max_iterations"], hit_threshold=r["hit_threshold"]))
        s = scoring.score_capture({"hit": out["hit"] > 0, "depth": out["depth"], "normal": np.zeros((H, W, 3))},
                                  xo.exact_capture(scene, cam), compute_ssim=False)
        assert r["oracle_iou"] == pytest.approx(s["hit"]["iou"]) and r["oracle_depth_mae"] == pytest.approx(s["depth"]["mae"])
        assert all(r[k] is not None for k in sweep.ORACLE_FIELDS) and r["oracle_iou"] > 0.9
    none = sweep.run_sweep(["Metaballs"], ["Standard"], "budget", W, H, budgets=[64], oracle="exact")
    assert none and all(r[k] is None for r in none for k in sweep.ORACLE_FIELDS)


def test_sweep_exact_oracle_composes_with_twins_ssim_device_score_and_ceiling(hip):
    """Bumpy Sphere has an exact form through its program twin only; the ceiling stays scored against the interval
    oracle"""
    W = H = 48
    kw = dict(mode="budget", width=W, height=H, budgets=[64], oracle="exact")
    plain = sweep.run_sweep(["Bumpy Sphere"], ["Standard"], **kw)
    assert plain and all(r[k] is None for r in plain for k in sweep.ORACLE_FIELDS)
    try:
        rows = sweep.run_sweep(["Bumpy Sphere"], ["Standard"], oracle_twins=True, ssim=True, device_score=True,
                               ceiling="segment", **kw)
        host = sweep.run_sweep(["Bumpy Sphere"], ["Standard"], oracle_twins=True, **kw)
    finally:
        if registry.find_program_scene(sp.twin_name("Bumpy Sphere")) is not None:
            sp.unregister_scene(sp.twin_name("Bumpy Sphere"))
    assert len(rows) == len(host) == len(plain)
    for r, h in zip(rows, host):
        assert all(r[k] is not None for k in sweep.ORACLE_FIELDS + sweep.CEILING_FIELDS)
        assert r["depth_ssim"] is not None and r["normal_ssim"] is not None
        assert r["oracle_iou"] == h["oracle_iou"] and r["oracle_depth_mae"] == pytest.approx(h["oracle_depth_mae"], rel=1e-9, nan_ok=True)
        assert r["oracle_iou"] > 0.9 and r["ceiling_iou"] > 0.9
