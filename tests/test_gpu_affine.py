"""The affine range on the MI355X: rm_affine_* against the reference's own results (tests/golden/affine_*.npz) and against
the host build of csrc/rm_affine.h (tests/native/affine_check.cpp), bit for bit in both modes; partial waves, row shards,
and the report of affine_range.evaluate.

Every launch is bounded by max_steps (at most RM_INTERVAL_MAX_STEPS steps per ray).  Every program made here is destroyed by
the fixture that made it, so the other suites see the catalogue scenes only."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from test_affine_host import (AFFINE, MEET, check_frame, form_cases, frame_cases, host_march, host_range, host_render, iv_cfg,
                              load_host_lib, ray_cases)
from test_segment_host import CATALOGUE_IDS, bits, random_segments

from raymarch_algo_compare_amd import _native, registry
from raymarch_algo_compare_amd import affine_range as ar
from raymarch_algo_compare_amd import interval_oracle as io
from raymarch_algo_compare_amd import scene_program as sp
from raymarch_algo_compare_amd.camera import Camera

pytestmark = pytest.mark.gpu
MODES = [AFFINE, MEET]
MODE_IDS = ["affine", "meet"]


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


# ---- the reference's fixtures, bit for bit --------------------------------------------------------------------------------

def test_range_eval_matches_reference():
    n = 0
    for sid, segs, want in form_cases():
        rng, form = _native.affine_range_eval(sid, segs)
        got = bits(np.concatenate([form, rng], axis=1))
        assert np.array_equal(got, want), (sid, np.argwhere(got != want)[:8])
        f = ar.affine_form(sid, segs[:, 0:3], segs[:, 3:6], segs[:, 6], segs[:, 7])
        assert np.array_equal(bits(f["e"]), want[:, 2]) and np.array_equal(bits(f["hi"]), want[:, 4])
        n += 1
    assert n == 4


def test_render_matches_reference():
    n = 0
    for p, sid, W, H, cam, cfg, want_hit, want_t, want_steps, score in frame_cases():
        out = _native.affine_render(sid, cam, W, H, AFFINE, iv_cfg(cfg))
        check_frame(out["depth"].ravel(), out["hit"].ravel(), out["steps"].ravel(), want_hit, want_t, want_steps, p)
        n += 1
    assert n == 8


def test_march_rays_matches_reference():
    n = 0
    for p, sid, o, d, cfg, want_t, want_steps in ray_cases():
        t, steps = _native.affine_march_rays(sid, o, d, AFFINE, iv_cfg(cfg))
        assert np.array_equal(bits(t), want_t), (p, np.nonzero(bits(t) != want_t)[0][:8])
        assert np.array_equal(steps, want_steps), p
        n += 1
    assert n == 10


# ---- the device against the host build ------------------------------------------------------------------------------------

def _fixture_camera(sid, W, H):
    """the camera the fixtures use: the scene's suggested one, else the default"""
    rc = registry.SCENES[sid].suggested_camera()
    pos, tgt = (rc.camera_position, rc.camera_target) if rc else ((0.0, 0.0, 5.0), (0.0, 0.0, 0.0))
    return Camera(pos, tgt, (0.0, 1.0, 0.0), 60.0, W, H).params14()


@pytest.mark.parametrize("sid", CATALOGUE_IDS)
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_device_equals_host_catalogue(host, mode, sid):
    W, H = 96, 72                                          # the fixtures' frame
    cam = _fixture_camera(sid, W, H)
    ops, n = sp.to_ctypes(sp.catalogue_expressions()[sid])
    depth, hit, steps = host_render(host, ops, n, mode, None, host.rma_scene_bound(sid), cam, W, H)
    out = _native.affine_render(sid, cam, W, H, mode)
    assert np.array_equal(out["hit"].ravel(), hit), sid
    assert np.array_equal(bits(out["depth"].ravel()), bits(depth)), sid
    assert np.array_equal(out["steps"].ravel(), steps), sid
    segs = random_segments(np.random.default_rng(sid), 1000)
    segs[::9, 3:6] *= 2.5
    want_rng, want_form = host_range(host, ops, n, mode, segs, want_form=mode == AFFINE)
    rng, form = _native.affine_range_eval(sid, segs, mode)
    assert np.array_equal(bits(rng), bits(want_rng)), sid
    assert (form is None and want_form is None) or np.array_equal(bits(form), bits(want_form)), sid


def _trees(k=6):
    with open(os.path.join(GOLDEN, "programs_trees.json"), encoding="utf-8") as f:
        trees = json.load(f)["trees"]
    return [sp.expr_from_json(t) for t in trees[:k]]


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_device_equals_host_programs(host, programs, mode):
    trees = _trees()
    assert len(trees) == 6
    for i, expr in enumerate(trees):
        pid = programs(expr)
        rng = np.random.default_rng(i)
        o = rng.uniform(-4, 4, size=(300, 3))
        d = -o + rng.normal(size=o.shape)                  # unnormalised directions included
        d[::2] /= np.linalg.norm(d[::2], axis=1, keepdims=True)
        ops, n = sp.to_ctypes(expr)
        cfg = _native.interval_config(t_max=20.0, max_steps=2000)
        t_h, s_h = host_march(host, ops, n, mode, cfg, o, d)
        t_d, s_d = _native.affine_march_rays(pid, o, d, mode, cfg)
        assert np.array_equal(bits(t_d), bits(t_h)) and np.array_equal(s_d, s_h), i
        segs = random_segments(rng, 1000)
        got, _ = _native.affine_range_eval(pid, segs, mode, want_form=False)
        assert np.array_equal(bits(got), bits(host_range(host, ops, n, mode, segs, want_form=False)[0])), i


@pytest.mark.parametrize("n", [1, 65])
def test_march_rays_small_counts(host, n):
    """one ray, and one more than a wave"""
    rng = np.random.default_rng(n)
    o = rng.normal(size=(n, 3))
    o = o / np.linalg.norm(o, axis=1, keepdims=True) * 4.0
    d = -o + rng.normal(scale=0.3, size=o.shape)
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    ops, nops = sp.to_ctypes(sp.catalogue_expressions()[3])
    for mode in MODES:
        t_h, s_h = host_march(host, ops, nops, mode, None, o, d)
        t_d, s_d = _native.affine_march_rays(3, o, d, mode)
        assert t_d.shape == (n,) and np.array_equal(bits(t_d), bits(t_h)) and np.array_equal(s_d, s_h), mode
    assert _native.affine_march_rays(3, np.empty((0, 3)), np.empty((0, 3)))[0].shape == (0,)


def test_row_shard_of_a_narrow_frame():
    """50 x 7, rows 2..5: a width that is no multiple of the wave, a non-zero row0"""
    cam = Camera((2.0, 2.0, 4.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 60.0, 50, 7).params14()
    for mode in MODES:
        for sid in (2, 6):
            whole = _native.affine_render(sid, cam, 50, 7, mode)
            part = _native.affine_render(sid, cam, 50, 7, mode, row0=2, rows=3)
            assert part["depth"].shape == (3, 50)
            assert np.array_equal(bits(part["depth"]), bits(whole["depth"][2:5])), (mode, sid)
            assert np.array_equal(part["hit"], whole["hit"][2:5]) and np.array_equal(part["steps"], whole["steps"][2:5]), (mode, sid)
            assert whole["hit"].any()


def test_evaluate_report():
    rep = ar.evaluate(["Sphere", "Cube", "Mandelbulb"], 48, 36)
    assert rep["resolution"] == [48, 36] and list(rep["scenes"]) == ["Sphere", "Cube"]
    for name, e in rep["scenes"].items():
        assert list(e) == ["affine", "interval", "meet", "eval_speedup_aa_over_ia", "eval_speedup_meet_over_ia"]
        for key in ("affine", "interval", "meet"):
            assert list(e[key]) == ["iou", "core_iou", "evals"]
        for key, mode in (("affine", "affine"), ("meet", "meet")):
            cap = ar.capture(name, 48, 36, mode)
            assert cap["depth"].shape == (36, 48) and cap["hit"].dtype == bool and cap["steps"].dtype == np.int32
            assert e[key]["evals"] == cap["evals"] == int(cap["steps"].sum())
        gold = io.interval_capture(name, ar._render_config(registry.get_scene_by_name(name), 48, 36))
        assert e["interval"]["evals"] == int(gold["steps"].sum()) and e["interval"]["iou"] == 1.0
        assert e["eval_speedup_aa_over_ia"] == e["interval"]["evals"] / e["affine"]["evals"]
        assert e["eval_speedup_meet_over_ia"] == e["interval"]["evals"] / e["meet"]["evals"]
    assert ar.capture("Mandelbulb", 8, 8) is None
