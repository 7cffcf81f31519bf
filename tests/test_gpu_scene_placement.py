"""The placement ops of scene programs (op_rotate, op_turn, op_mirror) on the MI355X: the device against the host build
(tests/native/placement_check.cpp) bit for bit in all five evaluations, on the inputs of tests/test_scene_placement_host.py;
half-turned catalogue scenes against the catalogue's own frames; a rotated scene against the same scene seen by the
counter-rotated camera; no tunnelling of the interval oracle on the tilted scene; the sweep, capture and features paths.

Every program made here is destroyed by the fixture that made it."""
import numpy as np
import pytest

import placement_cases as pc
import program_ext_cases as xc
from placement_cases import bits

from raymarch_algo_compare_amd import _native, features, registry, scoring, sweep
from raymarch_algo_compare_amd import exact_oracle as xo
from raymarch_algo_compare_amd import scene_program as sp
from raymarch_algo_compare_amd.camera import Camera
from raymarch_algo_compare_amd.config import MarchConfig, RenderConfig
from raymarch_algo_compare_amd.runner import GPURunner, ray_directions

pytestmark = pytest.mark.gpu

PROGRAMS = pc.programs()
W, H = 48, 36


@pytest.fixture(scope="module")
def host():
    return pc.host()


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


def _same(a, b, what):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    bad = np.argwhere(bits(a) != bits(b))
    assert bad.size == 0, (what, len(bad), bad[:4], a[tuple(bad[0])], b[tuple(bad[0])])


# ---- 7. the device equals the host build ----------------------------------------------------------------------------

@pytest.mark.parametrize("idx", range(len(pc.NAMES)), ids=pc.NAMES)
def test_device_equals_host_in_the_four_walks(host, programs, idx):
    name = pc.NAMES[idx]
    expr = PROGRAMS[name]
    pid = programs(expr)
    pts = pc.points()
    want = host.point(expr, pts)
    _same(_native.sdf_eval(pid, pts), want, (name, "rm_sdf_eval"))
    for n in pc.LANE_COUNTS:                                       # one lane, a wave less one, a wave, a wave and one
        _same(_native.sdf_eval(pid, pts[100:100 + n]), want[100:100 + n], (name, "rm_sdf_eval", n))
    lo, hi = xc.boxes(600 + idx, pc.OFF)
    dlo, dhi = _native.interval_sdf_eval(pid, lo, hi)
    iv = host.interval(expr, lo, hi)
    _same(np.stack([dlo, dhi], axis=1), iv, (name, "rm_interval_sdf_eval"))
    for n in pc.LANE_COUNTS:
        dlo, dhi = _native.interval_sdf_eval(pid, lo[490:490 + n], hi[490:490 + n])       # degenerate boxes, then wide ones
        _same(np.stack([dlo, dhi], axis=1), iv[490:490 + n], (name, "rm_interval_sdf_eval", n))
    segs = xc.segments(800 + idx)
    dual, box = host.dual(expr, segs)
    dev = _native.segment_sdf_eval(pid, segs)
    _same(dev, dual, (name, "rm_segment_sdf_eval"))
    _same(dev[:, :2], box, (name, "rm_segment_sdf_eval val against the interval range"))
    for n in pc.LANE_COUNTS:
        _same(_native.segment_sdf_eval(pid, segs[:n]), dual[:n], (name, "rm_segment_sdf_eval", n))
    for mode in (_native.RM_RANGE_AFFINE, _native.RM_RANGE_MEET):
        rng, _ = _native.affine_range_eval(pid, segs, mode, want_form=False)
        want_rng = host.affine(expr, mode, segs)
        _same(rng, want_rng, (name, "rm_affine_range_eval", mode))
        for n in pc.LANE_COUNTS:
            _same(_native.affine_range_eval(pid, segs[:n], mode, want_form=False)[0], want_rng[:n], (name, "rm_affine_range_eval", mode, n))


@pytest.mark.parametrize("name", [n for n in pc.NAMES if "mirror" not in n])        # (the exact caster refuses a mirror)
def test_device_equals_host_in_the_exact_caster(host, programs, name):
    expr = PROGRAMS[name]
    pid = programs(expr)
    o, d = pc.exact_rays()
    t, nrm, leaf = host.exact_march(expr, o, d)
    dt, dn, dl = _native.exact_march_rays(pid, o, d)
    _same(dt, t, (name, "rm_exact_march_rays t"))
    _same(dn, nrm, (name, "rm_exact_march_rays normal"))
    assert np.array_equal(dl, leaf), name
    assert np.isfinite(t).any() and not np.isfinite(t).all()
    for n in pc.LANE_COUNTS:
        _same(_native.exact_march_rays(pid, o[:n], d[:n])[0], t[:n], (name, "rm_exact_march_rays", n))
    cam = pc.default_camera().params14()
    frame = host.exact_render(expr, cam, 64, 48)
    out = _native.exact_render(pid, cam, 64, 48, _native.exact_config(t_max=100.0))
    assert np.array_equal(out["hit"] > 0, frame["hit"]) and np.array_equal(out["leaf"], frame["leaf"]), name
    _same(out["depth"], frame["depth"], (name, "rm_exact_render depth"))
    _same(out["normal"], frame["normal"], (name, "rm_exact_render normal"))


def test_the_mirror_is_refused_by_the_exact_caster_only(programs):
    pid = programs(PROGRAMS["mirror"])
    assert not _native.exact_supported(pid) and "mirror folds the ray" in _native.exact_refusal(pid)
    assert _native.interval_supported(pid) and _native.segment_supported(pid) and _native.affine_supported(pid)


# ---- 8. frames anchored in the reference: a half turn about z that neither SDF can see -----------------------------------

@pytest.mark.parametrize("sid", [4, 3], ids=["Cylinder", "Thin Torus"])
def test_half_turned_catalogue_scene_gives_the_catalogue_frames(programs, sid):
    scene = registry.SCENES[sid]
    W, H = 64, 48                                          # (at 48 x 36 no pixel centre meets the thin torus)
    pid = programs(sp.op_turn((0, 0, 2), sp.catalogue_expressions()[sid]), scene.lipschitz)
    cam = Camera(scene.camera_position or (0.0, 0.0, 5.0), scene.camera_target or (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 60.0,
                 W, H).params14()
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
        assert 0 < int(want["hit"].sum()) < W * H, (scene.name, key)


# ---- 9. conjugation: rotating the scene is counter-rotating the camera ------------------------------------------------------

def test_a_rotated_scene_is_the_scene_seen_by_the_counter_rotated_camera(programs):
    """exact captures, 64 x 48: the tilted scene under one more rotation by the default camera, and the tilted scene itself by
    the camera whose position, target and up went through the op's point transform (the inverse of the solid's rotation)"""
    consts = pc.rot_consts(pc.A5)
    turned = programs(sp.op_rotate(pc.A5, pc.tilted()))
    plain = programs(pc.tilted())
    cam = pc.default_camera()
    moved = pc.conjugate_camera(pc.A5)
    a = _native.exact_render(turned, cam.params14(), 64, 48, _native.exact_config(t_max=100.0))
    b = _native.exact_render(plain, moved.params14(), 64, 48, _native.exact_config(t_max=100.0))
    ha, hb = a["hit"] > 0, b["hit"] > 0
    assert 0.05 <= ha.mean() <= 0.95
    assert not ((ha ^ hb) & ~scoring.silhouette_band(ha, 2)).any()
    both = ha & hb
    ta, tb = a["depth"][both], b["depth"][both]
    assert both.any() and np.all(np.abs(ta - tb) <= 1e-9 * (1.0 + ta))
    core = ~scoring.silhouette_band(ha, 2)[both]                  # (normals jump at edges: compared away from them)
    na = pc.np_rotate(a["normal"][both][core], consts)            # world normals of the turned scene, in the tilted scene's frame
    assert np.abs(na - b["normal"][both][core]).max() <= 1e-6


# ---- 10. the interval oracle does not tunnel ---------------------------------------------------------------------------------

def test_oracle_of_the_tilted_scene_is_sound_against_the_point_samples(programs):
    """2048 equally spaced samples of every ray in [0, min(t_hit, t_max)): each is > 0"""
    pid = programs(pc.tilted())
    cam = pc.default_camera(W, H)
    cam14 = cam.params14()
    t_max = 100.0
    out = _native.interval_render(pid, cam14, W, H, want_normal=False)
    hit = out["hit"].astype(bool).ravel()
    rate = float(hit.mean())
    assert 0.05 <= rate <= 0.95, rate
    rd = np.asarray(ray_directions(cam), dtype=np.float64).reshape(-1, 3)
    ro = np.asarray(cam14[:3], dtype=np.float64)
    end = np.where(hit, np.minimum(out["depth"].ravel(), t_max), t_max)
    t = end[:, None] * (np.arange(2048) / 2048.0)[None, :]
    f = _native.sdf_eval(pid, (ro[None, None, :] + t[..., None] * rd[:, None, :]).reshape(-1, 3)).reshape(t.shape)
    bad = np.argwhere(~(f > 0.0))
    assert bad.size == 0, (len(bad), bad[:4], f[tuple(bad[0])], t[tuple(bad[0])])


def test_exact_against_interval_on_the_tilted_scene_on_the_device(programs):
    pid = programs(pc.tilted())
    cam = pc.default_camera().params14()
    ex = _native.exact_render(pid, cam, 64, 48, _native.exact_config(t_max=100.0))
    iv = _native.interval_render(pid, cam, 64, 48, _native.interval_config(bound_radius=-1.0), want_normal=False)
    eh, ih = ex["hit"] > 0, iv["hit"] > 0
    assert not (eh & ~ih).any()
    assert not ((ih & ~eh) & ~scoring.silhouette_band(eh, 2)).any()
    both = eh & ih
    te, ti = ex["depth"][both], iv["depth"][both]
    assert both.any() and (ti <= te + 1e-12 * (1.0 + te)).all()
    assert (te - ti).max() <= 4.0 * pc.TILTED_LAG_MEASURED


def test_device_renders_count_the_host_builds_steps(host, programs):
    """rm_interval_render and rm_affine_render (both modes) of the tilted scene and of the tilted scene under one more
    rotation, 48 x 36: hit, depth and steps are the host build's, so the evaluation counts of DESIGN.md section 3, "Placement
    ops", taken from the host build, are the device's."""
    cam = pc.default_camera(W, H).params14()
    for label, expr in (("tilted", pc.tilted()), ("tilted, rotated", sp.op_rotate(pc.A5, pc.tilted()))):
        pid = programs(expr)
        cfg = _native.interval_config(t_max=100.0, tol=1e-5, bound_radius=-1.0)
        dev, ref = _native.interval_render(pid, cam, W, H, cfg, want_normal=False), host.interval_render(expr, cam, W, H)
        assert np.array_equal(dev["hit"] > 0, ref["hit"]) and np.array_equal(dev["steps"], ref["steps"]), label
        _same(dev["depth"], ref["depth"], (label, "rm_interval_render depth"))
        for mode in (_native.RM_RANGE_AFFINE, _native.RM_RANGE_MEET):
            dev, ref = _native.affine_render(pid, cam, W, H, mode, cfg), host.affine_render(expr, mode, cam, W, H)
            assert np.array_equal(dev["hit"] > 0, ref["hit"]) and np.array_equal(dev["steps"], ref["steps"]), (label, mode)
            _same(dev["depth"], ref["depth"], (label, mode, "rm_affine_render depth"))


# ---- 11. whole-library paths ----------------------------------------------------------------------------------------------

def test_sweep_capture_and_features_accept_a_registered_tilted_scene(hip):
    name = "Tilted Block (placement test)"
    info = sp.register_scene(name, pc.tilted(), camera_position=(0.0, 0.0, 5.0))
    try:
        assert xo.has_exact(name) and xo.why_not(name) is None
        rows = sweep.run_sweep([name], ["Standard"], "budget", W, H, budgets=[64], oracle="exact", ceiling="segment")
        assert rows and all(r["scene"] == name for r in rows)
        for r in rows:
            for k in sweep.ORACLE_FIELDS + sweep.CEILING_FIELDS:
                assert r[k] is not None and np.isfinite(r[k]), (k, r[k])
        rc = RenderConfig(width=W, height=H, camera_position=(0.0, 0.0, 5.0), camera_target=(0.0, 0.0, 0.0))
        cap = GPURunner().capture(info.id, 0, rc, MarchConfig(), device=True)
        assert 0.05 <= cap["hit"].mean() <= 0.95 and np.isfinite(cap["normal"]).all()
        rng = np.random.default_rng(0)
        sets = [features.sample_sets((-2.0, -2.0, -2.0), (2.0, 2.0, 2.0), rng, n_lip=256, n_chords=16, chord_steps=32)]
        feat = features.intrinsic_features_device(info.id, sets)[0]
        assert feat and all(np.isfinite(v) for v in feat.values() if isinstance(v, float))
    finally:
        sp.unregister_scene(name)
