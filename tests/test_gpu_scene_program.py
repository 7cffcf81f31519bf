"""Scene programs on the MI355X: the interpreter's kernels against the reference's own values (tests/golden/programs_*,
tools/gen_program_golden.py) and against the built-in scenes they restate, through every frame entry point.

Registration is process-wide: every program made here is destroyed (every registered scene unregistered) by the
fixture that made it, so the other suites see the 20 catalogue scenes whatever the order."""
import ctypes
import importlib.util
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, sha_f64

from raymarch_algo_compare_amd import _native, registry
from raymarch_algo_compare_amd import scene_program as sp
from raymarch_algo_compare_amd.camera import Camera

pytestmark = pytest.mark.gpu

ALL_KERNELS = range(_native.RM_NUM_STRATEGY_KERNELS)


def _trees():
    with open(os.path.join(GOLDEN, "programs_trees.json"), encoding="utf-8") as f:
        return json.load(f)


def _fixture_points():
    """tools/program_fixture_points.py: the fixture stores results only, the points are rebuilt here"""
    spec = importlib.util.spec_from_file_location("program_fixture_points",
                                                  os.path.join(ROOT, "tools", "program_fixture_points.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def sdf_fixture():
    """[(tree, points, sha256 of all results, bits of the first results)] of tests/golden/programs_sdf.npz"""
    fp = _fixture_points()
    z = np.load(os.path.join(GOLDEN, "programs_sdf.npz"))
    n = int(z["npoints"][0])
    out = []
    for i, t in enumerate(_trees()["trees"]):
        pts = fp.fixture_points(i, n)
        assert fp.sha256_f64(pts) == z[f"t{i}_pts_sha"].tobytes(), f"the fixture points of tree {i} have drifted"
        out.append((t, pts, z[f"t{i}_sha"].tobytes(), z[f"t{i}_bits"]))
    return out, fp.sha256_f64


def _create(expr, lipschitz=1.0):
    arr, n = sp.to_ctypes(expr)
    return _native.scene_program_create(arr, n, lipschitz)


@pytest.fixture(scope="module")
def tree_programs(hip):
    ids = [_create(sp.expr_from_json(t)) for t in _trees()["trees"]]
    yield ids
    for i in ids:
        _native.scene_program_destroy(i)


@pytest.fixture(scope="module")
def catalogue_programs(hip):
    ids = {sid: _create(e, registry.SCENES[sid].lipschitz or 1.0) for sid, e in sp.catalogue_expressions().items()}
    yield ids
    for i in ids.values():
        _native.scene_program_destroy(i)


def _cam(sid, W, H):
    s = registry.SCENES[sid]
    return Camera(s.camera_position or (0.0, 0.0, 5.0), s.camera_target or (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 60.0,
                  W, H).params14()


def _frame(hip, scene_id, kid, cam, W, H, lipschitz, **kw):
    desc = hip.make_desc(scene_id, kid, cam, W, H, 0, None, 512, 1e-4, 100.0, lipschitz, True, **kw)
    return hip.render(desc, want_t_raw=True, want_final_sdf=True, want_evals=True)


def _same(a, b, what):
    for k in ("iters", "hit", "depth", "evals"):
        assert np.array_equal(a[k], b[k]), (what, k)
    for k in ("t_raw", "final_sdf"):
        assert np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)), (what, k)
    for k, v in a["stats"].items():
        assert np.array_equal(v, b["stats"][k]), (what, "stats", k)


def test_sdf_eval_matches_reference_bits(hip, tree_programs):
    cases, sha = sdf_fixture()
    for i, ((_, xyz, want_sha, want_bits), sid) in enumerate(zip(cases, tree_programs)):
        out = hip.sdf_eval(sid, xyz)
        bad = int((out[:len(want_bits)].view(np.uint64) != want_bits).sum())
        assert bad == 0, (i, bad)
        assert sha(out) == want_sha, (i, "a result beyond the stored bits differs")


def test_deep_program_is_the_fold_of_its_primitives(hip):
    """value slots 6-7 and point slot 3 (test_interval_host.py: DEEP): a union selects exactly, so the program's value is
    the py_min fold of its eight primitives under the same transforms, bit for bit; FUSED likewise from its two halves"""
    from test_interval_host import DEEP, DEEP_PRIMS, FUSED, deep_wrap, fold_min
    pts = np.random.default_rng(77).uniform(-6.0, 6.0, size=(3000, 3))
    ids = [_create(deep_wrap(prim)) for prim in DEEP_PRIMS] + [_create(DEEP), _create(FUSED)]
    try:
        vals = [hip.sdf_eval(i, pts) for i in ids]
    finally:
        for i in ids:
            _native.scene_program_destroy(i)
    assert np.array_equal(vals[8].view(np.uint64), fold_min(vals[:8]).view(np.uint64))
    torus, box = _create(sp.op_translate((0.4, -0.3, 0.2), sp.sd_torus(0.8, 0.2))), _create(sp.sd_box((0.3, 0.5, 0.2)))
    try:
        a, b = hip.sdf_eval(torus, pts), hip.sdf_eval(box, pts)
    finally:
        _native.scene_program_destroy(torus)
        _native.scene_program_destroy(box)
    assert np.array_equal(vals[9].view(np.uint64), np.where(b < a, b, a).view(np.uint64))


def test_frames_match_reference_all_strategies(hip, tree_programs):
    doc = _trees()
    z = np.load(os.path.join(GOLDEN, "programs_frames.npz"))
    W, H = doc["W"], doc["H"]
    for i in doc["frame_trees"]:
        for kid in range(_native.RM_NUM_STRATEGIES):
            p = f"s{i}_k{kid}_"
            meta = z[p + "meta"]
            desc = hip.make_desc(tree_programs[i], kid, z[p + "cam"], W, H, 0, H, int(meta[4]), float(meta[5]),
                                 float(meta[6]), float(meta[7]), True)
            out = hip.render(desc, want_t_raw=True, want_final_sdf=True)
            hit = np.unpackbits(z[p + "hitbits"])[:W * H].reshape(H, W)
            assert np.array_equal(out["iters"], z[p + "iters"].astype(np.int32)), (i, kid, "iters")
            assert np.array_equal(out["hit"], hit), (i, kid, "hit")
            assert sha_f64(out["t_raw"]) == z[p + "sha_t"].tobytes(), (i, kid, "t")
            assert sha_f64(out["final_sdf"]) == z[p + "sha_fs"].tobytes(), (i, kid, "final_sdf")


def test_restated_catalogue_scenes_equal_builtins(hip, catalogue_programs):
    W, H = 64, 48
    for sid, pid in catalogue_programs.items():
        lip = registry.SCENES[sid].lipschitz or 1.0
        for kid in ALL_KERNELS:
            cam = _cam(sid, W, H)
            _same(_frame(hip, pid, kid, cam, W, H, lip), _frame(hip, sid, kid, cam, W, H, lip), (sid, kid))
        cam = _cam(sid, 1920, 1080)
        _same(_frame(hip, pid, 0, cam, 1920, 1080, lip), _frame(hip, sid, 0, cam, 1920, 1080, lip), (sid, "1080p"))


def test_parked_rays_and_sdf_eval_equal_builtins(hip, catalogue_programs):
    """Explicit long-ray suspension (resume kernels), row shards and rm_sdf_eval of the restated scenes."""
    z = np.load(os.path.join(GOLDEN, "sdf_points.npz"))
    for sid, pid in catalogue_programs.items():
        assert np.array_equal(hip.sdf_eval(pid, z["pts"]).view(np.uint64), z[f"s{sid}"].view(np.uint64)), sid
    for sid in (1, 12, 13):
        pid, cam = catalogue_programs[sid], _cam(sid, 320, 240)
        for kw in ({"suspend_after": (16, 64)}, {"suspend_after": (8, 0)}):
            _same(_frame(hip, pid, 4, cam, 320, 240, 1.0, **kw), _frame(hip, sid, 4, cam, 320, 240, 1.0, **kw), (sid, kw))
        a = hip.render(hip.make_desc(pid, 0, cam, 320, 240, 40, 64, full=True), want_t_raw=True)
        b = hip.render(hip.make_desc(sid, 0, cam, 320, 240, 40, 64, full=True), want_t_raw=True)
        assert np.array_equal(a["iters"], b["iters"]) and np.array_equal(a["t_raw"].view(np.uint64), b["t_raw"].view(np.uint64))


def test_batch_with_program_equals_single_frames(hip, catalogue_programs):
    pid, W, H = catalogue_programs[7], 64, 48
    cams = np.stack([Camera((x, 0.5, 5.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 60.0, W, H).params14() for x in (-2.0, 0.0, 1.5)])
    for kid in (0, 10):
        shape = hip.make_desc(pid, kid, cams[0], W, H)
        b = hip.render_batch(shape, cams, want_evals=True)
        for f in range(len(cams)):
            one = hip.render(hip.make_desc(pid, kid, cams[f], W, H), want_evals=True)
            for k in ("iters", "hit", "depth"):
                assert np.array_equal(b[k][f], one[k]), (kid, f, k)
            assert b["stats"][f]["sum_iters"] == one["stats"]["sum_iters"]


def test_two_programs_on_two_streams(hip):
    """Two programs rendered alternately on two streams: each equals its single-stream frame."""
    W, H = 128, 96
    exprs = [sp.op_smooth_union(sp.sd_box((1, 1, 1)), sp.op_translate((1.5, 0, 0), sp.sd_sphere(0.7)), 0.3),
             sp.op_subtract(sp.op_repeat((1.7, 0.0, 1.7), sp.sd_capsule((0, -1, 0), (0, 1, 0), 0.3)), sp.sd_sphere(2.0))]
    ids = [_create(e) for e in exprs]
    L = hip.load()
    streams = []
    try:
        cam = Camera((0.5, 1.0, 6.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 60.0, W, H).params14()
        ref = [hip.render(hip.make_desc(i, 0, cam, W, H)) for i in ids]
        for _ in range(2):
            s = ctypes.c_void_p()
            hip.check(L.rm_stream_create(ctypes.byref(s)))
            streams.append(s)
        bufs = []
        for rep in range(3):
            for j, pid in enumerate(ids):
                dd, di, dh = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
                hip.check(L.rm_alloc_frame(W, H, ctypes.byref(dd), ctypes.byref(di), ctypes.byref(dh)))
                bufs.append((j, dd, di, dh))
                d = hip.make_desc(pid, 0, cam, W, H)
                hip.check(L.rm_render_device(ctypes.byref(d), dd, di, dh, None, streams[j]))
        for s in streams:
            hip.check(L.rm_stream_synchronize(s))
        for j, dd, di, dh in bufs:
            it = np.empty((H, W), np.int32)
            dep = np.empty((H, W), np.float32)
            h = np.empty((H, W), np.uint8)
            hip.check(L.rm_copy_frame_to_host(W, H, dd, di, dh, dep.ctypes.data, it.ctypes.data, h.ctypes.data))
            hip.check(L.rm_free_frame(dd, di, dh))
            assert np.array_equal(it, ref[j]["iters"]) and np.array_equal(h, ref[j]["hit"]) and np.array_equal(dep, ref[j]["depth"])
    finally:
        for s in streams:
            L.rm_stream_destroy(s)
        for i in ids:
            _native.scene_program_destroy(i)


def test_team_form_and_destroyed_programs_are_refused(hip):
    pid = _create(sp.sd_sphere(1.0))
    o = np.array([[0.0, 0.0, 5.0]])
    d = np.array([[0.0, 0.0, -1.0]])
    hit, t, it, fs = hip.march_rays(pid, 0, o, d)
    assert hit[0] == 1 and it[0] > 0
    with pytest.raises(_native.RmError) as e:
        hip.march_rays(pid, 0, o, d, team=True)
    assert e.value.code == -1
    _native.scene_program_destroy(pid)
    cam = Camera((0.0, 0.0, 5.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 60.0, 64, 48).params14()
    for call in (lambda: hip.render(hip.make_desc(pid, 0, cam, 64, 48)), lambda: hip.sdf_eval(pid, o),
                 lambda: hip.march_rays(pid, 0, o, d), lambda: hip.render_batch(hip.make_desc(pid, 0, cam, 64, 48), cam[None])):
        with pytest.raises(_native.RmError) as e:
            call()
        assert e.value.code == -1
    with pytest.raises(_native.RmError):
        hip.render(hip.make_desc(_native.RM_SCENE_PROGRAM_BASE - 1, 0, cam, 64, 48))


def test_run_once_on_a_registered_scene(hip):
    from raymarch_algo_compare_amd.main import run_once
    from raymarch_algo_compare_amd.config import MarchConfig, RenderConfig
    names = []
    try:
        for sid in (5, 12):
            s = registry.SCENES[sid]
            name = f"Restated {sid}"
            sp.register_scene(name, sp.catalogue_expressions()[sid], lipschitz=s.lipschitz or 1.0,
                              camera_position=s.camera_position, camera_target=s.camera_target)
            names.append(name)
            for strat in ("Standard", "Segment", "Enhanced"):
                a = run_once(RenderConfig(width=64, height=48), MarchConfig(), name, strat)
                b = run_once(RenderConfig(width=64, height=48), MarchConfig(), s.name, strat)
                assert a.scene_name == name and b.scene_name == s.name
                # everything but the name and the wall-clock fields
                skip = {"scene_name", "total_time_seconds", "time_per_ray_us", "kernel_ms"}
                da = {k: v for k, v in vars(a).items() if k not in skip and "gpu_" not in k}
                db = {k: v for k, v in vars(b).items() if k not in skip and "gpu_" not in k}
                assert da.keys() == db.keys()
                for k in da:
                    va, vb = da[k], db[k]
                    if isinstance(va, np.ndarray):
                        assert np.array_equal(va, vb), (name, strat, k)
                    else:
                        assert va == vb, (name, strat, k)
    finally:
        for n in names:
            sp.unregister_scene(n)
    assert len(registry.get_all_scenes()) == 20
