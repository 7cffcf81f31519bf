"""Capture on the device (rm_capture, rm_shade_frames, GPURunner.capture(device=True), sweep --device-capture) on the
MI355X: the capture kernel against the g++ build of csrc/rm_capture.h (tests/native/capture_check.cpp, pinned to a
Python restatement by tests/test_capture_host.py) bit for bit in all six maps; against rm_render_outputs; bands; timed
calls; batches of frames; and against the unchanged host path of GPURunner.capture.

Frames are 50x37 unless stated: 1850 pixels are no multiple of the 256-thread workgroup, so the last one is partial.

Bounds against the host path.  The two paths differ by an ulp-level shift of the hit point (runner.ray_directions
normalises with / sqrt, the kernels with pow(., 0.5) and a reciprocal multiply) and by <= 1 ulp of binary64 in NumPy's
`@` and `**`.  After rounding to float a map with values in [-1, 1] moves by at most one float ulp (2^-23 relative, so
<= 2^-23 absolute below 1; 2^-22 bounds a step across a binade edge), and a colour near zero by at most
pow(2.2e-16, 0.4545) ~ 7.6e-8 < 2^-22; an 8-bit level is far coarser, so the images differ by at most one level (a value
that sits on a level edge).  The float bound is asserted on the smooth scenes only: at a crease the ulp shift can move a
sample across it."""
import numpy as np
import pytest

import capture_cases as C
from raymarch_algo_compare_amd import _native, registry, ssim, sweep
from raymarch_algo_compare_amd import scene_program as sp
from raymarch_algo_compare_amd.config import MarchConfig, RenderConfig
from raymarch_algo_compare_amd.runner import GPURunner

pytestmark = pytest.mark.gpu

W, H = 50, 37
FLOAT_BOUND = 2.0 ** -22
SMOOTH = (0, 3, 19)      # Sphere, Thin Torus, Metaballs


@pytest.fixture(scope="module")
def host():
    return C.Host()


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


def desc_of(scene_id, kid, cam, lipschitz=1.0, w=W, h=H, **kw):
    return _native.make_desc(scene_id, kid, cam, w, h, full=True, lipschitz=lipschitz, **kw)


def frame_of(r):
    return {"hit": r["hit"], "t": r["t_raw"], "iters": r["iters"], "final_sdf": r["final_sdf"], "evals": r["evals"]}


def device_and_host(host, scene_id, host_scene, kid, cam, lipschitz=1.0):
    """(rm_capture's maps, the host build's maps from the device's own march outputs, the render)"""
    desc = desc_of(scene_id, kid, cam, lipschitz)
    r = _native.render(desc, want_t_raw=True, want_final_sdf=True, want_evals=True)
    got = _native.capture(desc)
    want, _ = host.capture(host_scene, cam, W, H, frame_of(r))
    return got, want, r


# ---- 1. the device equals the host build ------------------------------------------------------------------------------------

@pytest.mark.parametrize("sid", range(20))
def test_catalogue_scenes_equal_the_host_build(hip, host, sid):
    scene = registry.SCENES[sid]
    got, want, r = device_and_host(host, sid, sid, registry.STRATEGIES["Standard"], C.camera14(sid, W, H))
    assert np.array_equal(got["hit"], r["hit"])
    C.assert_same_maps(got, want, scene.name)
    assert np.isfinite(got["normal"]).all() and np.isfinite(got["color"]).all()


@pytest.mark.parametrize("key", list(registry.STRATEGIES))
@pytest.mark.parametrize("sid", [0, 10])
def test_every_strategy_equals_the_host_build(hip, host, sid, key):
    scene = registry.SCENES[sid]
    got, want, r = device_and_host(host, sid, sid, registry.STRATEGIES[key], C.camera14(sid, W, H), scene.lipschitz or 1.0)
    C.assert_same_maps(got, want, (scene.name, key))
    assert 0 < int(r["hit"].sum()) < W * H


def test_user_program_and_extension_twin_equal_the_host_build(hip, host, programs):
    expr = C.user_program()
    got, want, r = device_and_host(host, programs(expr), expr, 0, C.camera14(0, W, H))
    C.assert_same_maps(got, want, "user program")
    assert 0 < int(r["hit"].sum()) < W * H
    twin = C.ext_twin()
    lip = registry.SCENES[C.EXT_TWIN_ID].lipschitz or 1.0
    cam = C.camera14(C.EXT_TWIN_ID, W, H)
    got, want, r = device_and_host(host, programs(twin, lip), twin, 0, cam, lip)
    C.assert_same_maps(got, want, "extension twin")
    assert 0 < int(r["hit"].sum()) < W * H
    # ... and the twin's capture is its catalogue scene's
    C.assert_same_maps(got, _native.capture(desc_of(C.EXT_TWIN_ID, 0, cam, lip)), "twin vs scene")


# ---- 2. consistency with the render call --------------------------------------------------------------------------------

@pytest.mark.parametrize("sid", [0, 10])
def test_capture_restates_the_render(hip, sid):
    cam = C.camera14(sid, W, H)
    desc = desc_of(sid, 0, cam)
    r = _native.render(desc, want_t_raw=True, want_final_sdf=True, want_evals=True)
    c = _native.capture(desc)
    assert np.array_equal(c["hit"], r["hit"])
    assert C.bits32(c["depth"]).tobytes() == C.bits32(r["depth"]).tobytes()
    assert C.bits32(c["evals"]).tobytes() == C.bits32(r["evals"].astype(np.float32)).tobytes()
    geom = np.empty((H, W, 4), np.float32)
    geom[..., 0] = r["hit"]
    geom[..., 1] = r["iters"] / 512.0
    geom[..., 2] = r["t_raw"] / 100.0
    geom[..., 3] = r["final_sdf"]
    assert C.bits32(c["geom"]).tobytes() == C.bits32(geom).tobytes()
    assert c["stats"]["hit_count"] == r["stats"]["hit_count"] == int(r["hit"].sum())
    # only the requested maps come back
    part = _native.capture(desc, want=("normal",))
    assert sorted(k for k in part if k in C.TAILS) == ["normal"]
    C.assert_same_maps(part, c, "normal alone", keys=("normal", "hit"))
    # a band equals those rows of the whole frame
    band = _native.capture(desc_of(sid, 0, cam, row0=4, rows=8))
    C.assert_same_maps(band, {k: c[k][4:12] for k in C.MAPS}, "rows 4..12")
    # the timed call gives the same bits
    timed = _native.capture(desc, warmup=1, repeats=2)
    C.assert_same_maps(timed, c, "timed")
    assert len(timed["timing"]["ms_each"]) == 2 and all(ms > 0.0 for ms in timed["timing"]["ms_each"])


# ---- 3. rm_shade_frames ---------------------------------------------------------------------------------------------------

def eleven_cameras(sid):
    from raymarch_algo_compare_amd.camera import Camera
    return [Camera((0.4 * i - 2.0, 0.3 * (i % 3), 3.0 + 0.2 * i), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 60.0, W, H).params14()
            for i in range(11)]


@pytest.mark.parametrize("sid", [0, 10])
def test_shade_frames_equals_capture_alone_and_in_a_batch(hip, sid):
    cams = eleven_cameras(sid)
    caps, rs = [], []
    for cam in cams:
        desc = desc_of(sid, 0, cam)
        rs.append(_native.render(desc, want_t_raw=True))
        caps.append(_native.capture(desc, want=("normal", "color")))
    assert len({c["hit"].tobytes() for c in caps}) > 1      # the cameras see different frames
    one = [_native.shade_frames(sid, [cam], r["hit"][None], t=r["t_raw"][None]) for cam, r in zip(cams, rs)]
    for i, (c, o) in enumerate(zip(caps, one)):
        C.assert_same_maps({k: o[k][0] for k in o}, c, ("single", i), keys=("normal", "color"))
    batch = _native.shade_frames(sid, cams, np.stack([r["hit"] for r in rs]), t=np.stack([r["t_raw"] for r in rs]))
    assert batch["normal"].shape == (11, H, W, 3)
    for i, c in enumerate(caps):
        C.assert_same_maps({k: batch[k][i] for k in ("normal", "color")}, c, ("batch", i), keys=("normal", "color"))
    # a frame without the leading axis
    flat = _native.shade_frames(sid, cams[3], rs[3]["hit"], t=rs[3]["t_raw"])
    C.assert_same_maps(flat, caps[3], "one frame", keys=("normal", "color"))
    # fp32 depth is widened: the same as its double
    d32 = np.stack([r["depth"] for r in rs])
    hits = np.stack([r["hit"] for r in rs])
    a = _native.shade_frames(sid, cams, hits, depth=d32)
    b = _native.shade_frames(sid, cams, hits, t=d32.astype(np.float64))
    C.assert_same_maps(a, b, "depth vs t", keys=("normal", "color"))


def test_all_hit_and_all_miss_frames_in_one_batch_and_workspace_reuse(hip, host):
    cam = C.camera14(0, W, H)
    hit = np.stack([np.ones((H, W), np.uint8), np.zeros((H, W), np.uint8)])
    t = np.stack([np.full((H, W), 4.0), np.full((H, W), np.nan)])      # a miss's depth is never read
    got = _native.shade_frames(0, [cam, cam], hit, t=t)
    z = np.zeros((H, W))
    for f in range(2):
        frame = {"hit": hit[f], "t": np.nan_to_num(t[f]), "iters": z.astype(np.int32), "final_sdf": z, "evals": z.astype(np.int32)}
        want, calls = host.capture(0, cam, W, H, frame)
        assert calls == (4 * W * H if f == 0 else 0)
        C.assert_same_maps({k: got[k][f] for k in got}, want, ("all hit", "all miss")[f], keys=("normal", "color"))
    assert not got["normal"][1].any()
    # the workspace is reused across two shapes
    first = None
    for w, h in ((50, 37), (16, 12), (50, 37)):
        cam = C.camera14(0, w, h)
        c = _native.capture(_native.make_desc(0, 0, cam, w, h, full=True))
        r = _native.render(_native.make_desc(0, 0, cam, w, h, full=True), want_t_raw=True, want_final_sdf=True, want_evals=True)
        C.assert_same_maps(c, host.capture(0, cam, w, h, frame_of(r))[0], (w, h))
        s = _native.shade_frames(0, cam, r["hit"], t=r["t_raw"])
        C.assert_same_maps(s, c, ("shade", w, h), keys=("normal", "color"))
        if (w, h) == (50, 37):
            if first is None:
                first = c
            C.assert_same_maps(c, first, "50x37 again")


# ---- 4. against the unchanged host path ---------------------------------------------------------------------------------

@pytest.mark.parametrize("sid", range(20))
def test_device_capture_against_the_host_path(hip, sid, capsys):
    scene = registry.SCENES[sid]
    rc = RenderConfig(width=W, height=H, camera_position=scene.camera_position or (0.0, 0.0, 5.0),
                      camera_target=scene.camera_target or (0.0, 0.0, 0.0))
    runner = GPURunner()
    a = runner.capture(sid, 0, rc, MarchConfig(), device=False)
    b = runner.capture(sid, 0, rc, MarchConfig(), device=True)
    assert sorted(a) == sorted(b) and all(a[k].shape == b[k].shape and a[k].dtype == b[k].dtype for k in a)
    C.assert_same_maps(b, a, scene.name, keys=("hit", "depth", "evals", "geom"))
    dr = ssim.depth_range(a)
    ia, ib = ssim.to_images(a, dr), ssim.to_images(b, dr)
    lv = {k: int(np.abs(ia[k].astype(int) - ib[k]).max()) for k in ("normal", "color")}
    fl = {k: float(np.abs(a[k].astype(np.float64) - b[k]).max()) for k in ("normal", "color")}
    with capsys.disabled():
        print(f"\n{scene.name}: max 8-bit level difference {lv}, max float difference {fl}")
    assert lv["normal"] <= 1 and lv["color"] <= 1, (scene.name, lv)
    if sid in SMOOTH:
        assert fl["normal"] <= FLOAT_BOUND and fl["color"] <= FLOAT_BOUND, (scene.name, fl)


# ---- 5. the sweep ---------------------------------------------------------------------------------------------------------

def test_sweep_device_capture(hip, tmp_path, monkeypatch):
    """The SSIM columns of `--oracle interval --ssim --device-capture`.  Of the four, depth_ssim and normal_ssim are finite
    numbers; color_ssim and color_rmse are empty cells with the switch as without it: the interval oracle's captures carry
    no colour, so the sweep has nothing to score a colour against (sweep.SSIM_FIELDS), and filling them would change the
    default output's meaning.  The shaded colour is checked where a reference exists, in sections 1 to 4."""
    args = ["--scenes", "Sphere", "--strategies", "Standard,Relaxed", "--width", "40", "--height", "33", "--budgets", "32,512",
            "--oracle", "interval", "--ssim"]
    shaded = []
    real = _native.shade_frames

    def spy(scene_id, cams, hit, **kw):
        out = real(scene_id, cams, hit, **kw)
        shaded.append((np.asarray(hit).copy(), np.asarray(kw["depth"]).copy(), out["normal"].copy()))
        return out

    monkeypatch.setattr(_native, "shade_frames", spy)
    dev_csv, host_csv, host2_csv = (str(tmp_path / n) for n in ("dev.csv", "host.csv", "host2.csv"))
    assert sweep.main(args + ["--device-capture", "--out", dev_csv]) == 0
    n_calls = len(shaded)
    assert n_calls > 0
    assert sweep.main(args + ["--out", host_csv]) == 0
    assert sweep.main(args + ["--out", host2_csv]) == 0
    assert len(shaded) == n_calls      # without the switch the host path runs: no rm_shade_frames call
    import csv

    def rows(path):
        with open(path, newline="", encoding="utf-8") as f:
            return list(csv.DictReader(f))

    dev, hst, hst2 = rows(dev_csv), rows(host_csv), rows(host2_csv)
    assert list(dev[0]) == list(hst[0]) and len(dev) == len(hst) > 0
    strip = lambda rs: [{k: v for k, v in r.items() if k != "ms_per_frame"} for r in rs]      # noqa: E731
    assert strip(hst) == strip(hst2)      # the default path is deterministic (timings aside)
    for r in dev:
        assert np.isfinite(float(r["depth_ssim"])) and np.isfinite(float(r["normal_ssim"])), r
        assert r["color_ssim"] == "" and r["color_rmse"] == ""      # the oracle captures carry no colour
    # everything but the normal column is the host path's; the normal column is ssim_scores_batch of rm_shade_frames' normals
    for d, h in zip(dev, hst):
        assert {k: v for k, v in d.items() if k not in ("ms_per_frame", "normal_ssim")} == \
               {k: v for k, v in h.items() if k not in ("ms_per_frame", "normal_ssim")}
    scene = registry.get_scene_by_name("Sphere")
    truth = sweep.oracle_frames_for(scene, 40, 33, "interval", sweep.interval_oracle.DEFAULT_TOL)
    vps = [vp.name for vp in sweep.viewpoints_for(scene)]
    assert n_calls == len(vps)      # one call per viewpoint, all kept rows in it
    want = {}
    for name, (hit, depth, normal) in zip(vps, shaded[:n_calls]):
        methods = [{"hit": hit[i] != 0, "depth": depth[i], "normal": normal[i]} for i in range(len(hit))]
        want[name] = [s["normal_ssim"] for s in ssim.ssim_scores_batch(methods, truth[name])]
    for name in vps:
        got = [float(r["normal_ssim"]) for r in dev if r["viewpoint"] == name]      # row order: strategy, then budget
        assert len(got) == 4 and got == want[name], name
