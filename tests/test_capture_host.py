"""Capture on the device, without a GPU: csrc/rm_capture.h compiled for the host by g++ (tests/native/capture_check.cpp)
against a per-pixel restatement in Python floats (capture_cases.restate: `** 0.5` as camera._normalized, math.sqrt,
math.pow, the host-compiled SDF for the four samples, numpy.float32 for the final rounding), bit for bit in all six maps;
the key-light literals; the zero gradient; the all-miss frame; and the host checks of rm_capture / rm_shade_frames.

Frames come from the project's CPU oracle (oracle/oracle.py); a scene program's from the host build of the kernels'
march (the oracle has no interpreter), an extension-op twin's from the oracle's frame of its catalogue scene (the twin
renders those frames bit for bit: tests/test_gpu_scene_program_ext.py)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import capture_cases as C
from conftest import ROOT
from oracle import oracle
from raymarch_algo_compare_amd import _native, registry

SHAPES = [(16, 12), (50, 37)]
STRATEGIES = ["Standard", "Segment"]
# Sphere, Cube (creases), Thin Torus, Mandelbulb, Metaballs
CATALOGUE = [0, 2, 3, 10, 19]


@pytest.fixture(scope="module")
def host():
    return C.Host()


@pytest.fixture(scope="module")
def oracle_frames():
    """(scene id, strategy key, W, H) -> frame, rendered once"""
    cache = {}

    def get(sid, key, W, H):
        k = (sid, key, W, H)
        if k not in cache:
            scene = registry.SCENES[sid]
            r = oracle.render(sid, registry.STRATEGIES[key], C.camera14(sid, W, H), W, H, lipschitz=scene.lipschitz or 1.0, nthreads=4)
            f = {"hit": r.hit, "t": r.t, "iters": r.iters, "final_sdf": r.final_sdf}
            f["evals"] = C.synthetic_evals(f)
            cache[k] = f
        return cache[k]
    return get


def check(host, scene, cam, W, H, frame, what):
    got, calls = host.capture(scene, cam, W, H, frame)
    want = C.restate(lambda pts: host.sdf(scene, pts), cam, W, H, frame)
    C.assert_same_maps(got, want, what)
    nhit = int((frame["hit"] != 0).sum())
    assert calls == 4 * nhit, (what, calls, nhit)      # exactly four samples per hit, none on a miss
    assert np.isfinite(got["normal"]).all() and np.isfinite(got["color"]).all(), what
    return nhit


@pytest.mark.parametrize("key", STRATEGIES)
@pytest.mark.parametrize("W,H", SHAPES)
@pytest.mark.parametrize("sid", CATALOGUE)
def test_host_build_equals_the_restatement(host, oracle_frames, sid, W, H, key):
    frame = oracle_frames(sid, key, W, H)
    nhit = check(host, sid, C.camera14(sid, W, H), W, H, frame, (registry.SCENES[sid].name, key, W, H))
    assert nhit < W * H and (nhit > 0 or (W, H) == (16, 12))      # misses in every frame, hits in every 50x37 one (16x12 misses the thin torus)


@pytest.mark.parametrize("key", STRATEGIES)
@pytest.mark.parametrize("W,H", SHAPES)
def test_user_program_equals_the_restatement(host, W, H, key):
    expr = C.user_program()
    cam = C.camera14(0, W, H)
    frame = host.march_program(expr, registry.STRATEGIES[key], cam, W, H)
    assert 0 < check(host, expr, cam, W, H, frame, ("user program", key, W, H)) < W * H


@pytest.mark.parametrize("key", STRATEGIES)
@pytest.mark.parametrize("W,H", SHAPES)
def test_extension_twin_equals_the_restatement(host, oracle_frames, W, H, key):
    frame = oracle_frames(C.EXT_TWIN_ID, key, W, H)
    cam = C.camera14(C.EXT_TWIN_ID, W, H)
    twin = C.ext_twin()
    assert 0 < check(host, twin, cam, W, H, frame, ("extension twin", key, W, H)) < W * H
    # the twin's four samples are the catalogue scene's: so are its maps
    C.assert_same_maps(host.capture(twin, cam, W, H, frame)[0], host.capture(C.EXT_TWIN_ID, cam, W, H, frame)[0], "twin vs scene")


def test_band_equals_the_rows_of_the_frame(host, oracle_frames):
    W, H = 50, 37
    frame, cam = oracle_frames(0, "Standard", W, H), C.camera14(0, W, H)
    whole, _ = host.capture(0, cam, W, H, frame)
    band, _ = host.capture(0, cam, W, H, {k: v[4:12] for k, v in frame.items()}, row0=4)
    C.assert_same_maps(band, {k: v[4:12] for k, v in whole.items()}, "rows 4..12")


def test_key_light_literals_are_the_cpython_doubles(host):
    s = math.sqrt(0.6 ** 2 + 0.7 ** 2 + 0.5 ** 2)
    assert host.light() == (0.6 / s, 0.7 / s, 0.5 / s)
    assert [v.hex() for v in host.light()] == ["0x1.24e7595e85edep-1", "0x1.55b892ee46eadp-1", "0x1.e82c3f9d89e1dp-2"]


def test_equal_samples_give_the_zero_normal(host):
    """The centre of the Sphere scene's sphere: an odd frame's centre pixel is the optical axis, t the camera distance."""
    W, H = 15, 11
    cam = C.camera14(0, W, H)
    frame = {"hit": np.zeros((H, W), np.uint8), "t": np.full((H, W), 5.0), "iters": np.ones((H, W), np.int32),
             "final_sdf": np.zeros((H, W)), "evals": np.ones((H, W), np.int32)}
    frame["hit"][H // 2, W // 2] = 1
    o, d = C.camera_ray([float(v) for v in cam], W, H, W // 2, H // 2)
    assert [o[k] + 5.0 * d[k] for k in range(3)] == [0.0, 0.0, 0.0]
    f4 = host.sdf(0, [[C.EPS * k for k in ks] for ks in C.KS])
    assert len(set(f4.tolist())) == 1
    got, calls = host.capture(0, cam, W, H, frame)
    assert calls == 4
    assert got["normal"][H // 2, W // 2].tolist() == [0.0, 0.0, 0.0]
    s = 0.15 * (0.5 + 0.5 * 0.0) + 0.85 * 0.0
    assert s == 0.075
    want = [np.float32(math.pow(a * s, 0.4545)) for a in C.ALBEDO]
    assert got["color"][H // 2, W // 2].tolist() == want
    assert not np.isnan(got["normal"]).any() and not np.isnan(got["color"]).any()
    C.assert_same_maps(got, C.restate(lambda pts: host.sdf(0, pts), cam, W, H, frame), "zero gradient")


def test_all_miss_frame_is_the_background_and_evaluates_nothing(host):
    W, H = 16, 12
    for sid in (0, 10):
        cam = C.camera14(sid, W, H)
        frame = {"hit": np.zeros((H, W), np.uint8), "t": np.full((H, W), 100.5), "iters": np.full((H, W), 7, np.int32),
                 "final_sdf": np.full((H, W), 2.5), "evals": np.full((H, W), 8, np.int32)}
        got, calls = host.capture(sid, cam, W, H, frame)
        assert calls == 0
        assert not got["normal"].any() and not got["depth"].any()
        c = [float(v) for v in cam]
        for py in range(H):
            for px in range(W):
                tb = 0.5 * (C.camera_ray(c, W, H, px, py)[1][1] + 1.0)
                want = [np.float32((1.0 - tb) * a + tb * b) for a, b in zip(C.SKY_A, C.SKY_B)]
                assert got["color"][py, px].tolist() == want, (sid, px, py)
        assert got["geom"][0, 0].tolist() == [0.0, np.float32(7 / 512), np.float32(100.5 / 100.0), 2.5]


# ---- the C ABI before the device ------------------------------------------------------------------------------------------

def test_records_follow_the_header():
    import ctypes
    assert [f[0] for f in _native.RmCaptureOutputs._fields_] == ["geom", "normal", "depth", "color", "evals", "hit"]
    assert ctypes.sizeof(_native.RmCaptureOutputs) == 6 * ctypes.sizeof(ctypes.c_void_p)
    assert {"rm_capture", "rm_shade_frames"} <= set(_native.EXPORTS)


def test_argument_checks_answer_without_a_device():
    """Every host check of rm_capture and rm_shade_frames answers with its code and a message in a fresh process that never
    called rm_init; a call that passes them then needs a device."""
    code = (
        "import ctypes, numpy as np\n"
        "from raymarch_algo_compare_amd import _native\n"
        "from raymarch_algo_compare_amd import scene_program as sp\n"
        "L = _native.load()\n"
        "cam = np.array([0, 0, 5, 0, 0, -1, 1, 0, 0, 0, 1, 0, 0.77, 0.57], np.float64)\n"
        "def show(rc): print(rc, len(L.rm_last_error()))\n"
        "W, H = 8, 6\n"
        "hit = np.ones((H, W), np.uint8); geom = np.empty((H, W, 4), np.float32)\n"
        "def outs(with_hit=True): return _native.RmCaptureOutputs(geom.ctypes.data, None, None, None, None, hit.ctypes.data if with_hit else None)\n"
        "def desc(scene=0, full=True, w=W, **kw): return _native.make_desc(scene, 0, cam, w, H, full=full, **kw)\n"
        "def cap(d, o): show(L.rm_capture(None if d is None else ctypes.byref(d), None if o is None else ctypes.byref(o), None, None))\n"
        "cap(None, outs())\n"
        "cap(desc(), None)\n"
        "cap(desc(), outs(False))\n"
        "cap(desc(full=False), outs())\n"
        "cap(desc(rows=4, band_rows=4, band_stride=2), outs())\n"
        "cap(desc(w=0), outs())\n"
        "cap(desc(scene=99), outs())\n"
        "cap(desc(scene=_native.RM_SCENE_PROGRAM_BASE + 77777), outs())\n"
        "tm = _native.RmTiming(); tm.repeats = 0\n"
        "show(L.rm_capture(ctypes.byref(desc()), ctypes.byref(outs()), None, ctypes.byref(tm)))\n"
        "cap(desc(), outs())\n"
        "print('--')\n"
        "n = 2\n"
        "cams = np.stack([cam, cam]); t = np.full((n, H, W), 4.0); depth = t.astype(np.float32); hits = np.ones((n, H, W), np.uint8)\n"
        "nrm = np.empty((n, H, W, 3), np.float32); col = np.empty((n, H, W, 3), np.float32)\n"
        "p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)\n"
        "def shade(scene=0, w=W, h=H, nf=n, cams=cams, t=t, depth=None, hit=hits, normal=nrm, color=col):\n"
        "    show(L.rm_shade_frames(scene, w, h, nf, None if cams is None else cams.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),\n"
        "                           p(t), p(depth), p(hit), p(normal), p(color), None))\n"
        "shade(cams=None)\n"
        "shade(hit=None)\n"
        "shade(normal=None)\n"
        "shade(color=None)\n"
        "shade(depth=depth)\n"
        "shade(t=None)\n"
        "shade(nf=0)\n"
        "shade(nf=65536)\n"
        "bad = t.copy(); bad[1, 2, 3] = np.nan; shade(t=bad)\n"
        "bad = t.copy(); bad[0, 0, 0] = np.inf; shade(t=bad)\n"
        "badf = depth.copy(); badf[1, 5, 7] = -np.inf; shade(t=None, depth=badf)\n"
        "badc = cams.copy(); badc[1, 13] = np.nan; shade(cams=badc)\n"
        "badc = cams.copy(); badc[0, 4] = np.inf; shade(cams=badc)\n"
        "shade(w=0)\n"
        "shade(h=-1)\n"
        "shade(w=65536, h=65536, nf=1)\n"
        "shade(w=1 << 15, h=1 << 15, nf=2)\n"
        "shade(scene=99)\n"
        "shade(scene=-1)\n"
        "ops, k = sp.to_ctypes(sp.sd_sphere(1.0)); pid = _native.scene_program_create(ops, k); _native.scene_program_destroy(pid)\n"
        "shade(scene=pid)\n"
        "miss = hits.copy(); miss[1, 2, 3] = 0; bad = t.copy(); bad[1, 2, 3] = np.nan; shade(t=bad, hit=miss)\n"
        "shade()\n"
        "shade(t=None, depth=depth)\n")
    env = dict(os.environ, PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, check=True, capture_output=True, text=True).stdout
    first, second = out.strip().split("--\n")
    rows = [[int(v) for v in line.split()] for line in first.strip().splitlines()]
    ARG, DIMS, SCENE, NODEV = _native.RM_E_BAD_ARG, -3, _native.RM_E_BAD_SCENE, _native.RM_E_NO_DEVICE
    assert [r[0] for r in rows] == [ARG, ARG, ARG, ARG, ARG, DIMS, SCENE, SCENE, ARG, NODEV], first
    assert all(r[1] > 0 for r in rows), first
    rows = [[int(v) for v in line.split()] for line in second.strip().splitlines()]
    assert [r[0] for r in rows] == [ARG] * 13 + [DIMS] * 4 + [SCENE] * 3 + [NODEV] * 3, second
    assert all(r[1] > 0 for r in rows), second
