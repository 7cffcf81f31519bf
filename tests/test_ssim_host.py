"""SSIM / colour-RMSE capture scoring without a GPU: csrc/rm_ssim.h compiled for the host by g++
(tests/native/ssim_check.cpp) against a plain float64 restatement of the definition, the quantisation against the
reference's own images (tests/golden/ssim_images.npz, written by tools/gen_ssim_golden.py), the host-only behaviour of
rm_ssim_scores, and ssim.py around scoring.py.

The oracle is written here: Wang et al. 2004 with skimage's defaults, means by scipy.ndimage.uniform_filter over
float64, cropped by 3.  skimage is not installed, so NO SSIM value comes from the reference itself; what the reference
pins is the quantisation.  The bound between the host build and the oracle is 1e-9 absolute: the host's window sums are
exact integers, the oracle's running means carry about 1e-11 of rounding on (co)variances of at most 65025 * 49 / 48, and
the denominators are at least C1 * C2 ~ 380 -- a per-pixel error far below 1e-9, which a mean cannot exceed.

Section 2b feeds the host build what decides whether the quantisation is right (tests/ssim_edge_cases.py: k/255 and its
float32 neighbours, values outside [0, 1], NaN, +-inf, +-3.4e38, degenerate normals, non-finite hit depths, one hit, one
depth), the strongest contrasts, and captures one pixel apart at every tile seam; tests/test_gpu_ssim.py gives the device
the same inputs.
"""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest
from scipy.ndimage import uniform_filter

import ssim_edge_cases as E
from conftest import GOLDEN, ROOT, build_native
from raymarch_algo_compare_amd import _native, scoring, ssim

TOL = 1e-9
C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
u8p, f32p, dp = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double)


# ---- the float64 oracle ----------------------------------------------------------------------------------------------------

def oracle_plane(x, y):
    x, y = x.astype(np.float64), y.astype(np.float64)
    f = lambda a: uniform_filter(a, size=7)      # noqa: E731
    ux, uy = f(x), f(y)
    cov_norm = 49 / 48
    vx, vy, vxy = cov_norm * (f(x * x) - ux * ux), cov_norm * (f(y * y) - uy * uy), cov_norm * (f(x * y) - ux * uy)
    S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))
    return float(S[3:-3, 3:-3].mean())


def oracle_image(x, y):
    """a (H, W) or (H, W, 3) image pair: the mean of the channels' scores"""
    if x.ndim == 2:
        return oracle_plane(x, y)
    return float(np.mean([oracle_plane(x[..., c], y[..., c]) for c in range(x.shape[2])]))


def oracle_scores(method, reference):
    """the four scores of two capture dicts, through ssim.to_images"""
    with np.errstate(invalid="ignore", over="ignore"):      # non-finite maps (ssim_edge_cases.py)
        dr = ssim.depth_range(reference)
        r, m = ssim.to_images(reference, dr), ssim.to_images(method, dr)
    out = [oracle_image(r["depth"], m["depth"]), None, None, None]
    if r["normal"] is not None and m["normal"] is not None:
        out[1] = oracle_image(r["normal"], m["normal"])
    if r["color"] is not None and m["color"] is not None:
        out[2] = oracle_image(r["color"], m["color"])
        out[3] = float(np.sqrt(np.mean((r["color"].astype(np.float64) - m["color"]) ** 2)))
    return out


# ---- the host build ----------------------------------------------------------------------------------------------------

def load_host_lib():
    """tests/native/ssim_check.cpp built by g++, prototypes declared"""
    L = ctypes.CDLL(build_native("ssim_check"))
    L.rms_depth_range.argtypes = [ctypes.c_int, ctypes.c_int, f32p, u8p, dp]
    L.rms_images.argtypes = [ctypes.c_int, ctypes.c_int, f32p, f32p, f32p, u8p, ctypes.c_double, ctypes.c_double, u8p]
    L.rms_plane_ssim.argtypes = [u8p, u8p, ctypes.c_int, ctypes.c_int]
    L.rms_plane_ssim.restype = ctypes.c_double
    L.rms_scores.argtypes = [ctypes.c_int, ctypes.c_int, f32p, f32p, f32p, u8p, f32p, f32p, f32p, u8p, dp]
    return L


@pytest.fixture(scope="module")
def lib():
    return load_host_lib()


def _f(a):
    return None if a is None else a.ctypes.data_as(f32p)


def _maps(c):
    """contiguous float32 / uint8 maps of a capture dict (normal / color None when absent)"""
    g = lambda k: None if c.get(k) is None else np.ascontiguousarray(c[k], np.float32)      # noqa: E731
    return g("depth"), g("normal"), g("color"), np.ascontiguousarray(np.asarray(c["hit"]) != 0, np.uint8)


def host_scores(lib, method, reference, hit_byte=1):
    """rms_scores; hit_byte: what a hit is written as in the two hit maps"""
    H, W = np.shape(reference["hit"])
    rd, rn, rc, rh = _maps(reference)
    md, mn, mc, mh = _maps(method)
    rh, mh = rh * np.uint8(hit_byte), mh * np.uint8(hit_byte)
    out = np.empty(4)
    assert lib.rms_scores(W, H, _f(rd), _f(rn), _f(rc), rh.ctypes.data_as(u8p), _f(md), _f(mn), _f(mc), mh.ctypes.data_as(u8p),
                          out.ctypes.data_as(dp)) == 0
    return out


def host_image(lib, x, y):
    """as oracle_image, by the host build"""
    planes = [(x, y)] if x.ndim == 2 else [(x[..., c], y[..., c]) for c in range(x.shape[2])]
    m = []
    for a, b in planes:
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        m.append(lib.rms_plane_ssim(a.ctypes.data_as(u8p), b.ctypes.data_as(u8p), a.shape[1], a.shape[0]))
    return m[0] if len(m) == 1 else (m[0] + m[1] + m[2]) / 3.0


# ---- inputs ------------------------------------------------------------------------------------------------------------

SHAPES = [(7, 7), (8, 9), (40, 33), (64, 48)]      # (W, H); 7x7: a single window


def image_pairs(W, H, ch, seed):
    """(name, x, y) uint8 pairs of shape (H, W) or (H, W, 3): noise, gradients, a one-pixel shift"""
    rng = np.random.default_rng(seed)
    shape = (H, W) if ch == 1 else (H, W, ch)
    yy, xx = np.mgrid[0:H, 0:W]
    grad = (255.0 * (xx + 2 * yy) / max(W + 2 * H - 3, 1))
    grad2 = (255.0 * (0.5 + 0.5 * np.sin(0.3 * xx + 0.2 * yy)))
    if ch > 1:
        grad = np.stack([grad, grad[::-1], grad[:, ::-1]], axis=2)
        grad2 = np.stack([grad2, grad2[::-1], 255.0 - grad2], axis=2)
    noise = rng.integers(0, 256, shape).astype(np.uint8)
    yield "noise", noise, rng.integers(0, 256, shape).astype(np.uint8)
    yield "noisy", noise, np.clip(noise.astype(int) + rng.integers(-12, 13, shape), 0, 255).astype(np.uint8)
    yield "gradients", grad.astype(np.uint8), grad2.astype(np.uint8)
    yield "shift", grad2.astype(np.uint8), np.roll(grad2.astype(np.uint8), 1, axis=1)
    yield "noise-shift", noise, np.roll(noise, 1, axis=0)


def capture(W, H, seed, all_miss=False, color=True, normal=True):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    r2 = ((xx - W / 2) / (0.4 * W)) ** 2 + ((yy - H / 2) / (0.4 * H)) ** 2
    hit = (r2 < 1.0) & ~all_miss
    z = np.sqrt(np.maximum(1.0 - r2, 0.0))
    n = np.stack([(xx - W / 2) / (0.4 * W), (yy - H / 2) / (0.4 * H), z], axis=2) + rng.normal(0, 0.05, (H, W, 3))
    c = {"hit": hit, "depth": (4.0 - z + rng.normal(0, 0.02, (H, W))).astype(np.float32)}
    if normal:
        c["normal"] = (n / np.linalg.norm(n, axis=2, keepdims=True)).astype(np.float32)
    if color:
        c["color"] = np.clip(0.2 + 0.7 * z[..., None] * np.array([1.0, 0.8, 0.6]) + rng.normal(0, 0.03, (H, W, 3)), 0, 1).astype(np.float32)
    return c


# ---- 1. the arithmetic -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("W,H", SHAPES)
def test_host_build_equals_the_float64_restatement(lib, W, H, ch):
    for name, x, y in image_pairs(W, H, ch, seed=W * 100 + H + ch):
        got, want = host_image(lib, x, y), oracle_image(x, y)
        print(f"{W}x{H}x{ch} {name}: host {got!r} oracle {want!r} diff {abs(got - want):.3g}")
        assert abs(got - want) <= TOL, (name, got, want)
        assert host_image(lib, x, x) == 1.0 and host_image(lib, y, y) == 1.0, name      # identical images: exactly 1


@pytest.mark.parametrize("W,H", SHAPES)
def test_constant_images_match_the_closed_form(lib, W, H):
    assert E.CONSTANT_PAIRS == ((0, 255), (10, 200), (128, 129), (255, 254), (0, 1))
    for a, b in E.CONSTANT_PAIRS:
        x, y = np.full((H, W), a, np.uint8), np.full((H, W), b, np.uint8)
        want = (2.0 * a * b + C1) / (a * a + b * b + C1)
        assert abs(host_image(lib, x, y) - want) <= 1e-12, (a, b)
        assert abs(oracle_image(x, y) - want) <= TOL, (a, b)


@pytest.mark.parametrize("W,H", SHAPES)
def test_capture_scores_equal_the_restatement(lib, W, H):
    ref = capture(W, H, 1)
    cases = [("noisy", capture(W, H, 2), ref), ("all-miss reference", capture(W, H, 3), capture(W, H, 4, all_miss=True)),
             ("all-miss both", capture(W, H, 5, all_miss=True), capture(W, H, 6, all_miss=True)),
             ("all-miss method", capture(W, H, 7, all_miss=True), ref),
             ("no colour", capture(W, H, 8, color=False), capture(W, H, 9, color=False)),
             ("depth only", capture(W, H, 8, color=False, normal=False), capture(W, H, 9, color=False, normal=False))]
    for name, m, r in cases:
        got, want = host_scores(lib, m, r), oracle_scores(m, r)
        print(f"{W}x{H} {name}: host {list(got)} oracle {want}")
        for g, w in zip(got, want):
            if w is None:
                assert np.isnan(g), name
            else:
                assert abs(g - w) <= TOL, (name, g, w)
        if want[3] is not None:      # an exact integer sum, one division, one square root: 1 ulp
            assert abs(got[3] - want[3]) <= np.spacing(want[3]), (name, got[3], want[3])
        same = host_scores(lib, r, r)
        assert [v for v in same if not np.isnan(v)] == ([1.0, 1.0, 1.0, 0.0] if "color" in r else [1.0, 1.0] if "normal" in r else [1.0]), name
    assert ssim.depth_range(capture(W, H, 4, all_miss=True)) == (0.0, 1.0)


# ---- 2. the quantisation, against the reference's images ---------------------------------------------------------------------

def golden_cases():
    """(index, arrays) of the fixture's cases; c4 and later also carry own_drange and img_depth_own"""
    z = np.load(os.path.join(GOLDEN, "ssim_images.npz"))
    for i in range(int(z["ncases"][0])):
        keys = ["depth", "normal", "color", "hit", "drange", "img_depth", "img_normal", "img_color"]
        keys += [k for k in ("own_drange", "img_depth_own") if f"c{i}_{k}" in z.files]
        yield i, {k: z[f"c{i}_{k}"] for k in keys}


def golden_capture(g):
    return {"depth": g["depth"], "normal": g["normal"], "color": g["color"], "hit": g["hit"]}


def same_range(a, b):
    """two (lo, hi), a NaN equal to a NaN"""
    return np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)


def host_planes(lib, cap, lo, hi):
    """the (7, H, W) planes of rms_images, untouched ones 0"""
    H, W = np.shape(cap["hit"])
    planes = np.zeros((7, H, W), np.uint8)
    d, nrm, col, hit = _maps(cap)
    lib.rms_images(W, H, _f(d), _f(nrm), _f(col), hit.ctypes.data_as(u8p), lo, hi, planes.ctypes.data_as(u8p))
    return planes


def host_depth_range(lib, cap):
    H, W = np.shape(cap["hit"])
    d, _, _, hit = _maps(cap)
    lohi = np.empty(2)
    lib.rms_depth_range(W, H, _f(d), hit.ctypes.data_as(u8p), lohi.ctypes.data_as(dp))
    return tuple(lohi)


def test_quantisation_equals_the_reference_images(lib):
    n = own = 0
    for i, g in golden_cases():
        cap = golden_capture(g)
        ranges = [("", tuple(float(v) for v in g["drange"]))]
        if "own_drange" in g:      # the path rm_ssim_scores takes: the range of the capture's own hit depths
            ranges.append(("_own", tuple(float(v) for v in g["own_drange"])))
            own += 1
        for suffix, (lo, hi) in ranges:
            with np.errstate(invalid="ignore", over="ignore"):
                img = ssim.to_images(cap, (lo, hi))
            planes = host_planes(lib, cap, lo, hi)
            for key, sl in (("depth", planes[0]), ("normal", np.moveaxis(planes[1:4], 0, 2)), ("color", np.moveaxis(planes[4:7], 0, 2))):
                want = g["img_depth_own"] if (key, suffix) == ("depth", "_own") else g["img_" + key]
                assert img[key].dtype == np.uint8 and img[key].tobytes() == want.tobytes(), (i, key, suffix, "ssim.to_images")
                assert sl.tobytes() == want.tobytes(), (i, key, suffix, "host build")
        n += 1
    assert n == 12 and own == 8
    # the range of a capture's own depth, by both; a NaN on any hit makes it (nan, nan), as the reference's depth_range_of
    nan_ranges = 0
    for i, g in golden_cases():
        cap = golden_capture(g)
        got = host_depth_range(lib, cap)
        assert same_range(got, ssim.depth_range(cap)), (i, got)
        if "own_drange" in g:
            assert same_range(got, g["own_drange"]), (i, got, g["own_drange"])
            assert same_range(ssim.depth_range(cap), g["own_drange"]), i
            nan_ranges += bool(np.isnan(g["own_drange"]).all())
    assert nan_ranges == 2      # NaN at a late hit and at the first hit


# ---- 2b. edge inputs (ssim_edge_cases.py) -----------------------------------------------------------------------------------

def assert_scores_close(got, want, name):
    for g, w in zip(got, want):
        if w is None:
            assert np.isnan(g), name
        else:
            assert abs(g - w) <= TOL, (name, g, w)      # a NaN score fails here


@pytest.mark.parametrize("W,H", E.SHAPES)
def test_edge_captures_equal_the_restatement(lib, W, H):
    """Non-finite and edge-of-rounding maps: the host build's images equal ssim.to_images byte for byte and its scores the
    restatement's.  The reference with a NaN depth on a late hit failed before ssim_depth_minmax propagated the NaN."""
    for name, m, r in E.edge_pairs(W, H):
        with np.errstate(invalid="ignore", over="ignore"):
            dr = ssim.depth_range(r)
            assert same_range(host_depth_range(lib, r), dr), name
            for cap in (m, r):
                img, planes = ssim.to_images(cap, dr), host_planes(lib, cap, dr[0], dr[1])
                assert planes[0].tobytes() == img["depth"].tobytes(), (name, "depth")
                if img["normal"] is not None:
                    assert np.moveaxis(planes[1:4], 0, 2).tobytes() == img["normal"].tobytes(), (name, "normal")
                if img["color"] is not None:
                    assert np.moveaxis(planes[4:7], 0, 2).tobytes() == img["color"].tobytes(), (name, "color")
        got, want = host_scores(lib, m, r), oracle_scores(m, r)
        print(f"{W}x{H} {name}: range {dr} host {list(got)} oracle {want}")
        assert_scores_close(got, want, name)
        if want[3] is not None:
            assert abs(got[3] - want[3]) <= np.spacing(want[3]), (name, got[3], want[3])


def period_1_is_negative(name, scores):
    return "period 1" not in name or (scores[0] < -0.9 and scores[1] < -0.9 and scores[2] < -0.9)


@pytest.mark.parametrize("W,H", E.SHAPES)
def test_contrast_pairs(lib, W, H):
    for name, m, r, ab in E.contrast_pairs(W, H):
        got, want = host_scores(lib, m, r), oracle_scores(m, r)
        print(f"{W}x{H} {name}: host {list(got)} oracle {want}")
        assert_scores_close(got, want, name)
        for g, w in zip(got[:3], want[:3]):
            assert (g < 0.0) == (w < 0.0), (name, g, w)
        if ab is None:      # a checkerboard against its inverse; of period 7, a small image holds one field only
            assert period_1_is_negative(name, got)
        else:
            a, b = ab
            closed = (2.0 * a * b + C1) / (a * a + b * b + C1)
            assert abs(got[1] - closed) <= 1e-12 and abs(got[2] - closed) <= 1e-12, (name, got, closed)
            assert got[0] == 1.0 and got[3] == abs(a - b), (name, got)


@pytest.mark.parametrize("W,H", E.SHAPES)
def test_one_pixel_is_counted_exactly_once(lib, W, H):
    """ssim_owns: wherever the one differing pixel lies, the colour RMSE is that of one squared difference"""
    for name, m, r, d in E.one_hot_pairs(W, H):
        got = host_scores(lib, m, r)
        want = math.sqrt(d * d / (3 * W * H))
        assert abs(got[3] - want) <= np.spacing(want), (name, got[3], want)
        assert got[0] == 1.0 and got[1] == 1.0 and got[2] < 1.0, (name, got)


def test_any_non_zero_hit_byte_is_a_hit(lib):
    for name, m, r in E.edge_pairs(40, 33)[:4]:
        one = host_scores(lib, m, r)
        for byte in (2, 255):
            assert host_scores(lib, m, r, hit_byte=byte).tobytes() == one.tobytes(), (name, byte)


# ---- 3. the C ABI before the device -------------------------------------------------------------------------------------

def test_abi_record_and_errors_without_a_device():
    """RmCaptureMaps as the header lays it out; every host check of rm_ssim_scores answers with its code and a message, in a
    fresh process that never called rm_init; a valid call then needs a device."""
    assert ctypes.sizeof(_native.RmCaptureMaps) == 4 * ctypes.sizeof(ctypes.c_void_p)
    assert [f[0] for f in _native.RmCaptureMaps._fields_] == ["depth", "normal", "color", "hit"]
    code = (
        "import ctypes, numpy as np\n"
        "from raymarch_algo_compare_amd import _native\n"
        "L = _native.load()\n"
        "def cap(w, h, color=True):\n"
        "    c = {'depth': np.ones((h, w), np.float32), 'normal': np.zeros((h, w, 3), np.float32), 'hit': np.ones((h, w), bool)}\n"
        "    if color: c['color'] = np.zeros((h, w, 3), np.float32)\n"
        "    return _native.capture_maps(c, w, h)\n"
        "out = np.empty(4); po = out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))\n"
        "def call(w, h, r, m, n):\n"
        "    rc = L.rm_ssim_scores(w, h, None if r is None else ctypes.byref(r[0]), None if m is None else ctypes.byref(m[0]), n, po, None)\n"
        "    print(rc, len(L.rm_last_error()))\n"
        "call(6, 7, cap(6, 7), cap(6, 7), 1)\n"
        "call(7, 6, cap(7, 6), cap(7, 6), 1)\n"
        "call(8, 8, None, cap(8, 8), 1)\n"
        "call(8, 8, cap(8, 8), None, 1)\n"
        "call(8, 8, cap(8, 8), cap(8, 8), 0)\n"
        "call(8, 8, cap(8, 8), cap(8, 8, color=False), 1)\n"
        "call(8, 8, cap(8, 8, color=False), cap(8, 8), 1)\n"
        "nod = cap(8, 8); nod[0].depth = None\n"
        "call(8, 8, cap(8, 8), nod, 1)\n"
        "call(8, 8, cap(8, 8), cap(8, 8), 1)\n")
    env = dict(os.environ, PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, check=True, capture_output=True, text=True).stdout
    rows = [[int(v) for v in line.split()] for line in out.strip().splitlines()]
    BAD_DIMS, BAD_ARG = -3, _native.RM_E_BAD_ARG
    assert [r[0] for r in rows] == [BAD_DIMS, BAD_DIMS, BAD_ARG, BAD_ARG, BAD_ARG, BAD_ARG, BAD_ARG, BAD_ARG, _native.RM_E_NO_DEVICE], out
    assert all(r[1] > 0 for r in rows), out


# ---- 4. ssim.py around scoring.py ---------------------------------------------------------------------------------------

def test_score_capture_full_fills_the_tertiary_tier(monkeypatch):
    m, r = capture(40, 33, 11), capture(40, 33, 12)
    with pytest.raises(NotImplementedError):
        scoring.score_capture(m, r, compute_ssim=True)
    want = oracle_scores(m, r)
    seen = []

    def fake(width, height, reference, methods, warmup=0, repeats=0):      # stands in for the device call
        seen.append((width, height, sorted(reference), len(methods)))
        return np.array([want] * len(methods), np.float64)

    monkeypatch.setattr(_native, "ssim_scores", fake)
    base = scoring.score_capture(m, r, compute_ssim=False)
    full = ssim.score_capture_full(m, r)
    assert seen == [(40, 33, ["color", "depth", "hit", "normal"], 1)]
    for key in ("hit", "depth", "normal", "primary", "secondary"):
        assert full[key] == base[key], key
    assert tuple(full["ssim"]) == scoring.SSIM_KEYS and full["tertiary"] is full["ssim"]
    assert [full["tertiary"][k] for k in scoring.SSIM_KEYS] == want
    assert base["ssim"] == dict.fromkeys(scoring.SSIM_KEYS)
    # a map one side lacks is dropped on both sides, and its scores are None
    monkeypatch.setattr(_native, "ssim_scores", lambda w, h, ref, ms, **kw: np.array([[0.5, 0.25, np.nan, np.nan]] * len(ms)))
    r2 = {k: v for k, v in r.items() if k != "color"}
    got = ssim.ssim_scores_batch([m, m], r2)
    assert got == [{"depth_ssim": 0.5, "normal_ssim": 0.25, "color_ssim": None, "color_rmse": None}] * 2
    assert ssim.ssim_scores_batch([], r) == []
    with pytest.raises(ValueError):
        ssim.ssim_scores(capture(8, 6, 1), capture(8, 6, 2))
    with pytest.raises(ValueError):
        ssim.ssim_scores(capture(8, 8, 1), capture(9, 8, 2))


def test_sweep_ssim_needs_an_oracle():
    from raymarch_algo_compare_amd import sweep
    assert sweep.SSIM_FIELDS == list(scoring.SSIM_KEYS)
    with pytest.raises(ValueError):
        sweep.run_sweep(["Sphere"], ["Standard"], ssim=True)
    with pytest.raises(SystemExit):
        sweep.main(["--scenes", "Sphere", "--strategies", "Standard", "--ssim"])
