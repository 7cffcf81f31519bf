"""Capture scoring (hit-mask counts, depth error, normal angle, exact percentiles, the silhouette band) without a GPU:
csrc/rm_score.h compiled for the host by g++ (tests/native/score_check.cpp) against scoring.py on every case of
tests/score_cases.py, the binding of the two new records, the host-only behaviour of rm_score_captures, and
score_device.py around it.  tests/test_gpu_score.py gives the device the same inputs and asks for the host build's bits.

What is asked of a result against NumPy (check_against_numpy, also used for real captures on the GPU):
  * counts, and through them IoU and the rates: equal.  The band equals scoring.silhouette_band pixel for pixel.
  * depth_p95 == np.percentile(|gap|, 95) and depth_med == np.median(|gap|) bit for bit (a NaN equals a NaN): they are exact
    order statistics combined by NumPy's own expressions.
  * sums.  Two summation orders of n non-negative terms each differ from the exact sum by at most (n - 1) * 2^-53 relative,
    so from each other by at most 2 (n - 1) * 2^-53 relative: that bounds depth_mae, sum gap^2 / n and the mean angle.  The
    square root halves a relative error, so depth_rmse is held to the same bound.  depth_signed sums signed terms whose
    magnitudes sum to n * mae: absolute bound 2 (n - 1) * 2^-53 * mae.  A non-finite NumPy value must be met exactly (inf)
    or by a NaN.
  * angles.  Two evaluation orders of a 3-term dot product differ by at most about 4 * 2^-53 * S, S = |a0 b0| + |a1 b1| +
    |a2 b2| (1 for unit normals); acos moves by at most sqrt(2 * that) rad, the worst case being at |cos| = 1: 1.7e-6
    degrees for S = 1.  NumPy's vectorised arccos and rad2deg add a few ulps relative (8 are allowed).  normal_p95_deg
    is an order statistic of those angles, so it gets the per-angle bound, and the mean gets it on top of its summation bound.
"""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import score_cases as C
from conftest import ROOT, build_native
from raymarch_algo_compare_amd import _native, score_device, scoring

U = 2.0 ** -53
COUNT_FIELDS = ("n_method_hit", "n_reference_hit", "n_co_hit", "n_union", "n_co_hit_core", "n_union_core", "n_nan_depth", "n_nan_angle")
VALUE_FIELDS = ("depth_mae", "depth_rmse", "depth_signed", "depth_p95", "depth_med", "normal_mean_deg", "normal_p95_deg")
u8p = ctypes.POINTER(ctypes.c_uint8)


# ---- the host build ----------------------------------------------------------------------------------------------------

def load_host_lib():
    """tests/native/score_check.cpp built by g++, prototypes declared"""
    L = ctypes.CDLL(build_native("score_check"))
    L.rmsc_band.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, u8p, u8p]
    L.rmsc_band.restype = None
    L.rmsc_score.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p, ctypes.c_void_p, u8p, ctypes.c_int] * 2 + [ctypes.POINTER(_native.RmScoreResult)]
    return L


@pytest.fixture(scope="module")
def lib():
    return load_host_lib()


def result_dict(res):
    return {name: getattr(res, name) for name, _ in _native.RmScoreResult._fields_}


def host_score(lib, method, reference, band_k):
    """rmsc_score as a dict of RmScoreResult's fields"""
    H, W = reference["hit"].shape
    rd, rn, rh, r64 = C.raw_maps(reference)
    md, mn, mh, m64 = C.raw_maps(method)
    ptr = lambda a: None if a is None else a.ctypes.data      # noqa: E731
    res = _native.RmScoreResult()
    rc = lib.rmsc_score(W, H, band_k, ptr(rd), ptr(rn), rh.ctypes.data_as(u8p), r64, ptr(md), ptr(mn), mh.ctypes.data_as(u8p), m64,
                        ctypes.byref(res))
    assert rc == 0, rc      # 2: score_next_rank did not give the sorted sample's next element
    return result_dict(res)


def host_band(lib, hit, k):
    H, W = hit.shape
    band = np.empty((H, W), np.uint8)
    lib.rmsc_band(W, H, k, np.ascontiguousarray(hit, np.uint8).ctypes.data_as(u8p), band.ctypes.data_as(u8p))
    return band


def bits(x):
    return np.float64(x).view(np.uint64)


def same_bits(a, b):
    """bit for bit, a NaN equal to any NaN"""
    return (np.isnan(a) and np.isnan(b)) or bits(a) == bits(b)


# ---- against NumPy -------------------------------------------------------------------------------------------------------

def close(got, want, tol):
    if np.isfinite(want):
        return abs(got - want) <= tol
    return np.isnan(got) if np.isnan(want) else got == want


def check_against_numpy(got, method, reference, band_k, name):
    """the module docstring's rules for one result dict against scoring.py / NumPy"""
    mine, truth = scoring._mask(method["hit"]), scoring._mask(reference["hit"])
    both, either = mine & truth, mine | truth
    core = ~scoring.silhouette_band(truth, band_k) if band_k >= 0 else np.ones_like(truth)
    n = int(both.sum())
    with np.errstate(all="ignore"):
        gap = np.asarray(method["depth"], np.float64)[both] - np.asarray(reference["depth"], np.float64)[both]
        mag = np.abs(gap)
        angle = None
        if "normal" in method and "normal" in reference:
            a, b = np.asarray(method["normal"], np.float64)[both], np.asarray(reference["normal"], np.float64)[both]
            angle = np.rad2deg(np.arccos(np.minimum(np.maximum(np.einsum("ij,ij->i", a, b), -1.0), 1.0)))
            spread = np.abs(a * b).sum(axis=1)
            spread = max(1.0, float(spread[np.isfinite(spread)].max(initial=1.0)))
        want_counts = [int(mine.sum()), int(truth.sum()), n, int(either.sum()), int((both & core).sum()), int((either & core).sum()),
                       int(np.isnan(gap).sum()), 0 if angle is None else int(np.isnan(angle).sum())]
        assert [got[k] for k in COUNT_FIELDS] == want_counts, (name, [got[k] for k in COUNT_FIELDS], want_counts)
        if n == 0:
            assert all(np.isnan(got[k]) for k in VALUE_FIELDS), (name, got)
            return
        want = {"depth_mae": mag.mean(), "depth_rmse": np.sqrt(np.square(gap).mean()), "depth_signed": gap.mean(),
                "depth_p95": np.percentile(mag, 95), "depth_med": np.median(mag)}
        print(f"{name}: n {n} got {[got[k] for k in VALUE_FIELDS]} numpy {want}")
        assert same_bits(got["depth_p95"], want["depth_p95"]), (name, got["depth_p95"], want["depth_p95"])
        assert same_bits(got["depth_med"], want["depth_med"]), (name, got["depth_med"], want["depth_med"])
        rel = 2 * (n - 1) * U
        assert close(got["depth_mae"], want["depth_mae"], rel * want["depth_mae"]), (name, got["depth_mae"], want["depth_mae"])
        assert close(got["depth_rmse"], want["depth_rmse"], rel * want["depth_rmse"]), (name, got["depth_rmse"], want["depth_rmse"])
        assert close(got["depth_signed"], want["depth_signed"], rel * want["depth_mae"]), (name, got["depth_signed"], want["depth_signed"])
        if angle is None:
            assert np.isnan(got["normal_mean_deg"]) and np.isnan(got["normal_p95_deg"]), name
            return
        per_angle = np.degrees(np.sqrt(2.0 * 4.0 * U * spread))
        mean, p95 = angle.mean(), np.percentile(angle, 95)
        print(f"{name}: numpy angles mean {mean!r} p95 {p95!r}, per-angle bound {per_angle:.3g}")
        assert close(got["normal_mean_deg"], mean, per_angle + (rel + 8 * U) * mean), (name, got["normal_mean_deg"], mean)
        assert close(got["normal_p95_deg"], p95, per_angle + 8 * U * p95), (name, got["normal_p95_deg"], p95)


def test_the_case_list_covers_what_it_should():
    names = [c.name for c in C.cases()]
    assert len(names) == len(set(names)) and len(names) >= 80
    shapes = {c.reference["hit"].shape[::-1] for c in C.cases()}
    assert set(C.SHAPES) <= shapes
    assert {c.band_k for c in C.cases()} == set(C.BANDS)
    cohit = {int((scoring._mask(c.method["hit"]) & scoring._mask(c.reference["hit"])).sum()) for c in C.cases()}
    assert set(C.COHIT_COUNTS) <= cohit and 33 * 9 in cohit
    assert {(C.is_fp64(c.method), C.is_fp64(c.reference)) for c in C.cases()} == {(False, False), (False, True), (True, False), (True, True)}
    assert max(c.reference["hit"].size for c in C.cases()) <= 48 * 36


def test_host_build_against_scoring(lib):
    for c in C.cases():
        got = host_score(lib, c.method, c.reference, c.band_k)
        check_against_numpy(got, c.method, c.reference, c.band_k, c.name)


def test_band_equals_silhouette_band(lib):
    seen = 0
    for c in C.cases():
        for k in ([c.band_k] if c.band_k >= 0 else []) + [0, 1, 8]:
            want = scoring.silhouette_band(c.reference["hit"], k)
            got = host_band(lib, c.reference["hit"], k)
            assert np.array_equal(got.astype(bool), want), (c.name, k)
            assert set(np.unique(got)) <= {0, 1}
            seen += bool(want.any() and not want.all())
    assert seen > 50      # bands that are neither empty nor the whole image


def test_special_values(lib):
    by_name = {c.name: c for c in C.cases()}
    run = lambda name: host_score(lib, *by_name[name][1:])      # noqa: E731
    same = run("method = reference")
    assert all(bits(same[k]) == 0 for k in VALUE_FIELDS[:5])      # +0.0, not -0.0
    assert 0.0 <= same["normal_mean_deg"] < 2e-6 and 0.0 <= same["normal_p95_deg"] < 2e-6      # unit normals to rounding only
    minus = run("gaps of -0.0")
    assert minus["n_co_hit"] == 22 and all(minus[k] == 0.0 for k in VALUE_FIELDS[:5]) and bits(minus["depth_p95"]) == 0
    nan = run("NaN depth on a co-hit pixel")
    assert nan["n_nan_depth"] == 1 and all(np.isnan(nan[k]) for k in VALUE_FIELDS[:5]) and np.isfinite(nan["normal_p95_deg"])
    assert all(bits(nan[k]) == bits(np.nan) for k in VALUE_FIELDS[:5])      # the one quiet NaN, whatever the arithmetic left
    off = run("NaN depth on pixels that are not co-hit")
    assert off["n_nan_depth"] == 0 and all(np.isfinite(off[k]) for k in VALUE_FIELDS)
    inf = run("inf - inf")
    assert inf["n_nan_depth"] == 1 and np.isnan(inf["depth_mae"])
    nn = run("NaN normal on a co-hit pixel")
    assert nn["n_nan_angle"] == 1 and np.isnan(nn["normal_mean_deg"]) and np.isnan(nn["normal_p95_deg"]) and np.isfinite(nn["depth_p95"])
    assert run("cosine exactly 1")["normal_p95_deg"] == 0.0 and run("cosine 1 + ulp")["normal_mean_deg"] == 0.0
    assert run("cosine exactly -1")["normal_mean_deg"] == 180.0 and run("cosine -1 - ulp")["normal_p95_deg"] == 180.0
    assert 0.0 < run("cosine 1 - ulp")["normal_mean_deg"] < 2e-6
    none = run("no normals")
    assert np.isnan(none["normal_mean_deg"]) and np.isnan(none["normal_p95_deg"]) and none["n_nan_angle"] == 0
    one, two, ff = run("hit byte 1"), run("hit byte 2"), run("hit byte 255")
    assert all(same_bits(one[k], two[k]) and same_bits(one[k], ff[k]) for k in COUNT_FIELDS + VALUE_FIELDS)
    for k in C.BANDS:      # no band: the core counts are the full counts; a wider band leaves a smaller core
        r = run(f"48x36 band_k {k}")
        if k < 0:
            assert (r["n_co_hit_core"], r["n_union_core"]) == (r["n_co_hit"], r["n_union"])
    cores = [run(f"48x36 band_k {k}")["n_union_core"] for k in C.BANDS]
    assert cores == sorted(cores, reverse=True) and cores[0] > cores[-1]


# ---- the binding and the C ABI before the device ---------------------------------------------------------------------------

def test_records_follow_the_header():
    fields_m = ["depth", "normal", "hit", "fp64"]
    fields_r = list(COUNT_FIELDS + VALUE_FIELDS)
    assert [f[0] for f in _native.RmScoreMaps._fields_] == fields_m and [f[0] for f in _native.RmScoreResult._fields_] == fields_r
    probes = ["sizeof(RmScoreMaps)", "sizeof(RmScoreResult)"] + [f"offsetof(RmScoreMaps, {f})" for f in fields_m] + \
             [f"offsetof(RmScoreResult, {f})" for f in fields_r]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "rm_hip.h"\nint main(void){' + \
          "".join(f'printf("%zu\\n", {p});' for p in probes) + "return 0;}\n"
    with tempfile.TemporaryDirectory() as td:
        c, exe = os.path.join(td, "s.c"), os.path.join(td, "s")
        open(c, "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    want = [ctypes.sizeof(_native.RmScoreMaps), ctypes.sizeof(_native.RmScoreResult)] + \
           [getattr(_native.RmScoreMaps, f).offset for f in fields_m] + [getattr(_native.RmScoreResult, f).offset for f in fields_r]
    assert got == want
    assert "rm_score_captures" in _native.EXPORTS and hasattr(_native.load(), "rm_score_captures")


def test_argument_checks_answer_without_a_device():
    """every host check of rm_score_captures answers with its code and a message, in a fresh process that never called
    rm_init; valid calls -- 1 x 1, no band, no normals -- then need a device"""
    code = (
        "import ctypes, numpy as np\n"
        "from raymarch_algo_compare_amd import _native\n"
        "L = _native.load()\n"
        "def cap(w, h, normal=True):\n"
        "    c = {'depth': np.ones((max(h, 1), max(w, 1)), np.float32), 'hit': np.ones((max(h, 1), max(w, 1)), np.uint8)}\n"
        "    if normal: c['normal'] = np.zeros((max(h, 1), max(w, 1), 3), np.float32)\n"
        "    return _native.score_maps(c, max(w, 1), max(h, 1))\n"
        "out = _native.RmScoreResult()\n"
        "def call(w, h, k, r, m, n, o=out):\n"
        "    rc = L.rm_score_captures(w, h, k, None if r is None else ctypes.byref(r[0]), None if m is None else ctypes.byref(m[0]), n,\n"
        "                             None if o is None else ctypes.byref(o), None)\n"
        "    print(rc, len(L.rm_last_error()))\n"
        "call(8, 8, 2, None, cap(8, 8), 1)\n"
        "call(8, 8, 2, cap(8, 8), None, 1)\n"
        "call(8, 8, 2, cap(8, 8), cap(8, 8), 1, None)\n"
        "nod = cap(8, 8); nod[0].depth = None\n"
        "call(8, 8, 2, cap(8, 8), nod, 1)\n"
        "noh = cap(8, 8); noh[0].hit = None\n"
        "call(8, 8, 2, noh, cap(8, 8), 1)\n"
        "call(8, 8, 2, cap(8, 8), cap(8, 8, normal=False), 1)\n"
        "call(8, 8, 2, cap(8, 8, normal=False), cap(8, 8), 1)\n"
        "call(8, 8, 2, cap(8, 8), cap(8, 8), 0)\n"
        "call(8, 8, 2, cap(8, 8), cap(8, 8), 65536)\n"
        "call(8, 8, 9, cap(8, 8), cap(8, 8), 1)\n"
        "call(0, 8, 2, cap(0, 8), cap(0, 8), 1)\n"
        "call(8, -1, 2, cap(8, -1), cap(8, -1), 1)\n"
        "call(65536, 32768, 2, cap(8, 8), cap(8, 8), 1)\n"
        "call(1, 1, 8, cap(1, 1), cap(1, 1), 1)\n"
        "call(8, 8, -1, cap(8, 8, normal=False), cap(8, 8, normal=False), 1)\n")
    env = dict(os.environ, PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, check=True, capture_output=True, text=True).stdout
    rows = [[int(v) for v in line.split()] for line in out.strip().splitlines()]
    ARG, DIMS, NODEV = _native.RM_E_BAD_ARG, -3, _native.RM_E_NO_DEVICE
    assert [r[0] for r in rows] == [ARG] * 10 + [DIMS] * 3 + [NODEV] * 2, out
    assert all(r[1] > 0 for r in rows), out


# ---- score_device.py around the call ---------------------------------------------------------------------------------------

def test_score_device_reports_have_scoring_keys(lib, monkeypatch):
    """score_capture_batch and residual_batch with the host build standing in for the device call: scoring.py's key sets and
    grouping, counts and percentiles equal, means within the summation bound"""
    calls = []

    def fake(width, height, reference, methods, band_k=2, warmup=0, repeats=0):
        calls.append((width, height, sorted(reference), len(methods), band_k))
        return [host_score(lib, m, reference, band_k) for m in methods]

    monkeypatch.setattr(_native, "score_captures", fake)
    r = C.capture(48, 36, 81, np.float64)
    ms = [C.near(C.capture(48, 36, 81, np.float32), 82), C.near(r, 83), dict(C.near(r, 84), hit=np.zeros((36, 48), np.uint8))]

    def same_keys(a, b, path=""):
        assert list(a) == list(b), (path, list(a), list(b))
        for k in a:
            if isinstance(a[k], dict):
                same_keys(a[k], b[k], f"{path}/{k}")

    reports = score_device.score_capture_batch(ms, r)
    assert calls == [(48, 36, ["depth", "hit", "normal"], 3, -1)]
    for m, rep in zip(ms, reports):
        want = scoring.score_capture(m, r)
        same_keys(want, rep)
        assert rep["primary"] is rep["hit"] and rep["tertiary"] is rep["ssim"] and rep["secondary"]["depth"] is rep["depth"]
        assert rep["hit"] == want["hit"] and rep["ssim"] == want["ssim"] and rep["depth"]["n_pixels"] == want["depth"]["n_pixels"]
        assert type(rep["depth"]["n_pixels"]) is int
        n = want["depth"]["n_pixels"]
        assert same_bits(rep["depth"]["p95"], want["depth"]["p95"])
        for k in ("mae", "rmse"):
            assert close(rep["depth"][k], want["depth"][k], 2 * (n - 1) * U * want["depth"][k] if n else 0.0), (k, rep["depth"], want["depth"])
    no_normal = score_device.score_capture_batch([{k: v for k, v in ms[0].items() if k != "normal"}], r)
    assert calls[-1][2] == ["depth", "hit"] and np.isnan(no_normal[0]["normal"]["mean_deg"])
    assert score_device.score_capture_batch([], r) == [] and score_device.residual_batch([], r) == []

    residuals = score_device.residual_batch(ms, r, k=2)
    assert calls[-1] == (48, 36, ["depth", "hit"], 3, 2)
    band = scoring.silhouette_band(r["hit"], 2)
    for m, got in zip(ms, residuals):
        want = scoring.residual(m["hit"], m["depth"], r["hit"], r["depth"], band)
        assert list(got) == list(want)
        for k in ("iou", "core_iou", "false_hit", "false_miss", "n_analytic_hit", "n_method_hit", "n_co_hit"):
            assert got[k] == want[k] and type(got[k]) is type(want[k]), k
        assert same_bits(got["depth_med"], want["depth_med"]) and same_bits(got["depth_p95"], want["depth_p95"])
    with pytest.raises(ValueError):
        score_device.score_capture_batch([C.capture(8, 8, 1)], C.capture(9, 8, 2))


def test_sweep_device_score_needs_an_oracle():
    from raymarch_algo_compare_amd import sweep
    with pytest.raises(ValueError):
        sweep.run_sweep(["Sphere"], ["Standard"], device_score=True)
    with pytest.raises(SystemExit):
        sweep.main(["--scenes", "Sphere", "--strategies", "Standard", "--device-score"])
