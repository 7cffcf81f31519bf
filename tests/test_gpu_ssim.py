"""SSIM / colour-RMSE capture scoring on the MI355X (rm_ssim_scores, csrc/rm_ssim.hip): the device against the host build
of the same header (tests/native/ssim_check.cpp) bit for bit, a batch against single calls, two runs against each other,
real captures against the float64 restatement of test_ssim_host.py, and the sweep's --ssim columns.  The inputs are the
well-behaved captures of test_ssim_host.capture(), the reference-made fixture (tests/golden/ssim_images.npz) and the edge
inputs of tests/ssim_edge_cases.py: rounding edges of x * 255, non-finite colours, normals and hit depths, one hit, one
depth, checkerboards, and captures one pixel apart at the tile seams.

Host build and device share csrc/rm_ssim.h -- quantisation, per-pixel formula, tile size, the fold of a tile's values and
the index order of the tiles' sums -- so equality of all four outputs is the requirement, not a tolerance."""
import csv
import ctypes
import math

import numpy as np
import pytest

import ssim_edge_cases as E
import test_ssim_host as H
from raymarch_algo_compare_amd import registry, scoring, ssim, sweep
from raymarch_algo_compare_amd.config import MarchConfig, RenderConfig
from raymarch_algo_compare_amd.runner import GPURunner

pytestmark = pytest.mark.gpu

TILE_W, TILE_H = 32, 8      # kSsimTileW, kSsimTileH of csrc/rm_ssim.h: a tile's output pixels (its windows reach 6 further)
# (W, H): one window; barely more; several tiles; no multiple of the tile; exactly one tile plus one pixel each way
SHAPES = [(7, 7), (8, 9), (64, 48), (100, 37), (TILE_W + 6 + 1, TILE_H + 6 + 1)]


@pytest.fixture(scope="module")
def lib():
    return H.load_host_lib()


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64).tolist()


def device(hip, methods, reference):
    h, w = np.shape(reference["hit"])
    return hip.ssim_scores(w, h, reference, methods)


@pytest.mark.parametrize("W,Hh", SHAPES)
def test_device_equals_the_host_build(hip, lib, W, Hh):
    ref = H.capture(W, Hh, 21)
    cases = [("noisy", H.capture(W, Hh, 22), ref), ("itself", ref, ref),
             ("all-miss reference", H.capture(W, Hh, 23), H.capture(W, Hh, 24, all_miss=True)),
             ("no colour", H.capture(W, Hh, 25, color=False), H.capture(W, Hh, 26, color=False)),
             ("depth only", H.capture(W, Hh, 27, color=False, normal=False), H.capture(W, Hh, 28, color=False, normal=False))]
    for name, m, r in cases:
        got, want = device(hip, [m], r)[0], H.host_scores(lib, m, r)
        print(f"{W}x{Hh} {name}: device {list(got)} host {list(want)}")
        assert bits(got) == bits(want), name
    assert list(device(hip, [ref], ref)[0]) == [1.0, 1.0, 1.0, 0.0]


# ---- non-finite and edge inputs (ssim_edge_cases.py, tests/golden/ssim_images.npz) --------------------------------------------

def assert_device_equals_host(hip, lib, name, m, r):
    got, want = device(hip, [m], r)[0], H.host_scores(lib, m, r)
    print(f"{np.shape(r['hit'])[::-1]} {name}: device {list(got)} host {list(want)}")
    assert bits(got) == bits(want), name
    return got


def test_golden_captures_on_the_device(hip, lib):
    """every case of the reference-made fixture as a method against every case of its shape as the reference, itself
    included: NaN, +-inf and +-3.4e38 hit depths, degenerate normals, one hit, one depth"""
    by_shape = {}
    for i, g in H.golden_cases():
        by_shape.setdefault(g["hit"].shape, []).append((i, H.golden_capture(g)))
    assert sorted(len(v) for v in by_shape.values()) == [2, 10]
    for group in by_shape.values():
        for j, r in group:
            for i, m in group:
                assert_device_equals_host(hip, lib, f"c{i} against c{j}", m, r)


@pytest.mark.parametrize("W,Hh", E.SHAPES)
def test_edge_captures_on_the_device(hip, lib, W, Hh):
    for name, m, r in E.edge_pairs(W, Hh):
        assert_device_equals_host(hip, lib, name, m, r)


@pytest.mark.parametrize("W,Hh", E.SHAPES)
def test_contrast_pairs_on_the_device(hip, lib, W, Hh):
    for name, m, r, ab in E.contrast_pairs(W, Hh):
        got = assert_device_equals_host(hip, lib, name, m, r)
        if ab is None:
            assert H.period_1_is_negative(name, got), (name, got)
        else:
            a, b = ab
            closed = (2.0 * a * b + H.C1) / (a * a + b * b + H.C1)
            assert abs(got[1] - closed) <= 1e-12 and abs(got[2] - closed) <= 1e-12, (name, got, closed)
            assert got[0] == 1.0 and got[3] == abs(a - b), (name, got)


@pytest.mark.parametrize("W,Hh", [(2 * TILE_W + 6, 2 * TILE_H + 6), (45, 21)])
def test_one_pixel_is_counted_exactly_once_on_the_device(hip, lib, W, Hh):
    pairs = E.one_hot_pairs(W, Hh)
    assert len(pairs) >= 30
    for name, m, r, d in pairs:
        got = assert_device_equals_host(hip, lib, name, m, r)
        want = math.sqrt(d * d / (3 * W * Hh))
        assert abs(got[3] - want) <= np.spacing(want), (name, got[3], want)


def mixed_batch(W, Hh):
    """(five methods of different classes, their reference)"""
    ref = E.edge_capture(W, Hh, 71, nan=None, posinf=False, neginf=False, huge=False)
    return [H.capture(W, Hh, 72), E.require_classes(E.edge_capture(W, Hh, 73)), E.edge_capture(W, Hh, 74, all_miss=True),
            E.edge_capture(W, Hh, 75, one_hit=True), E.edge_capture(W, Hh, 76, equal_depth=True)], ref


def test_a_mixed_batch_equals_single_calls(hip, lib):
    ms, ref = mixed_batch(100, 37)
    batch = device(hip, ms, ref)
    assert batch.shape == (5, 4)
    for i, m in enumerate(ms):
        assert bits(device(hip, [m], ref)[0]) == bits(batch[i]) == bits(H.host_scores(lib, m, ref)), i
    assert bits(device(hip, ms[::-1], ref)[::-1]) == bits(batch)
    nan_ref = E.edge_capture(100, 37, 77)                              # a NaN depth at a late hit of the reference
    batch = device(hip, ms, nan_ref)
    for i, m in enumerate(ms):
        assert bits(batch[i]) == bits(H.host_scores(lib, m, nan_ref)), i


def test_the_workspace_is_reused_across_shapes(hip, lib):
    ms, ref = mixed_batch(100, 37)
    first = device(hip, ms, ref)
    small_m, small_r = E.edge_capture(7, 7, 78, color=False, normal=False), E.edge_capture(7, 7, 79, color=False, normal=False)
    small = device(hip, [small_m], small_r)
    assert small.shape == (1, 4) and bits(small[0]) == bits(H.host_scores(lib, small_m, small_r))
    assert bits(device(hip, ms, ref)) == bits(first)
    for i, m in enumerate(ms):
        assert bits(first[i]) == bits(H.host_scores(lib, m, ref)), i


def test_the_timed_call_gives_the_same_bits(hip):
    ms, ref = mixed_batch(100, 37)
    plain = device(hip, ms, ref)
    timed, tm = hip.ssim_scores(100, 37, ref, ms, warmup=1, repeats=2)
    assert bits(timed) == bits(plain)
    assert tm["repeats"] == 2 and len(tm["ms_each"]) == 2 and np.isfinite(tm["ms_each"]).all()


def test_any_non_zero_hit_byte_is_a_hit_on_the_device(hip):
    """rm_ssim_scores itself, with hit maps that hold 1, 2 or 255 for a hit (hip.capture_maps would write 1)"""
    W, Hh = 40, 33
    L = hip.init()
    for name, m, r in E.edge_pairs(W, Hh)[:4]:
        rows = []
        for byte in (1, 2, 255):
            keep, recs = [], []
            for c in (r, m):
                rec, k = hip.capture_maps(c, W, Hh)
                raw = np.ascontiguousarray((np.asarray(c["hit"]) != 0) * np.uint8(byte), np.uint8)
                rec.hit = raw.ctypes.data
                keep += [k, raw]
                recs.append(rec)
            out = np.empty(4)
            hip.check(L.rm_ssim_scores(W, Hh, ctypes.byref(recs[0]), ctypes.byref(recs[1]), 1,
                                       out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), None))
            rows.append(bits(out))
        assert rows[0] == rows[1] == rows[2] == bits(device(hip, [m], r)[0]), name


def test_batch_equals_single_calls_and_runs_repeat(hip):
    W, Hh = 100, 37
    ref = H.capture(W, Hh, 31)
    ms = [H.capture(W, Hh, 32), ref, H.capture(W, Hh, 33, all_miss=True)]
    batch = device(hip, ms, ref)
    assert batch.shape == (3, 4)
    for i, m in enumerate(ms):
        assert bits(device(hip, [m], ref)[0]) == bits(batch[i]), i
    assert bits(device(hip, ms, ref)) == bits(batch)                    # the same call twice
    assert bits(device(hip, ms[::-1], ref)[::-1]) == bits(batch)        # a method's place in the batch does not matter


def test_real_captures_against_the_restatement(hip):
    mc, runner = MarchConfig(), GPURunner()
    for name in ("Sphere", "Thin Torus"):
        sc = registry.get_scene_by_name(name)
        rc = RenderConfig(width=96, height=72, camera_position=sc.camera_position or (0.0, 0.0, 5.0),
                          camera_target=sc.camera_target or (0.0, 0.0, 0.0))
        std = runner.capture(sc.id, 0, rc, mc)
        dense = runner.capture(sc.id, 9, rc, mc)
        assert std["hit"].any(), name
        got, want = ssim.ssim_scores(std, dense), H.oracle_scores(std, dense)
        print(f"{name}: device {got} restatement {want}")
        for k, w in zip(scoring.SSIM_KEYS, want):
            assert abs(got[k] - w) <= H.TOL, (name, k, got[k], w)
        assert ssim.ssim_scores(std, std) == {"depth_ssim": 1.0, "normal_ssim": 1.0, "color_ssim": 1.0, "color_rmse": 0.0}, name
        full = ssim.score_capture_full(std, dense)
        assert full["tertiary"] == got and full["primary"] == scoring.score_capture(std, dense)["primary"]


def test_sweep_ssim_columns(hip, tmp_path):
    args = ["--scenes", "Sphere", "--strategies", "Standard,Enhanced", "--budgets", "32,64", "--width", "48", "--height", "36",
            "--oracle", "interval"]
    plain, with_ssim = str(tmp_path / "plain.csv"), str(tmp_path / "ssim.csv")
    assert sweep.main(args + ["--out", plain]) == 0
    assert sweep.main(args + ["--ssim", "--out", with_ssim]) == 0
    a = list(csv.reader(open(plain, encoding="utf-8")))
    b = list(csv.reader(open(with_ssim, encoding="utf-8")))
    assert a[0] == sweep.ROW_FIELDS + sweep.ORACLE_FIELDS                # today's header
    assert b[0] == a[0] + list(scoring.SSIM_KEYS) and len(a) == len(b) > 1
    timing = a[0].index("ms_per_frame")
    for ra, rb in zip(a[1:], b[1:]):
        assert [v for i, v in enumerate(ra) if i != timing] == [v for i, v in enumerate(rb[:len(ra)]) if i != timing]
        d, n, c, e = rb[len(ra):]
        assert -1.0 <= float(d) <= 1.0 and -1.0 <= float(n) <= 1.0 and np.isfinite([float(d), float(n)]).all()
        assert c == "" and e == ""                                       # the oracle capture carries no colour
