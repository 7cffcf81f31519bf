"""SSIM / colour-RMSE capture scoring on the MI355X (rm_ssim_scores, csrc/rm_ssim.hip): the device against the host build
of the same header (tests/native/ssim_check.cpp) bit for bit, a batch against single calls, two runs against each other,
real captures against the float64 restatement of test_ssim_host.py, and the sweep's --ssim columns.

Host build and device share csrc/rm_ssim.h -- quantisation, per-pixel formula, tile size, the fold of a tile's values and
the index order of the tiles' sums -- so equality of all four outputs is the requirement, not a tolerance."""
import csv

import numpy as np
import pytest

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
