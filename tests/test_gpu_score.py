"""Capture scoring on the MI355X (rm_score_captures, csrc/rm_score.hip): the device against the host build of the same header
(tests/native/score_check.cpp) bit for bit on every case of tests/score_cases.py, a batch against single calls, two runs and
a timed run against each other, real captures against scoring.py under the rules of tests/test_score_host.py, and the
sweep's --device-score columns.

Host build and device share csrc/rm_score.h -- the per-pixel values, the band, the rank rules, the tile size, the fold of a
tile's values, the index order of the tiles' sums and the one NaN every NaN output becomes -- so equality of every field is
the requirement, not a tolerance."""
import csv

import numpy as np
import pytest

import score_cases as C
import test_score_host as H
from raymarch_algo_compare_amd import interval_oracle, registry, score_device, scoring, sweep
from raymarch_algo_compare_amd.config import MarchConfig, RenderConfig
from raymarch_algo_compare_amd.runner import GPURunner
from raymarch_algo_compare_amd.viewpoints import viewpoints_for

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def lib():
    return H.load_host_lib()


def bits(result):
    """a result dict as integers: the counts, and the bit patterns of the doubles"""
    return [result[k] for k in H.COUNT_FIELDS] + [int(H.bits(result[k])) for k in H.VALUE_FIELDS]


def device(hip, methods, reference, band_k, **kw):
    h, w = reference["hit"].shape
    return hip.score_captures(w, h, reference, methods, band_k=band_k, **kw)


def test_device_equals_the_host_build_on_every_case(hip, lib):
    for c in C.cases():
        got, want = device(hip, [c.method], c.reference, c.band_k)[0], H.host_score(lib, c.method, c.reference, c.band_k)
        print(f"{c.name}: device {got}")
        assert bits(got) == bits(want), (c.name, got, want)


def batch_of_11():
    """eleven 48 x 36 methods of different kinds against one reference: float32 and float64, few and many co-hit pixels,
    none, NaN and infinite depths"""
    r = C.capture(48, 36, 91, np.float64)
    ms = [C.near(C.capture(48, 36, 91, np.float32), 92 + i) for i in range(4)] + [C.near(r, 100 + i, scale=0.3) for i in range(3)]
    ms.append(dict(C.near(r, 110), hit=np.zeros((36, 48), np.uint8)))
    few = C.near(r, 111)
    few["hit"] = few["hit"] * (np.arange(36 * 48).reshape(36, 48) % 53 == 0).astype(np.uint8)
    ms.append(few)
    nan = C.near(r, 112)
    nan["depth"][tuple(np.argwhere(nan["hit"] & r["hit"])[7])] = np.nan
    ms.append(nan)
    inf = C.near(r, 113)
    inf["depth"][10:12, 20:30] = np.inf
    ms.append(inf)
    assert len(ms) == 11
    return ms, r


def test_a_method_scores_the_same_alone_and_in_a_batch(hip, lib):
    ms, r = batch_of_11()
    batch = device(hip, ms, r, 2)
    assert len(batch) == 11
    for i, m in enumerate(ms):
        assert bits(device(hip, [m], r, 2)[0]) == bits(batch[i]) == bits(H.host_score(lib, m, r, 2)), i
    back = device(hip, ms[::-1], r, 2)[::-1]
    assert [bits(b) for b in back] == [bits(b) for b in batch]      # a method's place in the batch does not matter
    assert sum(b["n_co_hit"] == 0 for b in batch) == 1 and sum(b["n_nan_depth"] > 0 for b in batch) >= 1


def test_two_runs_and_a_timed_run_give_the_same_bits(hip):
    ms, r = batch_of_11()
    first = device(hip, ms, r, 2)
    small = C.cases()[0]                                                # another shape in between: the workspace is reused
    device(hip, [small.method], small.reference, small.band_k)
    again = device(hip, ms, r, 2)
    timed, tm = device(hip, ms, r, 2, warmup=1, repeats=2)
    assert [bits(b) for b in first] == [bits(b) for b in again] == [bits(b) for b in timed]
    assert tm["repeats"] == 2 and len(tm["ms_each"]) == 2 and np.isfinite(tm["ms_each"]).all()


def test_real_captures_against_scoring(hip):
    """each scene from its closest curated viewpoint (the thin torus is below a pixel from the others at 48 x 36)"""
    mc, runner = MarchConfig(), GPURunner()
    scored = []
    for name in ("Sphere", "Thin Torus", "Thin Planes Stack"):
        sc = registry.get_scene_by_name(name)
        vp = viewpoints_for(sc)[-1]
        assert tuple(vp.up) == (0.0, 1.0, 0.0)
        rc = RenderConfig(width=48, height=36, camera_position=vp.position, camera_target=vp.target)
        truth = interval_oracle.interval_capture(sc, rc)
        assert truth is not None, name
        methods = [runner.capture(sc.id, registry.STRATEGIES[key], rc, mc, device=dev)
                   for key in ("Standard", "Relaxed") for dev in (False, True)]
        reports = score_device.score_capture_batch(methods, truth)
        residuals = score_device.residual_batch(methods, truth, k=2)
        band = scoring.silhouette_band(truth["hit"], 2)
        raw = device(hip, methods, truth, 2)
        for i, (m, rep, res) in enumerate(zip(methods, reports, residuals)):
            H.check_against_numpy(raw[i], m, truth, 2, f"{name} method {i}")
            want = scoring.score_capture(m, truth)
            n = want["depth"]["n_pixels"]
            scored.append(n)
            assert rep["hit"] == want["hit"] and rep["depth"]["n_pixels"] == n, (name, i)
            assert H.same_bits(rep["depth"]["p95"], want["depth"]["p95"]), (name, i)
            rel = 2 * (n - 1) * H.U
            for k in ("mae", "rmse"):
                assert H.close(rep["depth"][k], want["depth"][k], rel * want["depth"][k]), (name, i, k, rep["depth"], want["depth"])
            assert list(rep["normal"]) == ["mean_deg", "p95_deg"]      # the values: raw's, checked above
            assert H.same_bits(rep["normal"]["mean_deg"], raw[i]["normal_mean_deg"]) and H.same_bits(rep["normal"]["p95_deg"], raw[i]["normal_p95_deg"])
            wres = scoring.residual(m["hit"], m["depth"], truth["hit"], truth["depth"], band)
            assert list(res) == list(wres)
            for k in ("iou", "core_iou", "false_hit", "false_miss", "n_analytic_hit", "n_method_hit", "n_co_hit"):
                assert res[k] == wres[k], (name, i, k)
            assert H.same_bits(res["depth_med"], wres["depth_med"]) and H.same_bits(res["depth_p95"], wres["depth_p95"]), (name, i)
            assert H.close(res["depth_rmse"], wres["depth_rmse"], rel * wres["depth_rmse"]), (name, i)
            assert H.close(res["depth_signed"], wres["depth_signed"], rel * want["depth"]["mae"]), (name, i)
    assert len(scored) == 12 and sum(n > 0 for n in scored) >= 8, scored      # at least two of the scenes have co-hit pixels


def test_sweep_device_score_columns(hip, tmp_path):
    args = ["--scenes", "Sphere", "--strategies", "Standard,Enhanced", "--budgets", "32,64", "--width", "48", "--height", "36",
            "--oracle", "interval", "--ceiling", "segment"]
    host, dev = str(tmp_path / "host.csv"), str(tmp_path / "device.csv")
    assert sweep.main(args + ["--out", host]) == 0
    assert sweep.main(args + ["--device-score", "--out", dev]) == 0
    a = list(csv.DictReader(open(host, encoding="utf-8")))
    b = list(csv.DictReader(open(dev, encoding="utf-8")))
    assert len(a) == len(b) > 1 and list(a[0]) == list(b[0]) == sweep.ROW_FIELDS + sweep.ORACLE_FIELDS + sweep.CEILING_FIELDS
    means = ("oracle_depth_mae", "oracle_depth_rmse")
    for ra, rb in zip(a, b):
        for k in ra:
            if k == "ms_per_frame":
                continue
            if k in means:      # summation order only: 2 (n - 1) * 2^-53 relative with n <= 48 * 36 co-hit pixels
                assert H.close(float(rb[k]), float(ra[k]), 2 * (48 * 36 - 1) * H.U * float(ra[k])), (k, ra[k], rb[k])
            else:               # count-derived and percentile columns, the ceiling's included
                assert ra[k] == rb[k], (k, ra[k], rb[k])
        assert ra["oracle_iou"] != "" and ra["ceiling_iou"] != ""
