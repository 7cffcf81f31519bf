"""The discovery features (csrc/rm_features.h, features.py) without a GPU: the header compiled for the host by g++
(tests/native/features_check.cpp) over the CPU oracle's point evaluation against the reference's recorded results bit for
bit, the run detection on synthetic sign patterns, the two order statistics against NumPy, the view features against
features.view_features_numpy on hand-made captures, the binding of the new records, every refusal of the two calls before
the device, the sweep's new option before the device, and the features.o code object.  tests/test_gpu_features.py gives
the device the same inputs and asks for the same bits."""
import ctypes
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import features_cases as C
from conftest import ROOT
from features_edge_cases import numpy_runs, sign_patterns
from oracle import oracle
from raymarch_algo_compare_amd import _native, features, sweep

CASES = C.fixture_cases()


@pytest.fixture(scope="module")
def host():
    return C.Host()


# ---- 1. the fixture --------------------------------------------------------------------------------------------------------

def test_the_fixture_holds_what_it_should():
    by_scene = {}
    for label, c in CASES:
        by_scene.setdefault(c["scene"], []).append(c)
        assert c["steps"] == features._CHORD_STEPS == 160 and c["set"]["pts"].shape == (c["n_lip"], 3)
        assert c["set"]["chords"].shape == (c["n_chords"], 6) and c["set"]["seglen"].shape == (c["n_chords"],)
    assert sorted(by_scene) == list(range(20))
    full = {c["scene"] for _, c in CASES if (c["n_lip"], c["n_chords"]) == (features._LIP_SAMPLES, features._CHORDS)}
    assert full == {0, 3, 10}                                                    # Sphere, Thin Torus, Mandelbulb
    small_box = {c["scene"] for _, c in CASES if c["box"][1, 0] == 0.4}
    assert small_box == {8, 13}                                                  # Onion Shell, Thin Planes Stack
    assert os.path.getsize(os.path.join(C.GOLDEN, "features_intrinsic.npz")) < 1_000_000


@pytest.mark.parametrize("label,case", CASES, ids=[c[0] for c in CASES])
def test_sample_sets_draws_what_the_reference_drew(label, case):
    """the recorded samples are the seed's draws in the reference's order (the generator asserted that they reproduce the
    reference's results), so sample_sets must give them again"""
    lo, hi, diag = features.padded_box(case["box"][0], case["box"][1])
    s = features.sample_sets(lo, hi, np.random.default_rng(case["seed"]), case["n_lip"], case["n_chords"], case["steps"])
    assert C.bits(diag)[0] == C.bits(case["diag"])[0]
    for k in ("pts", "chords", "seglen", "ts"):
        assert np.array_equal(C.bits(s[k]), C.bits(case["set"][k])), (label, k)


@pytest.mark.parametrize("label,case", CASES, ids=[c[0] for c in CASES])
def test_host_build_matches_the_reference_bit_for_bit(host, label, case):
    xyz = host.points([case["set"]])
    res, gmag, counts = host.intrinsic([case["set"]], oracle.sdf_eval(case["scene"], xyz))[0]
    C.check_case(case, res, gmag, counts, label)


def test_numpy_statement_matches_the_reference_bit_for_bit():
    for label, case in CASES[:20:3]:
        r = features.intrinsic_features_numpy(case["scene"], [case["set"]], sdf=lambda p: oracle.sdf_eval(case["scene"], p))[0]
        C.check_case(case, r, r["gmag"], r["slab_counts"], label)


def test_points_are_numpy_s(host):
    """p + e and p - e with e = +0.0 off the axis (the sum turns -0.0 into +0.0, the difference keeps it); chord samples
    a + ts * (b - a), unfused"""
    s = {k: v.copy() for k, v in CASES[0][1]["set"].items()}
    s["pts"][0] = [-0.0, 0.0, -0.0]
    s["pts"][1] = [1.0, -0.0, 1e-300]
    xyz = host.points([s, s])
    n_lip, n_chords, steps = len(s["pts"]), len(s["chords"]), len(s["ts"])
    want = []
    for ax in range(3):
        e = np.zeros(3)
        e[ax] = C.EPS
        want += [s["pts"] + e, s["pts"] - e]
    want = np.stack(want, axis=1).reshape(-1, 3)                                 # (sample, k = 2 * axis + minus)
    seg = (s["chords"][:, None, :3] + s["ts"][None, :, None] * (s["chords"][:, 3:] - s["chords"][:, :3])[:, None, :]).reshape(-1, 3)
    assert len(xyz) == 2 * (6 * n_lip + n_chords * steps)
    assert np.array_equal(C.bits(xyz[:6 * n_lip]), C.bits(want)) and np.array_equal(C.bits(xyz[6 * n_lip:12 * n_lip]), C.bits(want))
    assert np.array_equal(C.bits(xyz[12 * n_lip:12 * n_lip + n_chords * steps]), C.bits(seg))
    assert np.array_equal(C.bits(xyz[12 * n_lip + n_chords * steps:]), C.bits(seg))
    assert C.bits(xyz[0, 0])[0] == C.bits(C.EPS)[0] and C.bits(xyz[1, 2])[0] == 1 << 63 and C.bits(xyz[0, 2])[0] == 0


# ---- 2. run detection --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("steps", [2, 3, 63, 64, 65, 127, 128, 129, 160, 1023, 1024])
def test_runs_on_sign_patterns(host, steps):
    seglen = 2.718281828
    for name, inside in sign_patterns(steps):
        want = numpy_runs(inside, seglen)
        for by_lanes in (False, True):
            got = host.runs(inside, seglen, by_lanes)
            assert np.array_equal(C.bits(got), C.bits(want)), (steps, name, by_lanes, got, want)
        assert len(want) <= (steps + 1) // 2


# ---- 3. the order statistics ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 3, 100, 101, 1500])
def test_p99_and_median_are_numpy_s(host, n):
    rng = np.random.default_rng(n)
    samples = [rng.random(n) * 3.0, np.round(rng.random(n) * 4.0) / 4.0, np.full(n, 0.75), np.sort(rng.random(n))[::-1].copy(),
               np.r_[np.zeros(n // 2), rng.random(n - n // 2) * 1e-300]]
    for x in samples:
        assert C.bits(host.select(0, x))[0] == C.bits(np.percentile(x, 99))[0], (n, host.select(0, x), np.percentile(x, 99))
        assert C.bits(host.select(1, x))[0] == C.bits(np.median(x))[0], (n, host.select(1, x), np.median(x))
    assert C.bits(host.select(0, np.empty(0)))[0] == C.NAN_BITS and C.bits(host.select(1, np.empty(0)))[0] == C.NAN_BITS


def test_empty_and_non_finite_samples(host):
    s = CASES[0][1]["set"]
    xyz = host.points([s])
    f = oracle.sdf_eval(0, xyz)
    n_lip = len(s["pts"])
    f[0], f[6 + 3], f[12] = np.nan, np.inf, -np.inf                             # three samples leave
    f[6 * n_lip:] = 1.0                                                          # no chord sample is inside
    res, gmag, counts = host.intrinsic([s], f)[0]
    assert res["n_finite"] == n_lip - 3 and np.isnan(gmag[:3]).all() and np.isfinite(gmag[3:]).all()
    assert all(C.bits(g)[0] == C.NAN_BITS for g in gmag[:3])
    assert res["n_slabs"] == 0 and C.bits(res["slab_median"])[0] == C.NAN_BITS and not counts.any()
    assert C.bits(res["lipschitz_p99"])[0] == C.bits(np.percentile(gmag[3:], 99))[0]
    f[6 * n_lip:] = np.nan                                                       # a NaN is outside
    assert host.intrinsic([s], f)[0][0]["n_slabs"] == 0
    empty = {"pts": np.empty((0, 3)), "chords": np.empty((0, 6)), "seglen": np.empty(0), "ts": s["ts"]}
    res = host.intrinsic([empty], np.empty(0))[0][0]
    assert (res["n_finite"], res["n_slabs"]) == (0, 0)
    assert C.bits(res["lipschitz_p99"])[0] == C.NAN_BITS and C.bits(res["slab_median"])[0] == C.NAN_BITS


def test_sets_of_a_batch_are_independent(host):
    sets = [CASES[i][1]["set"] for i in (0, 2, 4)]                               # three scenes' samples, one shape
    xyz = host.points(sets)
    f = oracle.sdf_eval(7, xyz)
    batch = host.intrinsic(sets, f)
    for s, (res, gmag, counts) in zip(sets, batch):
        one, g1, c1 = host.intrinsic([s], oracle.sdf_eval(7, host.points([s])))[0]
        assert all(C.bits(res[k])[0] == C.bits(one[k])[0] for k in ("lipschitz_p99", "slab_median"))
        assert (res["n_finite"], res["n_slabs"]) == (one["n_finite"], one["n_slabs"])
        assert np.array_equal(C.bits(gmag), C.bits(g1)) and np.array_equal(counts, c1)


# ---- 4. the view features ------------------------------------------------------------------------------------------------------

VIEW_CASES = C.view_cases()


@pytest.mark.parametrize("label,capture,cam", VIEW_CASES, ids=[v[0] for v in VIEW_CASES])
def test_view_features_against_numpy(host, label, capture, cam):
    got = host.view(capture, cam.params14())
    want = features.view_features_numpy(capture, cam)
    print(label, got, want)
    C.check_view_against_numpy(got, want, label)


def test_view_feature_values_by_hand(host):
    cam = C.camera(16, 12)
    hit = np.zeros((12, 16), bool)
    hit[2:7, 3:9] = True                                                         # 5 x 6: 30 hits, 12 interior, 18 on the rim
    cap = C.capture_of(hit, 5)
    cap["evals"][hit] = 7.0
    got = host.view(cap, cam.params14())
    assert (got["n_hit"], got["n_perimeter"], got["sum_evals"]) == (30, 18, 210)
    assert got["hit_rate"] == 30 / 192 and got["silhouette_cplx"] == 18 / np.sqrt(30.0)
    assert got["hardness_mean"] == 7.0 and got["hardness_cv"] == 0.0
    full = C.capture_of(np.ones((12, 16), bool), 6)
    assert host.view(full, cam.params14())["n_perimeter"] == 2 * 16 + 2 * 12 - 4   # the image edge counts as a non-hit
    full["evals"][:] = 0.0
    zero = host.view(full, cam.params14())
    assert zero["hardness_mean"] == 0.0 and zero["hardness_cv"] == 0.0           # a mean of 0: no division
    nn = np.zeros((12, 16, 3), np.float32)
    nn[..., 0] = 1.0                                                             # normal +x: the cosine is the ray's x
    full["normal"] = nn
    from raymarch_algo_compare_amd.runner import ray_directions
    assert host.view(full, cam.params14())["n_grazing"] == int((np.abs(ray_directions(cam)[..., 0]) < features.GRAZING_COS).sum())


# ---- 5. the binding and the C ABI before the device --------------------------------------------------------------------------

def test_records_follow_the_header():
    records = {"RmIntrinsicFeatures": ["lipschitz_p99", "slab_median", "n_finite", "n_slabs"],
               "RmViewMaps": ["depth", "normal", "evals", "hit"],
               "RmViewFeatures": list(C.COUNT_KEYS + C.VALUE_KEYS) + ["box_lo", "box_hi"]}
    probes, want = [], []
    for name, fields in records.items():
        rec = getattr(_native, name)
        assert [f[0] for f in rec._fields_] == fields
        probes += [f"sizeof({name})"] + [f"offsetof({name}, {f})" for f in fields]
        want += [ctypes.sizeof(rec)] + [getattr(rec, f).offset for f in fields]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "rm_hip.h"\nint main(void){' + \
          "".join(f'printf("%zu\\n", {p});' for p in probes) + "return 0;}\n"
    with tempfile.TemporaryDirectory() as td:
        c, exe = os.path.join(td, "s.c"), os.path.join(td, "s")
        open(c, "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == want
    lib = _native.load()
    assert all(n in _native.EXPORTS and hasattr(lib, n) for n in ("rm_intrinsic_features", "rm_view_features"))


def test_limits_are_the_header_s(host):
    ok = dict(nsets=1, n_lip=4, pts=1, eps=1e-4, n_chords=2, chords=1, seglen=1, steps=160, ts=1, out=1)

    def why(**kw):
        a = dict(ok, **kw)
        return host.L.rmft_check_intrinsic(a["nsets"], a["n_lip"], a["pts"], a["eps"], a["n_chords"], a["chords"], a["seglen"], a["steps"],
                                           a["ts"], a["out"])
    assert why() is None
    for good in (dict(nsets=256), dict(n_lip=65536), dict(n_chords=4096), dict(steps=2), dict(steps=1024), dict(n_lip=0, pts=None),
                 dict(n_chords=0, chords=None, seglen=None)):
        assert why(**good) is None, good
    for bad in (dict(nsets=0), dict(nsets=257), dict(n_lip=-1), dict(n_lip=65537), dict(n_chords=-1), dict(n_chords=4097), dict(steps=1),
                dict(steps=1025), dict(eps=0.0), dict(eps=-1e-4), dict(eps=float("nan")), dict(eps=float("inf")), dict(pts=None),
                dict(chords=None), dict(seglen=None), dict(ts=None), dict(out=None)):
        assert why(**bad), bad

    # the lengths, which the call checks once the arguments above are in order (feat_check_seglen): NaN or a set sign bit is
    # refused and the element named; +inf, 0 and a subnormal are lengths
    def lengths(nsets, n_chords, i=0, v=1.0, n=None):
        a = np.ones(nsets * n_chords if n is None else n)
        a[i] = v
        return host.L.rmft_check_seglen(nsets, n_chords, a.ctypes.data)
    for v in (1.0, np.inf, 0.0, 5e-324, 1e308):
        assert lengths(1, 2, 1, v) is None, v
    for i, v in ((0, np.nan), (1, -1.0), (1, -0.0), (0, -np.inf), (1, -np.nan), (0, -5e-324)):
        assert lengths(1, 2, i, v) == f"seglen[{i}] is NaN or negative".encode(), (i, v)
    assert lengths(3, 5, 14, np.nan) == b"seglen[14] is NaN or negative"
    assert lengths(256, 4096, 256 * 4096 - 1, -1.0) == f"seglen[{256 * 4096 - 1}] is NaN or negative".encode()
    assert lengths(3, 4, 14, np.nan, n=15) is None                               # beyond nsets x n_chords: not read
    assert lengths(1, 0, 0, np.nan, n=1) is None and host.L.rmft_check_seglen(1, 0, None) is None      # no chord: no length


def test_argument_checks_answer_without_a_device():
    """every host check of the two calls answers with its code and a message, in a fresh process that never called
    rm_init; valid calls -- n_lip = 0 and n_chords = 0 among them -- then need a device"""
    code = (
        "import ctypes, numpy as np\n"
        "from raymarch_algo_compare_amd import _native\n"
        "L = _native.load(); dp = ctypes.POINTER(ctypes.c_double)\n"
        "pts, chords, seglen, ts = np.zeros((2, 4, 3)), np.ones((2, 3, 6)), np.ones((2, 3)), np.linspace(0.0, 1.0, 160)\n"
        "out = (_native.RmIntrinsicFeatures * 2)()\n"
        "P = lambda a: None if a is None else a.ctypes.data_as(dp)\n"
        "def intr(scene=0, nsets=2, n_lip=4, pts=pts, eps=1e-4, n_chords=3, chords=chords, seglen=seglen, steps=160, ts=ts, out=out):\n"
        "    rc = L.rm_intrinsic_features(scene, nsets, n_lip, P(pts), eps, n_chords, P(chords), P(seglen), steps, P(ts), out, None, None, None)\n"
        "    print(rc, len(L.rm_last_error()))\n"
        "for kw in (dict(nsets=0), dict(nsets=257), dict(n_lip=-1), dict(n_lip=65537), dict(n_chords=-1), dict(n_chords=4097), dict(steps=1),\n"
        "           dict(steps=1025), dict(eps=0.0), dict(eps=-1.0), dict(eps=float('nan')), dict(eps=float('inf')), dict(pts=None),\n"
        "           dict(chords=None), dict(seglen=None), dict(ts=None), dict(out=None)):\n"
        "    intr(**kw)\n"
        "intr(scene=20); intr(scene=-1); intr(scene=_native.RM_SCENE_PROGRAM_BASE + 5)\n"
        "intr(); intr(n_lip=0, pts=None); intr(n_chords=0, chords=None, seglen=None)\n"
        "cap = {'depth': np.ones((6, 8), np.float32), 'normal': np.zeros((6, 8, 3), np.float32), 'evals': np.ones((6, 8), np.float32),\n"
        "       'hit': np.ones((6, 8), np.uint8)}\n"
        "maps, keep = _native.view_maps(cap, 8, 6)\n"
        "cams = np.ones(14); res = _native.RmViewFeatures()\n"
        "def view(w=8, h=6, n=1, cams=cams, maps=maps, out=res):\n"
        "    rc = L.rm_view_features(w, h, n, P(cams), None if maps is None else ctypes.byref(maps), None if out is None else ctypes.byref(out), None)\n"
        "    print(rc, len(L.rm_last_error()))\n"
        "view(cams=None); view(maps=None); view(out=None); view(n=0); view(n=65536)\n"
        "for k in ('depth', 'normal', 'evals', 'hit'):\n"
        "    m = _native.RmViewMaps(maps.depth, maps.normal, maps.evals, maps.hit); setattr(m, k, None); view(maps=m)\n"
        "bad = cams.copy(); bad[5] = np.nan; view(cams=bad)\n"
        "view(w=0); view(h=-1); view(w=65536, h=32768)\n"
        "view()\n")
    env = dict(os.environ, PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, check=True, capture_output=True, text=True).stdout
    rows = [[int(v) for v in line.split()] for line in out.strip().splitlines()]
    ARG, SCENE, DIMS, NODEV = _native.RM_E_BAD_ARG, _native.RM_E_BAD_SCENE, -3, _native.RM_E_NO_DEVICE
    assert [r[0] for r in rows] == [ARG] * 17 + [SCENE] * 3 + [NODEV] * 3 + [ARG] * 10 + [DIMS] * 3 + [NODEV], out
    assert all(r[1] > 0 for r in rows), out


# ---- 6. features.py and the sweep around the calls -----------------------------------------------------------------------------

def test_constants_are_the_reference_s():
    assert (features.GRAZING_COS, features._LIP_SAMPLES, features._LIP_EPS, features._CHORDS, features._CHORD_STEPS) == \
        (0.20, 1500, 1e-4, 240, 160)
    assert features.FEATURE_KEYS == ("hit_rate", "grazing_frac", "silhouette_cplx", "hardness_mean", "hardness_cv", "lipschitz_p99",
                                     "thin_slab")


def test_padded_box():
    lo, hi, diag = features.padded_box([-1.0, 0.0, 2.0], [1.0, 0.0, 6.0])
    assert np.array_equal(lo, np.array([-1.0, 0.0, 2.0]) - (0.05 * np.array([2.0, 0.0, 4.0]) + 1e-3))
    assert np.array_equal(hi, np.array([1.0, 0.0, 6.0]) + (0.05 * np.array([2.0, 0.0, 4.0]) + 1e-3))
    assert diag == float(np.linalg.norm([2.0, 0.0, 4.0]))
    assert features.padded_box([1.0, 1.0, 1.0], [1.0, 1.0, 1.0])[2] == 1.0      # a point: diag falls back to 1


def test_intrinsic_features_draws_box_after_box_and_skips_views_without_hits(host, monkeypatch):
    """features.intrinsic_features with the host build over the oracle standing in for the device call: one call for all
    boxes, NaN and no draw for a view without a box, thin_slab in box diagonals"""
    calls = []

    def fake(scene_id, sets, eps=features._LIP_EPS, details=False, warmup=0, repeats=0):
        calls.append(len(sets))
        return [r for r, _, _ in host.intrinsic(sets, oracle.sdf_eval(scene_id, host.points(sets, eps)), eps)]

    monkeypatch.setattr(features, "intrinsic_features_device", fake)
    monkeypatch.setattr(features, "_LIP_SAMPLES", 60)
    monkeypatch.setattr(features, "_CHORDS", 12)
    boxes = [((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)), None, ((-0.5, -1.0, 0.0), (1.0, 0.5, 1.0))]
    got = features.intrinsic_features(2, boxes, np.random.default_rng(3))
    assert calls == [2] and np.isnan(got[1]["lipschitz_p99"]) and np.isnan(got[1]["thin_slab"])
    rng = np.random.default_rng(3)
    for i in (0, 2):
        lo, hi, diag = features.padded_box(*boxes[i])
        s = features.sample_sets(lo, hi, rng, 60, 12)
        want = features.intrinsic_features_numpy(2, [s], sdf=lambda p: oracle.sdf_eval(2, p))[0]
        assert C.bits(got[i]["lipschitz_p99"])[0] == C.bits(want["lipschitz_p99"])[0]
        assert C.bits(got[i]["thin_slab"])[0] == C.bits(float(np.float64(want["slab_median"]) / diag))[0]


def test_sweep_features_option_before_the_device():
    assert sweep.FEATURE_FIELDS == ["feat_hit_rate", "feat_grazing_frac", "feat_silhouette_cplx", "feat_hardness_mean", "feat_hardness_cv",
                                    "feat_lipschitz_p99", "feat_thin_slab"]
    assert not set(sweep.FEATURE_FIELDS) & set(sweep.ROW_FIELDS + sweep.ORACLE_FIELDS + sweep.CEILING_FIELDS + sweep.SSIM_FIELDS)
    with pytest.raises(KeyError):                                                # nothing new is refused: names are checked as before
        sweep.run_sweep(["No Such Scene"], ["Standard"], features=True)
    with pytest.raises(ValueError):
        sweep.run_sweep(["Sphere"], ["Standard"], features=True, oracle="nonesuch")
    row = dict.fromkeys(sweep.ROW_FIELDS, 0)
    with tempfile.TemporaryDirectory() as td:
        plain, feat = os.path.join(td, "a.csv"), os.path.join(td, "b.csv")
        sweep.write_rows([row], plain)
        sweep.write_rows([dict(row, **dict.fromkeys(sweep.FEATURE_FIELDS, 0.5))], feat)
        assert open(plain).readline().strip().split(",") == sweep.ROW_FIELDS
        assert open(feat).readline().strip().split(",") == sweep.ROW_FIELDS + sweep.FEATURE_FIELDS


def test_command_line_parses():
    with pytest.raises(SystemExit):
        features.main(["--no-such-option"])
    with pytest.raises(KeyError):
        features.build(["No Such Scene"], 16)


# ---- 7. the code object ----------------------------------------------------------------------------------------------------------

OBJ = os.path.join(ROOT, "raymarch_algo_compare_amd", "_build", "features.o")


def test_code_object_no_scratch_no_spills():
    """as test_segment_host does for segment.o"""
    import importlib.util
    assert os.path.exists(OBJ), "features.o is missing: build the library (make -C raymarch_algo_compare_amd/csrc)"
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    kernels = [k for k in tool.collect([OBJ]) if "_kernel" in k["demangled"]]
    assert sorted(re.search(r"\w+_kernel", k["demangled"]).group(0) for k in kernels) == \
        ["feat_chord_kernel", "feat_grad_kernel", "feat_points_kernel", "feat_select_kernel", "view_finish_kernel", "view_mean_kernel",
         "view_tile_kernel", "view_var_kernel"]
    found = tool.matching_instructions(OBJ, r"\b(scratch|buffer)_")
    for k in kernels:
        assert found.get(k["name"]) == [], (k["demangled"], found.get(k["name"], "not disassembled")[:4])
        assert k["vgpr_spill_count"] == 0, k["demangled"]
        assert k["private_segment_fixed_size"] == 0, k["demangled"]
