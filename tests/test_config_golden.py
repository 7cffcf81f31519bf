"""The oracle (oracle/rm_oracle.c), the host build of the kernel headers (tests/native/host_check.cpp) and camera.py
against what the REFERENCE computes away from the default MarchConfig: tests/golden/frames_config_<family>.npz and
rays_config.npz, written by oracle/gen_golden.py --only config / rays (seed CONFIG_SEED there).

  A  the sweep's grid: every budget and epsilon level (caps 512 and 2048) from the curated viewpoints, fov 60
  B  budget edges 0..18 and bisection counts 0, 1, budget, budget + 1
  C  hit thresholds 0 / 1e-9 / 0.5, far planes below / inside / far beyond the object, Lipschitz 0.1..4, constructor
     arguments at both ends of their range, budgets around the last bin of the iteration histogram
  D  cameras inside and on the object, degenerate bases, other up vectors, fov 5 / 150; odd frame shapes and row slices
  E  seeded random draws over all of it
  rays  explicit rays: unit, un-normalised, zero and near-1e-12 directions, origins inside and beyond the far plane

Everything is compared bit for bit: iterations, hits, the stored bits of t, and the hashes of t, final_sdf and of
the float32 depth map.  The coverage the families promise is recomputed here from the files themselves."""
import ctypes
import json
import os

import numpy as np
import pytest

import config_cases as cc
from conftest import GOLDEN, build_native, sha_f64
from oracle import oracle

SHADER_PARAMS = {"step_scale": 1.0, "dense_min_step": 1e-4}      # the two RmStrategyParams fields after the reference's sixteen
BUDGETS = [32, 64, 128, 256, 512]                                # the reference's DEFAULT_BUDGETS (sweep.py:48)
EPSILONS = [1e-2, 3e-3, 1e-3, 3e-4, 1e-4, 3e-5, 1e-5]            # ... and DEFAULT_EPSILONS (sweep.py:54)
BUDGET_EDGES = (0, 1, 2, 3, 15, 16, 17, 18)
FRACTALS = (9, 10)
LARGEST_FIXTURE_BEFORE = 1200132                                 # frames_64x48.npz
DP = ctypes.POINTER(ctypes.c_double)


def _check(c, hit, t, it, fs, who):
    """One frame against its fixture.  fs None: the lean path, which has no final_sdf."""
    what = f"{who}: {cc.label(c)}"
    assert (np.asarray(it).reshape(-1) == c["iters"].reshape(-1)).all(), what
    assert (np.asarray(hit).reshape(-1) == c["hit"].reshape(-1)).all(), what
    assert cc.first_bad_ray(c, t) is None, (what, "first ray with another t", cc.first_bad_ray(c, t))
    assert sha_f64(t) == c["sha_t"], what
    assert cc.sha_depth32(hit, t) == c["sha_depth32"], what
    if fs is not None:
        assert sha_f64(fs) == c["sha_fs"], what


@pytest.mark.parametrize("fam", cc.FAMILIES)
def test_oracle_matches_reference(fam):
    cases = cc.family(fam)
    for c in cases:
        fr = oracle.render(c["sid"], c["kid"], c["cam"], c["W"], c["H"], c["row0"], c["rows"], c["max_iterations"],
                           c["hit_threshold"], c["max_distance"], c["lipschitz"], params=c["prm"])
        _check(c, fr.hit, fr.t, fr.iters, fr.final_sdf, "oracle")
    print(f"family {fam}: {len(cases)} cases")


@pytest.fixture(scope="module")
def hostlib():
    L = ctypes.CDLL(build_native("host_check"))
    L.rmh_render.argtypes = ([ctypes.c_int] * 3 + [ctypes.c_double] * 3 + [ctypes.c_int, DP] + [ctypes.c_int] * 4
                             + [ctypes.c_void_p, DP, ctypes.c_void_p, DP, DP])
    L.rmh_march_rays.argtypes = ([ctypes.c_int] * 3 + [ctypes.c_double] * 3 + [ctypes.c_int, DP, DP, ctypes.c_size_t]
                                 + [ctypes.c_void_p, DP, ctypes.c_void_p, DP, DP])
    return L


def _prm18(prm):
    return np.array([float(prm[k]) for k in cc.PARAM_ORDER] + [SHADER_PARAMS["step_scale"], SHADER_PARAMS["dense_min_step"]])


@pytest.mark.parametrize("full", [1, 0])
@pytest.mark.parametrize("fam", cc.FAMILIES)
def test_kernel_headers_match_reference(hostlib, fam, full):
    for c in cc.family(fam):
        n = c["rows"] * c["W"]
        hit, t, it, fs = np.empty(n, np.uint8), np.empty(n, np.float64), np.empty(n, np.int32), np.empty(n, np.float64)
        cam, prm = np.ascontiguousarray(c["cam"]), _prm18(c["prm"])
        rc = hostlib.rmh_render(c["sid"], c["kid"], c["max_iterations"], c["hit_threshold"], c["max_distance"], c["lipschitz"],
                                full, cam.ctypes.data_as(DP), c["W"], c["H"], c["row0"], c["rows"], hit.ctypes.data,
                                t.ctypes.data_as(DP), it.ctypes.data, fs.ctypes.data_as(DP), prm.ctypes.data_as(DP))
        assert rc == 0
        _check(c, hit, t, it, fs if full else None, f"kernel headers, full={full}")


@pytest.mark.parametrize("fam", cc.FAMILIES)
def test_cameras_match_reference(fam):
    """camera.py and oracle.camera14 build the 14 doubles of every case's camera bit for bit -- degenerate bases included."""
    from raymarch_algo_compare_amd.camera import Camera
    for c in cc.family(fam):
        v = c["view"]
        want = c["cam"].view(np.uint64)
        got = Camera(tuple(v[0:3]), tuple(v[3:6]), tuple(v[6:9]), float(v[9]), c["W"], c["H"]).params14()
        assert (got.view(np.uint64) == want).all(), ("camera.py", cc.label(c))
        got = oracle.camera14(tuple(v[0:3]), tuple(v[3:6]), tuple(v[6:9]), float(v[9]), c["W"], c["H"])
        assert (got.view(np.uint64) == want).all(), ("oracle.camera14", cc.label(c))


def _check_rays(p, hit, t, it, fs, who):
    what = (who, p["n"], p["sid"], p["kid"])
    bad = np.nonzero((it != p["iters"]) | (hit != p["hit"]) | (t.view(np.uint64) != p["t_bits"]))[0]
    assert len(bad) == 0, (what, "first bad ray", int(bad[0]), p["o"][bad[0]].tolist(), p["d"][bad[0]].tolist())
    if fs is not None:
        assert (fs.view(np.uint64) == p["fs_bits"]).all(), what


def test_oracle_rays_match_reference():
    for p in cc.ray_pairs():
        hit, t, it, fs = oracle.march_rays(p["sid"], p["kid"], p["o"], p["d"], p["max_iterations"], p["hit_threshold"],
                                           p["max_distance"], p["lipschitz"], params=p["prm"])
        _check_rays(p, hit, t, it, fs, "oracle")


@pytest.mark.parametrize("full", [1, 0])
def test_kernel_headers_rays_match_reference(hostlib, full):
    """rmh_march_rays: the headers' own normalized() and march_one on the stored origins and directions."""
    for p in cc.ray_pairs():
        n = len(p["o"])
        hit, t, it, fs = np.empty(n, np.uint8), np.empty(n, np.float64), np.empty(n, np.int32), np.empty(n, np.float64)
        o, d, prm = np.ascontiguousarray(p["o"]), np.ascontiguousarray(p["d"]), _prm18(p["prm"])
        rc = hostlib.rmh_march_rays(p["sid"], p["kid"], p["max_iterations"], p["hit_threshold"], p["max_distance"], p["lipschitz"],
                                    full, o.ctypes.data_as(DP), d.ctypes.data_as(DP), n, hit.ctypes.data, t.ctypes.data_as(DP),
                                    it.ctypes.data, fs.ctypes.data_as(DP), prm.ctypes.data_as(DP))
        assert rc == 0
        _check_rays(p, hit, t, it, fs if full else None, f"kernel headers, full={full}")


# ---- what the fixtures cover, recomputed from the files --------------------------------------------------------------

def _default_prm(c):
    return all(c["prm"][k] == v for k, v in oracle.DEFAULT_PARAMS.items() if k in c["prm"])


def _scenes(cases):
    return {c["sid"] for c in cases}


def test_family_a_covers_the_sweep_grid():
    A = cc.family("A")
    assert all(c["view"][9] == 60.0 and c["max_distance"] == 100.0 and _default_prm(c) for c in A)
    levels = [(b, 1e-4) for b in BUDGETS] + [(512, e) for e in EPSILONS] + [(2048, e) for e in EPSILONS]
    assert {(c["max_iterations"], c["hit_threshold"]) for c in A} == set(levels)
    for kid in range(11):
        for lv in levels:
            sc = _scenes(c for c in A if c["kid"] == kid and (c["max_iterations"], c["hit_threshold"]) == lv)
            assert len(sc) >= 3, (kid, lv, sc)
            assert lv[0] != 2048 or not sc & set(FRACTALS), (kid, lv, sc)
        mandel = [c for c in A if c["kid"] == kid and c["sid"] == 10]
        assert len({c["max_iterations"] for c in mandel if c["hit_threshold"] == 1e-4}) >= 2, kid
        assert len({c["hit_threshold"] for c in mandel if c["max_iterations"] == 512}) >= 2, kid
    seen = {(c["sid"], tuple(c["view"][:9])) for c in A}
    with open(os.path.join(GOLDEN, "viewpoints.json"), encoding="utf-8") as f:
        curated = json.load(f)
    assert len(curated) == 20 and sum(len(v) for v in curated.values()) == 53
    for scene, views in curated.items():
        for name, _, pos, tgt, up in views:
            assert (oracle.SCENE_NAMES.index(scene), tuple(map(float, pos + tgt + up))) in seen, (scene, name)
    # every frame belongs to a group the sweep would issue as one batch: same scene, strategy and viewpoint, >= 5 levels
    groups = {}
    for c in A:
        groups.setdefault(c["tag"].rsplit("/", 1)[0], []).append(c)
    assert all(len(g) >= 5 and len({(c["sid"], c["kid"], tuple(c["view"])) for c in g}) == 1 for g in groups.values())


def test_family_b_covers_the_budget_edges():
    B = cc.family("B")
    for kid in range(11):
        for b in BUDGET_EDGES:
            assert len(_scenes(c for c in B if c["kid"] == kid and c["max_iterations"] == b and _default_prm(c))) >= 3, (kid, b)
    for kid, field in ((6, "overstep_bisection_steps"), (10, "segment_bisection_steps"), (8, "revaa_bisection_steps")):
        for b in BUDGET_EDGES:
            for n in (0, 1, b, b + 1):
                assert len(_scenes(c for c in B if c["kid"] == kid and c["max_iterations"] == b and c["prm"][field] == n)) >= 3, (kid, b, n)
    # the two frames test_oracle_golden.test_edge_cases asserts on
    assert [(c["sid"], c["kid"], c["W"], c["H"], c["max_iterations"]) for c in B if c["tag"].startswith("B/edge/")] == \
        [(0, 0, 8, 4, 0), (0, 6, 8, 4, 10)]


# constructor arguments and march() literals, and the two ends of the range each is exercised at
PARAM_ENDS = dict(omega=(1.0, 2.5), ar_omega_min=(1.0, 2.5), ar_omega_max=(1.0, 2.5), ar_smoothing=(0.0, 1.0), ar_growth_rate=(1.0, 2.0),
                  ar_decay_rate=(0.0, 1.0), beta=(0.0, 1.0), overstep_min_step=(0.0, 1.0), hybrid_stuck_step_ratio=(0.0, 1.0),
                  hybrid_min_step=(0.0, 1.0), margin=(0.0, 1.0), ar_omega_init=(1.0, 2.0), overstep_bisection_steps=(1, 64),
                  hybrid_stuck_threshold=(0, 1), segment_bisection_steps=(1, 64), revaa_bisection_steps=(1, 64))


def test_family_c_covers_thresholds_far_planes_lipschitz_and_parameter_ends():
    from raymarch_algo_compare_amd import registry
    C = cc.family("C")
    for thr in (0.0, 1e-9, 0.5):
        assert {c["kid"] for c in C if c["hit_threshold"] == thr} == set(range(11)), thr
    # far planes: the SDF at the camera is a lower bound of its distance to the object
    for kid in range(11):
        mine = [c for c in C if c["kid"] == kid and c["tag"].startswith("C/far/")]
        key = lambda c: (c["sid"], tuple(c["view"]), c["max_iterations"], c["hit_threshold"])      # noqa: E731
        wide = {key(c): int(c["hit"].sum()) for c in mine if c["max_distance"] == 1e4}
        below = [c for c in mine if c["max_distance"] < oracle.sdf_eval(c["sid"], c["view"][:3])[0]]
        assert below and all(c["hit"].sum() == 0 for c in below), kid
        between = [c for c in mine if c["max_distance"] < 100.0 and 0 < c["hit"].sum() < wide[key(c)]]
        assert between, kid
        assert {1e4, 1e9} <= {c["max_distance"] for c in mine}, kid
    far_hits = 0                              # hits beyond the default far plane (t from the oracle, which sha_t pins to the fixture)
    for c in C:
        if c["max_distance"] == 1e9:
            fr = oracle.render(c["sid"], c["kid"], c["cam"], c["W"], c["H"], c["row0"], c["rows"], c["max_iterations"],
                               c["hit_threshold"], c["max_distance"], c["lipschitz"], params=c["prm"])
            far_hits += int(((fr.hit > 0) & (fr.t > 100.0)).sum())
    assert far_hits >= 10, far_hits
    for lip in (0.1, 0.5, 2.0, 4.0):
        sc = _scenes(c for c in C if c["kid"] == 10 and c["lipschitz"] == lip)
        assert any(registry.SCENES[s].lipschitz is None for s in sc), lip
        assert any(registry.SCENES[s].lipschitz not in (None, lip) for s in sc), lip
    for field, ends in PARAM_ENDS.items():
        for v in ends:
            assert any(c["prm"][field] == v and c["max_iterations"] != 512 and c["hit_threshold"] != 1e-4 for c in C), (field, v)
    # budgets around the last bin of RmStats.iter_hist (543): frames whose iterations reach 542, 543, 544 and beyond
    tops = {int(c["iters"].max()) for c in C}
    assert {542, 543, 544} <= tops and max(tops) > 2000


def test_family_d_covers_cameras_and_shapes():
    D = cc.family("D")
    at_camera = np.array([oracle.sdf_eval(c["sid"], c["view"][:3])[0] for c in D])
    assert (at_camera < 0).sum() >= 10 and (at_camera == 0.0).sum() >= 10                  # inside, exactly on the surface
    fwd_nonzero = [c for c in D if np.any(c["cam"][3:6] != 0.0)]
    assert sum(1 for c in fwd_nonzero if not np.any(c["cam"][6:12] != 0.0)) >= 10              # forward parallel to up: right = up = 0
    assert any(not np.any(c["cam"][3:12] != 0.0) for c in D)                                   # target == position
    ups = {tuple(c["view"][6:9]) for c in D}
    assert {(0.0, 0.0, 1.0), (1.0, 1.0, 0.0), (0.0, -1.0, 0.0)} <= ups
    assert {5.0, 150.0} <= {c["view"][9] for c in D}
    shapes = {(c["W"], c["H"]) for c in D}
    assert (1, 1) in shapes and any(w == 1 and h > 1 for w, h in shapes) and any(h == 1 and w > 1 for w, h in shapes)
    assert {63, 64, 65} <= {w for w, _ in shapes} and {3, 4, 5} <= {c["rows"] for c in D}
    assert sum(1 for c in D if c["row0"] % 4 and c["rows"] % 4 and c["rows"] < c["H"]) >= 5
    whole = [c for c in D if c["row0"] == 0 and c["rows"] == c["H"]]
    assert whole and all(c["refstats"] is not None for c in whole)
    for c in whole:                                                                            # the reference's own integer statistics
        s = c["refstats"]
        assert (s["total_rays"], s["hit_count"], s["miss_count"]) == (c["iters"].size, int(c["hit"].sum()), int((c["hit"] == 0).sum()))
        assert (s["sample_count"], s["iteration_min"], s["iteration_max"]) == (int(c["iters"].sum()), int(c["iters"].min()), int(c["iters"].max()))


def test_family_e_draws_from_everything():
    E = cc.family("E")
    assert len(E) >= 300
    assert _scenes(E) == set(range(20)) and {c["kid"] for c in E} == set(range(11))
    for field, least in (("max_iterations", 10), ("hit_threshold", 8), ("max_distance", 6)):
        assert len({c[field] for c in E}) >= least, field
    assert {0, 2048} <= {c["max_iterations"] for c in E} and {0.0, 0.5} <= {c["hit_threshold"] for c in E}
    assert sum(1 for c in E if not _default_prm(c)) >= 60
    assert len({c["lipschitz"] for c in E if c["kid"] == 10}) >= 4
    assert sum(1 for c in E if c["rows"] < c["H"]) >= 30 and len({tuple(c["view"][6:9]) for c in E}) == 4


def test_rays_cover_what_a_caller_may_pass():
    pairs = cc.ray_pairs()
    assert len(pairs) >= 8 and len({(p["sid"], p["kid"]) for p in pairs}) == len(pairs)
    assert len({p["kid"] for p in pairs if p["sid"] == 10}) >= 3
    assert len({(p["max_iterations"], p["hit_threshold"], p["max_distance"]) for p in pairs}) >= 6
    for p in pairs:
        assert p["o"].shape == (300, 3) and p["d"].shape == (300, 3)
        l = np.sqrt((p["d"] ** 2).sum(1))
        assert (np.abs(l - 1.0) < 1e-15).sum() >= 50                          # unit
        assert (l < 1e-5).sum() >= 10 and (l > 1e5).sum() >= 3 and l.max() <= 1e7     # un-normalised
        assert ((p["d"] == 0.0).all(1)).sum() >= 5                            # exactly zero
        assert ((l > 0) & (l < 1e-12)).sum() >= 10                            # normalises to the zero vector ...
        assert ((l > 1e-12) & (l < 1.2e-12)).sum() >= 3                       # ... and just does not
        assert (oracle.sdf_eval(p["sid"], p["o"]) < 0).sum() >= (3 if p["sid"] != 3 else 0)      # origins inside (the thin torus: none fit)
        assert (np.sqrt((p["o"] ** 2).sum(1)) > p["max_distance"]).sum() >= 20       # origins beyond the far plane


def test_fixture_sizes_and_skipped_cases():
    sizes = {f: os.path.getsize(os.path.join(GOLDEN, f)) for f in cc.FILES}
    assert max(sizes.values()) <= LARGEST_FIXTURE_BEFORE, sizes
    assert sum(sizes.values()) <= 4_000_000, sizes
    for c in cc.all_cases():
        assert c["tag"].startswith("D/shape/") or (c["W"] <= 32 and c["H"] <= 24), cc.label(c)
    sk = cc.skipped()
    assert sk["drawn"] == len(cc.all_cases()) + len(sk["skipped"])
    assert len(sk["skipped"]) <= 0.02 * sk["drawn"], [s["tag"] for s in sk["skipped"]]
    print("cases per family:", {f: len(cc.family(f)) for f in cc.FAMILIES}, "rays:", len(cc.ray_pairs()), "x 300; skipped:", len(sk["skipped"]))
