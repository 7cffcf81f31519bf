"""Shared by tests/test_features_host.py and tests/test_gpu_features.py: the reference's recorded intrinsic features
(tests/golden/features_intrinsic.npz, written by tools/gen_features_golden.py from the reference itself), the host build
of csrc/rm_features.h (tests/native/features_check.cpp) and hand-made captures for the view features."""
import ctypes
import os

import numpy as np

from conftest import GOLDEN, build_native
from raymarch_algo_compare_amd import _native
from raymarch_algo_compare_amd.camera import Camera

dp = ctypes.POINTER(ctypes.c_double)
u8p = ctypes.POINTER(ctypes.c_uint8)
NAN_BITS = 0x7ff8000000000000
EPS = 1e-4


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


# ---- the fixture -----------------------------------------------------------------------------------------------------------

_fixture = None


def fixture_cases():
    """[(label, dict)]: scene, seed, n_lip, n_chords, steps, the sample set, diag, gmag bits, slab_counts, the reference's
    lipschitz_p99 and thin_slab bits"""
    global _fixture
    if _fixture is None:
        z = np.load(os.path.join(GOLDEN, "features_intrinsic.npz"))
        out = []
        for c in range(int(z["ncases"][0])):
            p = f"c{c}_"
            sid, seed, n_lip, n_chords, steps = (int(v) for v in z[p + "meta"])
            half = float(z[p + "box"][1, 0])
            out.append((f"{c}-{z['names'][c]}-{half:g}-{n_lip}", {
                "scene": sid, "seed": seed, "n_lip": n_lip, "n_chords": n_chords, "steps": steps, "box": z[p + "box"],
                "set": {k: z[p + k] for k in ("pts", "chords", "seglen", "ts")}, "diag": float(z[p + "diag"][0]),
                "gmag": z[p + "gmag"], "slab_counts": z[p + "slab_counts"], "want": z[p + "want"]}))
        _fixture = out
    return _fixture


def thin_slab(slab_median, diag):
    """the host's one step after the device: the median length in box diagonals"""
    return float(np.float64(slab_median) / diag)


def check_case(case, res, gmag, counts, label):
    """one set's result (a dict of RmIntrinsicFeatures' fields, gmag, slab_counts) against the reference, bit for bit"""
    assert np.array_equal(bits(gmag), case["gmag"]), (label, "gmag", int((bits(gmag) != case["gmag"]).sum()))
    assert np.array_equal(np.asarray(counts, np.int32), case["slab_counts"]), (label, "slab counts")
    assert res["n_finite"] == case["n_lip"] and res["n_slabs"] == int(case["slab_counts"].sum()), (label, res)
    assert bits(res["lipschitz_p99"])[0] == case["want"][0], (label, res["lipschitz_p99"], case["want"][0].view(np.float64))
    if res["n_slabs"] == 0:
        assert bits(res["slab_median"])[0] == NAN_BITS and np.isnan(case["want"][1:].view(np.float64)[0]), label
    else:
        got = thin_slab(res["slab_median"], case["diag"])
        assert bits(got)[0] == case["want"][1], (label, got, case["want"][1:].view(np.float64)[0])


# ---- the host build ------------------------------------------------------------------------------------------------------

class Host:
    """tests/native/features_check.cpp built by g++, prototypes declared"""

    def __init__(self):
        L = ctypes.CDLL(build_native("features_check"))
        i32, vp = ctypes.c_int32, ctypes.c_void_p
        L.rmft_check_intrinsic.argtypes = [i32, i32, vp, ctypes.c_double, i32, vp, vp, i32, vp, vp]
        L.rmft_check_intrinsic.restype = ctypes.c_char_p
        L.rmft_check_seglen.argtypes = [i32, i32, vp]
        L.rmft_check_seglen.restype = ctypes.c_char_p
        L.rmft_num_points.argtypes = [ctypes.c_int] * 4
        L.rmft_num_points.restype = ctypes.c_size_t
        L.rmft_points.argtypes = [ctypes.c_int] * 4 + [ctypes.c_double, dp, dp, dp, dp]
        L.rmft_points.restype = None
        L.rmft_intrinsic.argtypes = [ctypes.c_int] * 4 + [ctypes.c_double, dp, dp, ctypes.POINTER(_native.RmIntrinsicFeatures), dp, vp]
        L.rmft_runs.argtypes = [ctypes.c_int, u8p, ctypes.c_double, dp]
        L.rmft_runs_by_lanes.argtypes = L.rmft_runs.argtypes
        L.rmft_select.argtypes = [ctypes.c_int, ctypes.c_int64, dp, dp]
        L.rmft_view.argtypes = [ctypes.c_int, ctypes.c_int, dp, vp, vp, vp, u8p, ctypes.POINTER(_native.RmViewFeatures)]
        self.L = L

    def points(self, sets, eps=EPS):
        """the xyz buffer rm_intrinsic_features makes of `sets` (sample_sets dicts of one shape): (n, 3)"""
        pts, chords, seglen, ts = _stacked(sets)
        n = self.L.rmft_num_points(len(sets), pts.shape[1], chords.shape[1], len(ts))
        xyz = np.empty((n, 3))
        self.L.rmft_points(len(sets), pts.shape[1], chords.shape[1], len(ts), eps, _dp(pts), _dp(chords), _dp(ts), _dp(xyz))
        return xyz

    def intrinsic(self, sets, f, eps=EPS):
        """the results of `sets` from the values f of points(sets): [(fields dict, gmag, slab_counts)]"""
        pts, chords, seglen, ts = _stacked(sets)
        n, n_lip, n_chords = len(sets), pts.shape[1], chords.shape[1]
        res = (_native.RmIntrinsicFeatures * n)()
        gmag, counts = np.empty((n, n_lip)), np.empty((n, n_chords), np.int32)
        f = np.ascontiguousarray(f, np.float64)
        rc = self.L.rmft_intrinsic(n, n_lip, n_chords, len(ts), eps, _dp(seglen), _dp(f), res, _dp(gmag), counts.ctypes.data)
        assert rc == 0, rc      # 2: score_next_rank did not give the sorted sample's next element; 3: more runs than slots
        return [({k: getattr(res[i], k) for k, _ in _native.RmIntrinsicFeatures._fields_}, gmag[i], counts[i]) for i in range(n)]

    def runs(self, inside, seglen, by_lanes=False):
        inside = np.ascontiguousarray(inside, np.uint8)
        out = np.full(len(inside) // 2 + 2, -1.0)
        fn = self.L.rmft_runs_by_lanes if by_lanes else self.L.rmft_runs
        n = fn(len(inside), inside.ctypes.data_as(u8p), float(seglen), _dp(out))
        assert n >= 0, "a run end without a start"
        return out[:n]

    def select(self, sel, values):
        values = np.ascontiguousarray(values, np.float64)
        out = ctypes.c_double()
        rc = self.L.rmft_select(sel, len(values), _dp(values), ctypes.byref(out))
        assert rc == 0, rc
        return out.value

    def view(self, capture, cam14):
        """rm_view_features of one capture dict, as _native.view_features gives it"""
        h, w = np.asarray(capture["hit"]).shape
        maps, keep = _native.view_maps(capture, w, h)
        res = _native.RmViewFeatures()
        cam14 = np.ascontiguousarray(cam14, np.float64)
        rc = self.L.rmft_view(w, h, _dp(cam14), maps.depth, maps.normal, maps.evals, keep[3].ctypes.data_as(u8p), ctypes.byref(res))
        assert rc == 0, rc
        out = {k: getattr(res, k) for k, _ in _native.RmViewFeatures._fields_[:9]}
        out["box_lo"], out["box_hi"] = np.array(res.box_lo[:]), np.array(res.box_hi[:])
        return out


def _dp(a):
    return a.ctypes.data_as(dp)


def _stacked(sets):
    from raymarch_algo_compare_amd import features
    return features._stack(sets)


# ---- hand-made captures -----------------------------------------------------------------------------------------------------

def camera(width, height):
    return Camera((0.3, 0.4, 5.0), (0.0, 0.1, 0.0), (0.0, 1.0, 0.0), 60.0, width, height)


def capture_of(hit, seed):
    """a capture dict with the hit mask `hit`: depths in [2, 7], unit normals of every direction (some grazing), integer
    eval counts with ties; values off the mask are junk that must not be read"""
    hit = np.asarray(hit, bool)
    h, w = hit.shape
    rng = np.random.default_rng(seed)
    normal = rng.normal(size=(h, w, 3))
    normal /= np.linalg.norm(normal, axis=2, keepdims=True)
    depth = rng.uniform(2.0, 7.0, size=(h, w))
    evals = rng.integers(1, 400, size=(h, w)).astype(np.float64)
    depth[~hit], evals[~hit] = np.nan, 1e9
    normal[~hit] = np.nan
    return {"hit": hit, "depth": depth.astype(np.float32), "normal": normal.astype(np.float32), "evals": evals.astype(np.float32)}


def masks(width, height):
    """[(name, hit mask)] of one frame size"""
    yy, xx = np.mgrid[0:height, 0:width]
    block = np.zeros((height, width), bool)
    block[: max(1, height // 2), : max(1, width // 3)] = True                  # touches the top and the left edge
    one = np.zeros((height, width), bool)
    one[height // 2, width // 2] = True
    disc = (xx - width / 2.0) ** 2 + (yy - height / 2.0) ** 2 < (min(width, height) / 3.0) ** 2
    return [("all hit", np.ones((height, width), bool)), ("no hit", np.zeros((height, width), bool)), ("one pixel", one),
            ("checkerboard", (xx + yy) % 2 == 0), ("edge block", block), ("disc", disc)]


SHAPES = [(1, 1), (16, 12), (50, 37)]
COUNT_KEYS = ("n_hit", "n_grazing", "n_perimeter", "sum_evals")
VALUE_KEYS = ("hit_rate", "grazing_frac", "silhouette_cplx", "hardness_mean", "hardness_cv")


def view_cases():
    return [(f"{w}x{h} {name}", capture_of(mask, 1000 * w + i), camera(w, h)) for w, h in SHAPES for i, (name, mask) in enumerate(masks(w, h))]


def check_view_against_numpy(got, want, label):
    """counts equal; doubles within 1e-12 relative; box corners within 1e-12 absolute (the host's ray_directions and the
    kernel's ray differ by a few ulp, and depth <= 100)"""
    assert [got[k] for k in COUNT_KEYS] == [want[k] for k in COUNT_KEYS], (label, got, want)
    for k in VALUE_KEYS:
        assert abs(got[k] - want[k]) <= 1e-12 * abs(want[k]), (label, k, got[k], want[k])
    if want["n_hit"] == 0:
        assert all(got[k] == 0.0 for k in VALUE_KEYS) and np.all(got["box_lo"] == np.inf) and np.all(got["box_hi"] == -np.inf), label
        return
    assert np.all(np.abs(got["box_lo"] - want["box_lo"]) <= 1e-12) and np.all(np.abs(got["box_hi"] - want["box_hi"]) <= 1e-12), \
        (label, got["box_lo"], want["box_lo"], got["box_hi"], want["box_hi"])


def same_view(a, b, label):
    """two rm_view_features results, bit for bit"""
    for k in COUNT_KEYS:
        assert a[k] == b[k], (label, k, a[k], b[k])
    for k in VALUE_KEYS:
        assert bits(a[k])[0] == bits(b[k])[0], (label, k, a[k], b[k])
    assert np.array_equal(bits(a["box_lo"]), bits(b["box_lo"])) and np.array_equal(bits(a["box_hi"]), bits(b["box_hi"])), label
