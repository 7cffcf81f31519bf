"""The device math on the MI355X, routine by routine (rm_debug_math_eval, csrc/rm_math_check.hip), against the host
restatement of the same headers (tests/native/math_check.cpp) bit for bit, and against 200-bit values (mpmath).

tests/test_math_exact.py proves the headers equal glibc on the host.  That the device computes the same bits was an
inference (IEEE fp64 arithmetic on gfx950); what the host build cannot see is checked here: clang's amdgcn lowering of
sqrt, division and ldexp, the ISA peephole, the LDS table mirrors (re-laid-out strides, copied by rm_load_tables), and
the wave-level code that exists only on the device -- the ballots of the band-skipping forms (rm_band_needed<true>) and
of the sparse square root (rm_pow_half<true>: the guarded root with at most 16 live lanes, pow for the lanes the guard
refuses).  Argument sets: tests/math_cases.py (band edges, every table row, spread samples).

NaN is one class (the host's (x - x) / (x - x) is a negative NaN, the device's may not be); every other bit counts, on
every input, claimed or not."""
import ctypes

import numpy as np
import pytest

import math_cases as mc
from conftest import build_native
from raymarch_algo_compare_amd._native import MATH_FNS

pytestmark = pytest.mark.gpu

ALL = (1 << 64) - 1
N_REPORT = 10


@pytest.fixture(scope="module")
def host():
    L = ctypes.CDLL(build_native("math_check"))
    L.rmc_pow2.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.c_size_t, ctypes.c_double, ctypes.c_double,
                           ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
    return L


def _differ(dev, ref):
    return (mc.u64(dev) != mc.u64(ref)) & ~(np.isnan(dev) & np.isnan(ref))


def _lanes(mask):
    return [l for l in range(64) if (mask >> l) & 1]


def _report(fn, what, a, b, dev, ref, bad, mask):
    """prints the first N_REPORT mismatches: argument bits, device bits, host bits, the live-lane mask and the lane"""
    idx = np.flatnonzero(bad)[:N_REPORT]
    lanes = _lanes(mask)
    for e in idx:
        arg = f"a={int(mc.u64(a[e:e + 1])[0]):016x} ({a[e]!r})"
        if b is not None:
            arg += f" b={int(mc.u64(b[e:e + 1])[0]):016x} ({b[e]!r})"
        print(f"MISMATCH {fn} {what}: {arg} device={int(mc.u64(dev[e:e + 1])[0]):016x} ({dev[e]!r}) "
              f"host={int(mc.u64(ref[e:e + 1])[0]):016x} ({ref[e]!r}) lane_mask={mask:016x} wave={e // len(lanes)} "
              f"lane={lanes[e % len(lanes)]}")
    return int(bad.sum())


def _compare(hip, host, fn, a, b, mask, what):
    dev0, dev1 = hip.debug_math_eval(fn, a, b, lane_mask=mask)
    ref0, ref1 = mc.host_eval(host, fn, a, b)
    nbad = _report(fn, what + " out0", a, b, dev0, ref0, _differ(dev0, ref0), mask)
    if ref1 is not None:
        nbad += _report(fn, what + " out1", a, b, dev1, ref1, _differ(dev1, ref1), mask)
    return nbad, dev0, dev1


@pytest.mark.parametrize("fn", list(MATH_FNS))
def test_dense_waves_equal_the_host(hip, host, fn):
    """every argument set of the routine's family, all 64 lanes live"""
    bad, n = {}, 0
    for name, args in mc.FAMILY_SETS[mc.FN_FAMILY[fn]]().items():
        a, b = args[0], (args[1] if len(args) > 1 else None)
        nbad, dev0, dev1 = _compare(hip, host, fn, a, b, ALL, name)
        n += len(a)
        if nbad:
            bad[name] = nbad
        if fn == "SQRT":                                   # correctly rounded wherever it is defined
            ok = np.isfinite(a) & (a >= 0)
            with np.errstate(invalid="ignore"):
                assert _report(fn, name + " vs np.sqrt", a, None, dev0, np.sqrt(a), ok & _differ(dev0, np.sqrt(a)), ALL) == 0
    print(f"{fn}: {n} arguments, mismatches per set {bad}")
    assert not bad


# ---- sparse waves: the band-skipping forms and the sparse square root -------------------------------------------

def _masks():
    rng = np.random.default_rng(40)

    def pick(k):
        return sum(1 << int(l) for l in rng.choice(64, k, replace=False))
    return {"lane0": 1, "lane63": 1 << 63, "two": (1 << 9) | (1 << 50), "15": pick(15), "16": pick(16), "17": pick(17),
            "32": pick(32), "63": ALL & ~(1 << 37), "random": int(rng.integers(1, 1 << 63, dtype=np.int64)) | (1 << 63)}


MASKS = _masks()


def _side(x0, down, n=24, spread=2.0 ** -20):
    """n positive doubles on one side of the boundary x0 > 0 (below it, or from it up): the nearest, then further in"""
    steps = np.arange(n // 2, dtype=np.uint64)
    b0 = mc.u64([float(x0)])[0]
    near = mc.f64(b0 - np.uint64(1) - steps) if down else mc.f64(b0 + steps)
    far = float(x0) * (1.0 + (-1.0 if down else 1.0) * spread * np.linspace(0.01, 1.0, n - n // 2))
    return np.concatenate([near, far])


def _layout(pools, live, waves=24, seed=0):
    """arguments (tuples of columns, drawn from `pools`) in three wave layouts: every live lane of a wave from ONE pool
    (one side of one boundary), waves that straddle two neighbouring pools, waves holding one argument of each pool"""
    rng = np.random.default_rng(seed)
    cols = len(pools[0])
    out = [[] for _ in range(cols)]

    def emit(src):                                           # one wave: lane r takes an argument of pool src[r]
        picks = [int(rng.integers(len(p[0]))) for p in src]
        for c in range(cols):
            out[c].append(np.array([p[c][i] for p, i in zip(src, picks)]))
    for p in pools:
        for _ in range(waves):
            emit([p] * live)
    if live > 1:
        for p, q in zip(pools[:-1], pools[1:]):
            for _ in range(waves):
                src = [p if r % 2 == 0 else q for r in range(live)]
                emit([src[r] for r in rng.permutation(live)])
        for _ in range(waves):
            emit([pools[r % len(pools)] for r in range(live)])
    return [np.concatenate(o) for o in out]


def _acos_pools():
    pools = []
    for t in mc.ACOS_THRESHOLDS:
        x0 = float(mc.hiword([t])[0])
        pools += [(_side(x0, True),), (_side(x0, False),)]
    pools.append((np.array([0.0, -0.0, 1e-30, 0.05, 0.3, 0.6, 0.99]),))
    return [(np.concatenate([p[0], -p[0]]),) for p in pools]


def _sincos_pools():
    k = np.arange(1, 200)
    p = [(_side(0.126, True),), (_side(0.126, False),),
         (_side(float(mc.hiword([0x3feb6000])[0]), True),), (_side(float(mc.hiword([0x3feb6000])[0]), False),),
         (_side(float(mc.hiword([0x400368fd])[0]), True),), (_side(float(mc.hiword([0x400368fd])[0]), False),),
         (np.pi / 2 * k + 0.1259,), (np.pi / 2 * k + 0.1261,), (np.pi / 2 * k - 0.1259,), (np.pi / 2 * k - 0.1261,)]
    return [(np.concatenate([q[0], -q[0]]),) for q in p]


def _atan2_pools():
    d = np.array([1.0, 3.0, 2.0 ** -300, 2.0 ** 400, 0.7])
    below, above = _side(0.0625, True, 12), _side(0.0625, False, 12)
    one_dn = np.nextafter(1.0, 0.0)
    pools = []
    for u, xs in ((below, 1.0), (above, 1.0), (above, -1.0), (below, -1.0)):
        pools.append((np.outer(d, u).ravel(), np.outer(d, np.full(len(u), xs)).ravel()))
    pools.append((np.outer(d, np.full(len(below), 1.0)).ravel(), np.outer(d, below).ravel()))           # |y| > |x|, series
    pools.append((np.outer(d, np.full(len(above), 1.0)).ravel(), np.outer(d, above).ravel()))           # |y| > |x|, table
    pools.append((d.copy(), d.copy()))                                                                   # |y| == |x|
    pools.append((d * one_dn, d.copy()))                                                                 # |y| < |x| by 1 ulp
    return [(np.concatenate([y, -y]), np.concatenate([x, x])) for y, x in pools]


def _pow_half_pools(host):
    """arguments the guard accepts, arguments it refuses on which the rounded root differs from pow, and refused ones on
    which it does not"""
    rng = np.random.default_rng(41)
    cand = np.concatenate([mc.near_midpoint_roots(rng, 200000), rng.uniform(0, 40.0, 20000),
                           mc.nbrs([2.0 ** -60, 2.0 ** 60], 4), 4.0 ** np.arange(-20, 21)])
    root, safe = mc.host_eval(host, "POW_HALF_GUARD", cand)
    pw, _ = mc.host_eval(host, "POW_HALF_SPARSE", cand)
    differ = _differ(root, pw)
    assert not (differ & (safe > 0)).any()
    return [(cand[safe > 0],), (cand[(safe == 0) & differ],), (cand[(safe == 0) & ~differ],)]


@pytest.fixture(scope="module")
def pow_half_pools(host):
    return _pow_half_pools(host)


@pytest.mark.parametrize("mask_name", list(MASKS))
@pytest.mark.parametrize("fn", ["ACOS_U", "ATAN2_U", "SINCOS_U", "POW_HALF_SPARSE"])
def test_sparse_waves_equal_the_host(hip, host, pow_half_pools, fn, mask_name):
    """few live lanes, placed so that a skip predicate off by one boundary value (or a missing fallback) shows"""
    mask = MASKS[mask_name]
    live = bin(mask).count("1")
    pools = {"ACOS_U": _acos_pools, "ATAN2_U": _atan2_pools, "SINCOS_U": _sincos_pools}.get(fn, lambda: pow_half_pools)()
    args = _layout(pools, live, seed=live)
    a, b = args[0], (args[1] if len(args) > 1 else None)
    nbad, _, _ = _compare(hip, host, fn, a, b, mask, f"{mask_name} ({live} live lanes)")
    assert nbad == 0
    if fn == "POW_HALF_SPARSE" and live <= 16:
        # the guarded path ran, and the fallback had work: refused lanes whose root differs from pow were in the waves
        root, safe = hip.debug_math_eval("POW_HALF_GUARD", a, lane_mask=mask)
        ref_root, ref_safe = mc.host_eval(host, "POW_HALF_GUARD", a)
        assert not _differ(root, ref_root).any() and (safe == ref_safe).all()
        pw, _ = mc.host_eval(host, "POW_HALF_SPARSE", a)
        assert ((safe == 0) & _differ(root, pw)).sum() >= 8 and (safe > 0).sum() >= 8


def test_guard_on_the_device_equals_the_host(hip, host):
    """rm_pow_half_guard: the device's rounded root and the guard's verdict are the host's, lane for lane"""
    for name, (x,) in mc.pow_half_sets().items():
        root, safe = hip.debug_math_eval("POW_HALF_GUARD", x)
        ref_root, ref_safe = mc.host_eval(host, "POW_HALF_GUARD", x)
        assert _report("POW_HALF_GUARD", name, x, None, root, ref_root, _differ(root, ref_root), ALL) == 0
        assert (safe == ref_safe).all(), name


# ---- against 200-bit values ---------------------------------------------------------------------------------------

def _subsample(fn, n=2000, seed=50):
    """the family's band-edge set in full (or its `thresholds` set), topped up with picks from every other set"""
    sets = mc.FAMILY_SETS[mc.FN_FAMILY[fn]]()
    rng = np.random.default_rng(seed)
    first = "thresholds" if "thresholds" in sets else "edges"
    parts = [sets[first]]
    rest = [k for k in sets if k != first]
    k = max(1, (n - len(sets[first][0])) // len(rest))
    for name in rest:
        i = rng.choice(len(sets[name][0]), min(k, len(sets[name][0])), replace=False)
        parts.append(tuple(c[i] for c in sets[name]))
    return [np.concatenate([p[c] for p in parts]) for c in range(len(parts[0]))]


@pytest.mark.parametrize("fn", [f for f in MATH_FNS if f != "POW_HALF_GUARD"])
def test_device_results_are_within_one_ulp(hip, fn):
    """inside the claimed domain every device result is one of the two doubles around the exact value"""
    pytest.importorskip("mpmath")
    args = _subsample(fn)
    a, b = args[0], (args[1] if len(args) > 1 else None)
    dev0, dev1 = hip.debug_math_eval(fn, a, b)
    keep = mc.claimed(fn, a, b)
    truth = mc.true_values(fn, a[keep], None if b is None else b[keep])
    outs = [(dev0[keep], [t[0] if isinstance(t, tuple) else t for t in truth])]
    if dev1 is not None:
        outs.append((dev1[keep], [t[1] for t in truth]))
    worst, nbad = 0.0, 0
    for k, (got, tv) in enumerate(outs):
        ok, err = mc.bracket_errors(got, tv)
        worst = max(worst, float(err.max()) if len(err) else 0.0)
        for i in np.flatnonzero(~ok)[:N_REPORT]:
            print(f"OUTSIDE 1 ULP {fn} out{k}: a={a[keep][i]!r}" + ("" if b is None else f" b={b[keep][i]!r}") +
                  f" device={got[i]!r} error={err[i]:.3f} ulp")
        nbad += int((~ok).sum())
    print(f"{fn}: {int(keep.sum())} claimed arguments of {len(a)}, largest error {worst:.4f} ulp")
    assert keep.sum() > 0.5 * len(a) and nbad == 0


def test_bad_calls_are_refused(hip):
    """fn out of range, no live lane, a NULL buffer the routine needs: RM_E_BAD_ARG, nothing launched"""
    L = hip.load()
    x = np.ones(4)
    dp = ctypes.POINTER(ctypes.c_double)
    p = x.ctypes.data_as(dp)
    for fn, a, b, mask, o0, o1 in [(-1, p, None, ALL, p, None), (len(MATH_FNS), p, None, ALL, p, None),
                                   (MATH_FNS["LOG"], p, None, 0, p, None), (MATH_FNS["LOG"], None, None, ALL, p, None),
                                   (MATH_FNS["LOG"], p, None, ALL, None, None), (MATH_FNS["POW"], p, None, ALL, p, None),
                                   (MATH_FNS["ATAN2_U"], p, None, ALL, p, None), (MATH_FNS["SINCOS"], p, None, ALL, p, None),
                                   (MATH_FNS["POW_HALF_GUARD"], p, None, ALL, p, None)]:
        assert L.rm_debug_math_eval(fn, a, b, 4, mask, o0, o1) == -6, fn
