"""The argument sets of tests/math_cases.py reach what they are meant to reach (no GPU needed): every band boundary of
csrc/rm_math_*.h on both sides, every row of every libm table -- computed with the headers' own index formulas -- so that
an edit of the sets cannot quietly drop the arguments tests/test_gpu_math_exact.py depends on.  And on the new sets the
host restatement equals glibc wherever its STATUS claims so."""
import ctypes

import numpy as np
import pytest

import math_cases as mc
from conftest import build_native


def _all(rows, n):
    got = set(np.unique(rows[rows >= 0]).tolist())
    assert got == set(range(n)), sorted(set(range(n)) - got)[:20]


def _sides(values, boundary_bits):
    """some value just below and some at-or-above each boundary (bit patterns of positive doubles)"""
    b = mc.u64(np.abs(values))
    for t in boundary_bits:
        t = np.uint64(t)
        assert (b == t - np.uint64(1)).any() and (b == t).any() and (b == t + np.uint64(1)).any(), hex(int(t))


def test_pow_sets_reach_every_row_and_edge():
    x, y = mc.pow_sets()["rows"]
    _all(mc.rows_pow_log(x), 128)
    _all(mc.rows_exp(x, y), 128)
    x, y = mc.pow_sets()["edges"]
    _sides(x[y == 0.5], [0x3c30000000000000, 0x43b0000000000000])            # the sparse guard's 2^-60 and 2^60
    _sides(x, [0x3ff0000000000000])                                           # x next to 1
    assert ((x > 0) & (x < 2.0 ** -1022) & (y == 0.5)).sum() >= 5             # subnormal bases of the square root
    mpmath = pytest.importorskip("mpmath")
    with np.errstate(all="ignore"):
        r = np.log2(x) * y
    for yy in (2.0, 7.0, 8.0):                                                # results on both sides of 2^-1022, 2^1024
        for edge in (-1022, 1024):
            near = x[(y == yy) & (np.abs(r - edge) < 0.01)]
            with mpmath.workprec(200):
                side = [mpmath.power(mpmath.mpf(float(v)), int(yy)) < mpmath.mpf(2) ** edge for v in near]
            assert any(side) and not all(side), (yy, edge)
    _all(mc.rows_pow_log(mc.pow2_sets()["rows"][0]), 128)


def test_sincos_sets_reach_every_row_and_edge():
    e = mc.sincos_sets()["edges"][0]
    rng, a = mc.sincos_reduced(e)
    _all(mc.rows_sincos(a[rng == 1]), 110)                                     # do_cos of range 1 reads every row
    _all(mc.rows_sincos(a[(rng == 1) & (np.abs(a) >= 0.126)]) - 17, 110 - 17)  # do_sin's table band: rows 17 .. 109
    _all(mc.rows_sincos(a[rng == 2]), 110)                                     # do_sin(hp0 - |x|) of range 2
    th = mc.sincos_sets()["thresholds"][0]
    _sides(th, [int(mc.u64(mc.hiword([k]))[0]) for k in mc.SINCOS_THRESHOLDS] + [int(mc.u64([0.126])[0])])
    assert (th < 0).sum() == (th > 0).sum()
    m = mc.sincos_sets()["multiples"][0]
    k = np.rint(np.abs(m) / (np.pi / 2))
    assert k.max() == 2 ** 20 and len(np.unique(k)) > 2 ** 20 - 10
    r, a = mc.sincos_reduced(mc.sincos_sets()["edges"][0])
    red = a[r == 3]
    assert ((np.abs(red) < 0.126) & (np.abs(red) > 0.1259)).any() and ((np.abs(red) > 0.126) & (np.abs(red) < 0.1261)).any()


def test_acos_sets_reach_every_band_row_and_edge():
    s = mc.acos_sets()
    _all(mc.rows_asncs(s["rows"][0]), 216)
    _all(mc.rows_inroot(s["rows"][0]), 128)
    assert set(mc.bands_acos(s["edges"][0]).tolist()) == {0, 1, 2, 3, 4}
    _sides(s["edges"][0], [int(mc.u64(mc.hiword([k]))[0]) for k in mc.ACOS_THRESHOLDS])
    _sides(-s["edges"][0][s["edges"][0] < 0], [int(mc.u64(mc.hiword([k]))[0]) for k in mc.ACOS_THRESHOLDS])


def test_atan2_sets_reach_every_band_row_and_edge():
    s = mc.atan2_sets()
    y, x = s["rows"]
    _all(mc.rows_cij(y, x), 241)
    y, x = s["edges"]
    fin = np.isfinite(x) & np.isfinite(y) & (x != 0) & (y != 0)
    assert set(mc.bands_atan2(y[fin], x[fin]).tolist()) == {0, 1, 2, 3}
    u = mc.atan2_quotient(y[fin], x[fin])
    _sides(u, [int(mc.u64([0.0625])[0])])                                      # the quotient at 1/16
    de = ((mc.u64(y) >> np.uint64(52)) & np.uint64(0x7ff)).astype(np.int64) - ((mc.u64(x) >> np.uint64(52)) & np.uint64(0x7ff)).astype(np.int64)
    for g in (56, 57, 58):
        assert (de[fin] == g).any() and (de[fin] == -g).any(), g
    ax, ay = np.abs(x), np.abs(y)
    for t in (2.0 ** -500, 2.0 ** 500):
        assert (ax == t).any() and (ax == np.nextafter(t, 0)).any() and (ay == np.nextafter(t, np.inf)).any()
    quad = {(bool(np.signbit(a)), bool(np.signbit(b))) for a, b in zip(y[fin], x[fin])}
    assert len(quad) == 4
    zeros = {(bool(np.signbit(a)), bool(np.signbit(b))) for a, b in zip(y, x) if a == 0 and b == 0}
    assert len(zeros) == 4                                                      # (+-0, +-0)


def test_log_sets_reach_every_row_and_edge():
    s = mc.log_sets()
    x = s["rows"][0]
    _all(mc.rows_log(x), 128)
    _all(mc.rows_log(x[x < 2.0 ** -1022]), 128)                                # through the subnormal normalisation too
    e = s["edges"][0]
    _sides(e, [mc.LOG_NEAR1_LO, mc.LOG_NEAR1_LO + mc.LOG_NEAR1_SPAN, mc.LOG_OFF, 0x0010000000000000])
    assert ((e > 0) & (e < 2.0 ** -1022)).sum() >= 5 and (e == 5e-324).any()


def test_sqrt_and_pow_half_sets_hold_their_edges():
    e = mc.sqrt_sets()["edges"][0]
    assert (e == 5e-324).any() and (e == np.finfo(np.float64).max).any() and ((e > 0) & (e < 2.0 ** -1022)).sum() >= 5
    assert len(mc.sqrt_sets()["near_midpoint"][0]) >= 100_000
    _sides(mc.pow_half_sets()["edges"][0], [0x3c30000000000000, 0x43b0000000000000])


# ---- the host restatement on the new sets --------------------------------------------------------------------------

@pytest.fixture(scope="module")
def m():
    return ctypes.CDLL(build_native("math_check"))


def _libm(L, name, a, b=None):
    dp = ctypes.POINTER(ctypes.c_double)
    out = np.empty_like(a)
    args = [a] if b is None else [a, b]
    getattr(L, name)(*[v.ctypes.data_as(dp) for v in args], ctypes.c_size_t(len(a)), out.ctypes.data_as(dp))
    return out


@pytest.mark.parametrize("fam,fn,lib", [("pow", "POW", "rml_pow"), ("sincos", "SIN", "rml_sin"), ("sincos", "COS", "rml_cos"),
                                        ("acos", "ACOS", "rml_acos"), ("atan2", "ATAN2", "rml_atan2"), ("log", "LOG", "rml_log")])
def test_host_restatement_equals_libm_where_claimed(m, fam, fn, lib):
    for name, args in mc.FAMILY_SETS[fam](200_000).items():
        a, b = args[0], (args[1] if len(args) > 1 else None)
        got = mc.host_eval(m, fn, a, b)[0]
        ref = _libm(m, lib, a, b)
        keep = mc.claimed(fn, a, b) | (np.isnan(a) if b is None else np.isnan(a) | np.isnan(b))
        if fn == "ATAN2":
            keep |= (a == 0) | (b == 0)                                         # signed zeros are claimed, bit for bit
        bad = keep & (mc.u64(got) != mc.u64(ref)) & ~(np.isnan(got) & np.isnan(ref))
        assert not bad.any(), (name, a[bad][:4], None if b is None else b[bad][:4])


def test_pow_outside_its_claim_is_what_the_status_says(m):
    """512 <= |y log x| with a normal result is not claimed: there glibc rescales (specialcase) and rm_pow does not.  Pinned
    so that the STATUS comment of csrc/rm_math_pow.h stays true: results rarely differ by 1 ulp, and are NaN next to
    2^1024"""
    rng = np.random.default_rng(9)
    y = rng.uniform(0.5, 16, 400_000)
    x = np.exp(rng.uniform(-708, -512, len(y)) / y)
    got, ref = mc.host_eval(m, "POW", x, y)[0], _libm(m, "rml_pow", x, y)
    d = mc.u64(got).astype(np.int64) - mc.u64(ref).astype(np.int64)
    assert 0 < (d != 0).sum() < 0.002 * len(y) and np.abs(d).max() == 1
    x = np.nextafter(2.0 ** 512, 0)
    assert np.isnan(mc.host_eval(m, "POW", np.array([x]), np.array([2.0]))[0][0])
