"""The two bodies behind every rare-path test of the team forms (csrc/rm_math_trig.h ONE RARE-PATH TEST PER CALL:
rm_acos_team, rm_atan2_team, rm_sincos_team, rm_do_sin_team) and the root with the sparse flag handed down
(rm_pow_half_sparse, csrc/rm_math_pow.h), on the host.

On the device a wave takes the general body when some live lane needs a rare band and the common body otherwise; which
one an argument meets therefore depends on its neighbours in the wave.  Both must return the dense form's bits.  The
host build of tests/native/math_common_check.cpp can send a call down either body whatever its argument, per test site,
and reports which sites' own predicates asked for the general body.  With the harness of tests/test_math_exact_team.py
(its argument sets, its comparison, its libm) every function is held

  * natural (each argument alone, a wave of one), every site forced general, each site forced general on its own: to
    the dense form bit for bit on every argument, claimed or not, and to glibc on the claimed domain;
  * every site forced common, and each site forced common on its own: the same, on every argument whose own predicate
    at the forced sites is "common" -- the arguments a wave could bring to that body.  This is the check that the
    factored band bodies stayed one arithmetic.

Arguments: the sets of tests/test_math_exact_team.py, and for every high-word threshold of a predicate the value at,
below and above it with their neighbours 1 ulp away, a few thousand seeded arguments per band, and for the root the
near-midpoint set of tests/test_math_exact.py.  The banded forms (COMMON false: what a full wave runs) are held to the
same on the same arguments."""
import ctypes

import numpy as np
import pytest

import math_cases as mc
import test_math_exact_team as team
from conftest import build_native

N_BAND = 4000
DP = ctypes.POINTER(ctypes.c_double)
BP = ctypes.POINTER(ctypes.c_uint8)
SITE = {"ACOS": 0, "SINCOS": 1, "DO_SIN": 2, "ATAN2_ENTRY": 3, "ATAN2_FORM": 4}       # RM_SITE_* of csrc/rm_math_trig.h
SITES = {"acos": ["ACOS"], "sincos": ["SINCOS", "DO_SIN"], "atan2": ["ATAN2_ENTRY", "ATAN2_FORM"]}
NATURAL, GENERAL, COMMON = 0, 1, 2


@pytest.fixture(scope="module")
def libm():
    return ctypes.CDLL(build_native("math_check"))


@pytest.fixture(scope="module")
def forms():
    return ctypes.CDLL(build_native("math_common_check"))


def _p(a, t=DP):
    return a.ctypes.data_as(t)


def _team(L, family, cols, modes):
    """the team form with the sites of `modes` forced; returns (results, mask of the sites whose own predicate was rare)"""
    for s in SITE.values():
        L.rmt_force(s, NATURAL)
    for name, mode in modes.items():
        L.rmt_force(SITE[name], mode)
    cols = [np.ascontiguousarray(c, np.float64) for c in cols]
    n = len(cols[0])
    rare = np.zeros(n, np.uint8)
    if family == "sincos":
        s, c = np.empty(n), np.empty(n)
        L.rmt_sincos(_p(cols[0]), ctypes.c_size_t(n), _p(s), _p(c), _p(rare, BP))
        out = (s, c)
    else:
        o = np.empty(n)
        getattr(L, "rmt_" + family)(*[_p(c) for c in cols], ctypes.c_size_t(n), _p(o), _p(rare, BP))
        out = (o,)
    for s in SITE.values():
        L.rmt_force(s, NATURAL)
    return out, rare


def _threshold_words(words):
    """high-word thresholds: the value at, below and above each, with the neighbours 1 ulp away"""
    k = np.asarray(words, np.uint64)
    return mc.nbrs(np.concatenate([mc.hiword(k - 1), mc.hiword(k), mc.hiword(k + 1)]), 1)


def _own_sets(family):
    rng = np.random.default_rng({"acos": 61, "sincos": 62, "atan2": 63}[family])
    if family == "acos":
        thr = mc.both_signs(_threshold_words([0x3c880000, 0x3fc00000, 0x3fef0000, 0x3ff00000]))
        bands = [rng.uniform(-0.125, 0.125, N_BAND), rng.uniform(0.125, 0.96875, N_BAND), -rng.uniform(0.125, 0.96875, N_BAND),
                 rng.uniform(0.96875, 1.0, N_BAND), -rng.uniform(0.96875, 1.0, N_BAND),
                 np.exp(rng.uniform(-45, -36, N_BAND)) * rng.choice([-1, 1], N_BAND)]
        return [("thresholds", (thr,))] + [(f"band {i}", (b,)) for i, b in enumerate(bands)]
    if family == "sincos":
        thr = mc.both_signs(_threshold_words([0x3e400000, 0x3e500000, 0x3feb6000, 0x400368fd, 0x419921fb]))
        k = np.arange(0, 40, dtype=np.float64)
        taylor = mc.both_signs(np.concatenate([mc.nbrs(0.126, 2), mc.nbrs(k[2:] * (np.pi / 2) + 0.126, 2),
                                               mc.nbrs(k[2:] * (np.pi / 2) - 0.126, 2)]))
        bands = [rng.uniform(-0.855, 0.855, N_BAND), rng.uniform(0.8555, 2.4262, N_BAND) * rng.choice([-1, 1], N_BAND),
                 rng.uniform(2.4263, 8 * np.pi, N_BAND) * rng.choice([-1, 1], N_BAND), rng.uniform(-1e8, 1e8, N_BAND),
                 np.exp(rng.uniform(-20, -17, N_BAND)), (np.rint(rng.uniform(2, 40, N_BAND)) * (np.pi / 2) + rng.uniform(-0.126, 0.126, N_BAND))]
        return [("thresholds", (thr,)), ("do_sin 0.126", (taylor,))] + [(f"band {i}", (b,)) for i, b in enumerate(bands)]
    # atan2: the exponent window [2^-500, 2^500) of either operand, the exponent gap of 57, u = 1/16, |y| = |x|, the sign of x
    e = _threshold_words([(1023 - 500) << 20, (1023 + 500) << 20])
    one = np.full(len(e), 1.5)
    gap = np.concatenate([mc.nbrs(np.ldexp(1.5, g), 1) for g in (-58, -57, -56, -55, 55, 56, 57, 58)])
    x = rng.uniform(0.5, 4.0, 64)
    ys = [np.concatenate([e, one, gap]), np.concatenate([np.nextafter(0.0625 * v, [0, np.inf, v]) for v in x] + [mc.nbrs(v, 1) for v in x])]
    xs = [np.concatenate([one, e, np.full(len(gap), 1.5)]), np.concatenate([np.full(3, v) for v in x] + [np.full(3, v) for v in x])]
    sets = [("thresholds", mc.quadrants(np.concatenate(ys), np.concatenate(xs)))]
    for i, (lo, hi) in enumerate([(0.0, 0.0625), (0.0625, 1.0)]):       # series and table forms, x the larger and the smaller
        big, q = rng.uniform(0.1, 8.0, N_BAND), rng.uniform(lo, hi, N_BAND)
        sets.append((f"band {2 * i}", mc.quadrants(big * q, big)))
        sets.append((f"band {2 * i + 1}", mc.quadrants(big, big * q)))
    sets.append(("off the plain path", mc.quadrants(np.exp(rng.uniform(-700, 700, N_BAND)), np.exp(rng.uniform(-700, 700, N_BAND)))))
    return sets


def _all_sets(family):
    return [(n, [np.ascontiguousarray(c, np.float64) for c in cols]) for n, cols in team._sets(family) + _own_sets(family)]


def _claimed(family, cols, ref):
    if family == "atan2":          # the rule of tests/test_math_exact_team.py: zeros count, subnormal quotients do not
        return np.isfinite(cols[0]) & np.isfinite(cols[1]) & ((np.abs(ref[0]) >= 2.2250738585072014e-308) | (ref[0] == 0.0))
    return mc.claimed(team.FORMS[family][2], *cols)


@pytest.mark.parametrize("family", list(SITES))
def test_both_bodies_equal_the_dense_form_and_libm(libm, forms, family):
    sites = SITES[family]
    plans = [("natural", {}, [])] + [("all general", {s: GENERAL for s in sites}, [])] + \
            [(f"{s} general", {s: GENERAL}, []) for s in sites] + \
            [("all common", {s: COMMON for s in sites}, sites)] + [(f"{s} common", {s: COMMON}, [s]) for s in sites]
    took_common = {name: 0 for name, _, forced in plans if forced}
    met_rare = {s: 0 for s in sites}
    for set_name, cols in _all_sets(family):
        dense = team._eval(forms, team.FORMS[family][1], *cols)
        ref = team._libm(libm, family, cols)
        claimed = _claimed(family, cols, ref)
        for plan, modes, forced in plans:
            got, rare = _team(forms, family, cols, modes)
            entitled = np.ones(len(cols[0]), bool)
            for s in forced:
                entitled &= (rare & (1 << SITE[s])) == 0
            if forced:
                took_common[plan] += int(entitled.sum())
            else:
                for s in sites:
                    met_rare[s] += int(((rare & (1 << SITE[s])) != 0).sum())
            for o, (g, d, r) in enumerate(zip(got, dense, ref)):
                for what, want, keep in (("dense", d, entitled), ("libm", r, entitled & claimed)):
                    bad = np.flatnonzero(team._differ(g, want) & keep)
                    for i in bad[:5]:
                        print(f"{family} out{o} [{plan}] {set_name}: args {[float(c[i]) for c in cols]!r} team={g[i]!r} {what}={want[i]!r}")
                    assert len(bad) == 0, (family, plan, set_name, what, len(bad))
    # neither body was left untested: every site met arguments of both kinds
    assert all(n > 10_000 for n in took_common.values()), took_common
    assert all(n > 1_000 for n in met_rare.values()), met_rare


@pytest.mark.parametrize("family", list(SITES))
def test_banded_forms_equal_the_dense_form_and_libm(libm, forms, family):
    """the forms a full wave runs (COMMON false, csrc/rm_math_trig.h): the general bodies with no entry test"""
    for set_name, cols in _all_sets(family):
        got = team._eval(forms, "rmb_" + family, *cols)
        dense = team._eval(forms, team.FORMS[family][1], *cols)
        ref = team._libm(libm, family, cols)
        claimed = _claimed(family, cols, ref)
        for o, (g, d, r) in enumerate(zip(got, dense, ref)):
            assert not (team._differ(g, d)).any(), (family, set_name, o, "dense")
            assert not (team._differ(g, r) & claimed).any(), (family, set_name, o, "libm")


def test_thresholds_sit_where_the_predicates_put_them(forms):
    """the value at a threshold and the one 1 ulp below it fall on different sides of the site's own predicate"""
    def rare_of(family, cols, site):
        return (_team(forms, family, cols, {})[1] & (1 << SITE[site])) != 0

    at, below = mc.hiword([0x3fc00000, 0x3fef0000]), np.nextafter(mc.hiword([0x3fc00000, 0x3fef0000]), 0.0)
    assert list(rare_of("acos", [at], "ACOS")) == [False, True] and list(rare_of("acos", [below], "ACOS")) == [True, False]
    at = mc.hiword([0x3e500000, 0x3feb6000, 0x400368fd, 0x419921fb])
    assert list(rare_of("sincos", [at], "SINCOS")) == [False, True, False, True]
    assert list(rare_of("sincos", [np.nextafter(at, 0.0)], "SINCOS")) == [True, False, True, False]
    assert list(rare_of("sincos", [np.array([0.126, np.nextafter(0.126, 0.0)])], "DO_SIN")) == [False, True]
    y = np.array([2.0 ** -500, np.nextafter(2.0 ** -500, 0.0), np.nextafter(2.0 ** 500, 0.0), 2.0 ** 500, 1.0, 1.0, 1.0, 1.0])
    x = np.array([2.0 ** -500, 2.0 ** -500, 2.0 ** 499, 2.0 ** 499, 2.0 ** 56, 2.0 ** 57, 2.0 ** -56, 2.0 ** -57])
    assert list(rare_of("atan2", [y, x], "ATAN2_ENTRY")) == [False, True, False, True, False, True, False, True]
    y, x = np.array([0.0625, np.nextafter(0.0625, 0.0), 0.5, 0.5, 2.0]), np.array([-1.0, -1.0, 1.0, -1.0, 1.0])
    assert list(rare_of("atan2", [y, x], "ATAN2_FORM")) == [False, True, True, False, False]


def test_the_root_with_the_flag_handed_down(forms):
    """rm_pow_half_sparse: with the flag on or off, guard passed or failed, the bits are pow(x, 0.5)'s"""
    rng = np.random.default_rng(64)
    x = np.concatenate([mc.near_midpoint_roots(rng, 200_000), rng.uniform(0, 100.0, 100_000), np.exp(rng.uniform(-30, 30, 100_000)),
                        mc.nbrs(np.array([0.0, 2.0 ** -60, 2.0 ** 60, 1.0, 4.0, 16.0]), 2)])
    x = np.ascontiguousarray(x[(x >= 0) & ~np.signbit(x)])
    ref = np.empty(len(x))
    forms.rmc_pow_half(_p(x), ctypes.c_size_t(len(x)), _p(ref))
    failed = np.zeros(len(x), np.uint8)
    for sparse in (1, 0):
        got = np.empty(len(x))
        forms.rmt_pow_half_sparse(_p(x), ctypes.c_size_t(len(x)), sparse, _p(got), _p(failed, BP))
        bad = np.flatnonzero(team._differ(got, ref))
        for i in bad[:5]:
            print(f"sparse={sparse} x={float(x[i])!r} got={got[i]!r} pow={ref[i]!r}")
        assert len(bad) == 0, (sparse, len(bad))
    assert 1_000 < int(failed.sum()) < len(x) - 1_000        # both sides of the guard were there
