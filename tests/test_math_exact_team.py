"""The team forms of the libm restatements (rm_acos_team, rm_atan2_team, rm_sincos_team, rm_do_sin_team: what
rm_acos<true>, rm_atan2<true> and rm_sincos<true> run, csrc/rm_math_atan.h and rm_math_trig.h) on the host.

They restate the arithmetic of the dense forms in another block order, so nothing tests/test_math_exact.py says about
the dense forms carries over.  Here the host build of the team forms (rmc_acos_u, rmc_atan2_u, rmc_sincos_u of
tests/native/math_check.cpp; on the host every guarded block runs and every select chooses) is held

  * to glibc's libm bit for bit, on the ranges tests/test_math_exact.py uses for the dense forms, on every argument
    set of tests/math_cases.py inside the claimed domain, and on the operands tests/test_gpu_uniform_paths.py lays its
    waves out from;
  * to the dense forms bit for bit on every argument of those sets, claimed or not (NaN is one class).

The device tests compare the device's team forms with host values; this is what ties those host values to libm."""
import ctypes

import numpy as np
import pytest

import math_cases as mc
import uniform_path_cases as up
from conftest import build_native

N = 400_000
DP = ctypes.POINTER(ctypes.c_double)


@pytest.fixture(scope="module")
def m():
    return ctypes.CDLL(build_native("math_check"))


def _p(a):
    return a.ctypes.data_as(DP)


def _eval(L, name, *cols):
    """one- or two-argument routine with one result; rmc_sincos / rmc_sincos_u: (sin, cos)"""
    cols = [np.ascontiguousarray(c, np.float64) for c in cols]
    n = ctypes.c_size_t(len(cols[0]))
    if "sincos" in name:
        s, c = np.empty(len(cols[0])), np.empty(len(cols[0]))
        getattr(L, name)(_p(cols[0]), n, _p(s), _p(c))
        return s, c
    out = np.empty(len(cols[0]))
    getattr(L, name)(*[_p(c) for c in cols], n, _p(out))
    return (out,)


def _differ(a, b):
    return (mc.u64(a) != mc.u64(b)) & ~(np.isnan(a) & np.isnan(b))


def _libm(L, family, cols):
    if family == "acos":
        return _eval(L, "rml_acos", *cols)
    if family == "atan2":
        return _eval(L, "rml_atan2", *cols)
    return _eval(L, "rml_sin", *cols) + _eval(L, "rml_cos", *cols)


FORMS = {"acos": ("rmc_acos_u", "rmc_acos", "ACOS_U"), "atan2": ("rmc_atan2_u", "rmc_atan2", "ATAN2_U"),
         "sincos": ("rmc_sincos_u", "rmc_sincos", "SINCOS_U")}


def _own_ranges(family):
    """the ranges of tests/test_math_exact.py for the dense form of the family"""
    rng = np.random.default_rng({"acos": 6, "atan2": 7, "sincos": 3}[family])
    if family == "sincos":
        return [(x,) for x in (rng.uniform(-8 * np.pi, 8 * np.pi, N), rng.uniform(-0.2, 0.2, N), rng.uniform(-3, 3, N),
                               rng.uniform(-400, 400, N), rng.uniform(-1e8, 1e8, N),
                               np.exp(rng.uniform(-40, 3, N)) * rng.choice([-1, 1], N),
                               np.array([0.0, -0.0, 0.126, -0.126, 0.855469, 2.426265, np.pi, -np.pi, np.pi / 2, 1e-9, 105414300.0]))]
    if family == "acos":
        v = rng.normal(size=(N, 3))
        return [(x,) for x in (rng.uniform(-1, 1, N), rng.uniform(0.96, 1.0, N), -rng.uniform(0.96, 1.0, N),
                               rng.uniform(-0.13, 0.13, N), 1.0 - np.exp(rng.uniform(-40, -3, N)),
                               -1.0 + np.exp(rng.uniform(-40, -3, N)), np.exp(rng.uniform(-60, 0, N)) * rng.choice([-1, 1], N),
                               np.array([0.0, -0.0, 1.0, -1.0, 0.125, 0.5, 0.75, 0.921875, 0.953125, 0.96875, -0.125, -0.5,
                                         -0.75, -0.921875, -0.953125, -0.96875, 0.25, -0.25, 1e-17, 2.7e-17, 0.9999999999999999]),
                               np.clip(v[:, 2] / np.sqrt((v * v).sum(1)), -1, 1))]

    def sg():
        return rng.choice([-1, 1], N)
    sp = np.array([0.0, -0.0, 1.0, -1.0, 2.0, -2.0, 1e-300, -1e-300, 1e300, 0.0625, 16.0])
    yy, xx = np.meshgrid(sp, sp)
    return [(rng.uniform(-4, 4, N), rng.uniform(-4, 4, N)), (rng.normal(size=N), rng.normal(size=N)),
            (np.exp(rng.uniform(-30, 30, N)) * sg(), np.exp(rng.uniform(-30, 30, N)) * sg()),
            (np.exp(rng.uniform(-700, 700, N)) * sg(), np.exp(rng.uniform(-700, 700, N)) * sg()),
            (rng.uniform(-1, 1, N) * 1e-3, rng.uniform(-4, 4, N)), (rng.uniform(-4, 4, N), rng.uniform(-1, 1, N) * 1e-3),
            (yy.ravel().copy(), xx.ravel().copy())]


def _sets(family):
    """(name, columns) of every argument set the team form of the family is compared on"""
    out = [(f"range {i}", cols) for i, cols in enumerate(_own_ranges(family))]
    out += [(f"math_cases {name}", cols) for name, cols in mc.FAMILY_SETS[family]().items()]
    out.append(("uniform-path operands", up.OPERANDS[FORMS[family][2]]()[0]))
    return out


@pytest.mark.parametrize("family", list(FORMS))
def test_team_forms_equal_libm(m, family):
    """inside the claimed domain every bit of the team form is libm's"""
    team, _, fn = FORMS[family]
    checked = 0
    for name, cols in _sets(family):
        cols = [np.ascontiguousarray(c, np.float64) for c in cols]
        got, ref = _eval(m, team, *cols), _libm(m, family, cols)
        keep = mc.claimed(fn, *cols)
        if family == "atan2":                  # the rule of tests/test_math_exact.py: zeros count, subnormal quotients do not
            keep = np.isfinite(cols[0]) & np.isfinite(cols[1]) & ((np.abs(ref[0]) >= 2.2250738585072014e-308) | (ref[0] == 0.0))
        for o, (g, r) in enumerate(zip(got, ref)):
            bad = np.flatnonzero(_differ(g, r) & keep)
            for i in bad[:5]:
                print(f"{team} out{o} {name}: args {[float(c[i]) for c in cols]!r} team={g[i]!r} libm={r[i]!r}")
            assert len(bad) == 0, (team, name, len(bad))
        checked += int(keep.sum())
    assert checked > 1_000_000


@pytest.mark.parametrize("family", list(FORMS))
def test_team_forms_equal_the_dense_forms(m, family):
    """every argument, claimed or not: the team form returns what the dense form returns"""
    team, dense, _ = FORMS[family]
    for name, cols in _sets(family):
        for o, (g, r) in enumerate(zip(_eval(m, team, *cols), _eval(m, dense, *cols))):
            bad = np.flatnonzero(_differ(g, r))
            for i in bad[:5]:
                print(f"{team} out{o} {name}: args {[float(np.asarray(c)[i]) for c in cols]!r} team={g[i]!r} dense={r[i]!r}")
            assert len(bad) == 0, (team, name, len(bad))
