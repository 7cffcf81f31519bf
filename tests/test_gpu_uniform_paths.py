"""The wave-uniform select paths of rm_acos<true>, rm_atan2<true> and rm_sincos<true> (csrc/rm_math_atan.h,
rm_math_trig.h: rm_acos_team, rm_atan2_team, rm_sincos_team) on the MI355X, bit for bit against the host values of the
DENSE forms (math_cases.host_eval of ACOS, ATAN2, SINCOS), which tests/test_math_exact.py holds to libm.  The host build of
the team forms is not the reference: it is the same restated arithmetic as the code under test.  (tests/test_math_exact_team.py
holds that host build to libm and to the dense forms as well.)

With U the selects of these routines sit inside ballot-guarded blocks: which of them a lane's value passes through
depends on what the OTHER live lanes of its wave hold.  tests/test_gpu_math_exact.py draws its sparse waves at random
from pools around the band edges; here every wave is laid out on purpose, from operands at and next to every cut, so
that each guarded block is entered and skipped with the lane under test on either side of its select:

  alone       one live lane: every operand by itself
  same        two live lanes holding operands of one class
  different   two live lanes, every ordered pair of distinct classes
  special     five live lanes: one special operand among four ordinary ones, and one ordinary among four special
  dense       all 64 lanes: one class per wave, then every operand mixed

A class is the set of blocks an operand selects (band, range, quadrant case), or `special` for the operands the
ladders serve.  The class functions restate the headers' predicates in NumPy (math_cases.bands_*).

NaN is one class, as in tests/test_gpu_math_exact.py; every other bit counts."""
import ctypes
import itertools

import numpy as np
import pytest

import math_cases as mc
from uniform_path_cases import OPERANDS, SPECIAL
from conftest import build_native

pytestmark = pytest.mark.gpu

LANES = {"alone": [17], "same": [9, 50], "different": [9, 50], "special": [0, 13, 31, 32, 63], "dense": list(range(64))}


# ---- wave layouts (index arrays into the operands, `live` entries per wave) ----------------------------------------

def _waves(pattern, cls):
    idx = np.arange(len(cls))
    groups = {c: idx[cls == c] for c in sorted(set(cls))}
    ordinary = np.concatenate([g for c, g in groups.items() if c != SPECIAL])
    special = groups[SPECIAL]
    if pattern == "alone":
        return [[i] for i in idx]
    if pattern == "same":
        return [[a, b] for g in groups.values() for a, b in zip(g, np.roll(g, 1))]
    if pattern == "different":
        out = []
        for p, q in itertools.permutations(groups, 2):
            n = max(len(groups[p]), len(groups[q]))
            out += [[groups[p][j % len(groups[p])], groups[q][j % len(groups[q])]] for j in range(n)]
        return out
    if pattern == "special":
        out = []
        for j, s in enumerate(special):                      # each special operand in each of the five places
            for place in range(5):
                w = [ordinary[(5 * j + place + t) % len(ordinary)] for t in range(5)]
                w[place] = s
                out.append(w)
        for j, o in enumerate(ordinary):                     # and each ordinary operand among special ones
            w = [special[(j + t) % len(special)] for t in range(5)]
            w[j % 5] = o
            out.append(w)
        return out
    if pattern == "dense":
        out = [[g[t % len(g)] for t in range(64)] for g in groups.values()]
        mixed = np.resize(idx, 64 * -(-len(idx) // 64))
        return out + [list(r) for r in mixed.reshape(-1, 64)] + [list(r) for r in np.roll(mixed, 7).reshape(-1, 64)]
    raise KeyError(pattern)


# ---- the reference, once per routine ------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def reference():
    host = ctypes.CDLL(build_native("math_check"))
    out = {}
    for fn, make in OPERANDS.items():
        args, cls = make()
        assert SPECIAL in cls and len(set(cls)) >= 4, fn
        ref = mc.host_eval(host, fn[:-2], *args)                  # the dense form: ACOS_U -> ACOS, ...
        for r in ref:
            if r is not None:
                r.setflags(write=False)
        out[fn] = (args, cls, ref)
    return out


def _differ(dev, ref):
    return (mc.u64(dev) != mc.u64(ref)) & ~(np.isnan(dev) & np.isnan(ref))


@pytest.mark.parametrize("pattern", list(LANES))
@pytest.mark.parametrize("fn", list(OPERANDS))
def test_uniform_paths_equal_the_host(hip, reference, fn, pattern):
    args, cls, ref = reference[fn]
    waves = np.array(_waves(pattern, cls), dtype=np.int64)
    lanes = LANES[pattern]
    assert waves.shape[1] == len(lanes)
    if pattern == "different":                               # every ordered pair of classes shares a wave
        assert {(cls[a], cls[b]) for a, b in waves} == set(itertools.permutations(set(cls), 2))
    e = waves.reshape(-1)
    mask = sum(1 << l for l in lanes)
    dev = hip.debug_math_eval(fn, *[c[e] for c in args], lane_mask=mask)
    nbad = 0
    for o, (d, r) in enumerate(zip(dev, ref)):
        if r is None:
            continue
        bad = np.flatnonzero(_differ(d, r[e]))
        for i in bad[:10]:
            print(f"MISMATCH {fn} {pattern} out{o}: args " + " ".join(f"{c[e[i]]!r}" for c in args) +
                  f" device={d[i]!r} host={r[e[i]]!r} wave={i // len(lanes)} lane={lanes[i % len(lanes)]} "
                  f"wave classes={[int(cls[j]) for j in waves[i // len(lanes)]]}")
        nbad += len(bad)
    print(f"{fn} {pattern}: {len(waves)} waves of {len(lanes)} live lanes, {nbad} mismatches")
    assert nbad == 0
