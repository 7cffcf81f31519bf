"""Operands of the wave-uniform select paths of rm_acos_team, rm_atan2_team and rm_sincos_team (csrc/rm_math_atan.h,
rm_math_trig.h) -- a plain module, imported by tests/test_gpu_uniform_paths.py (which lays waves out from them) and by
tests/test_math_exact_team.py (which holds the host build of the team forms to libm on them).

Each maker returns (columns, classes): operands at and next to every cut of the routine, and for each operand the set
of blocks it selects (band, range, quadrant case) as a small integer, or SPECIAL for the operands the ladders serve.
The class functions restate the headers' predicates in NumPy (math_cases.bands_*)."""
import numpy as np

import math_cases as mc

SPECIAL = -1


def _acos_operands():
    cuts = np.concatenate([[2.0 ** -55, 0.125, 0.25, 0.5, 0.96875, 1.0], mc.hiword([0x3c880000])])   # the last: 1.5 * 2^-55
    x = mc.both_signs(np.concatenate([mc.nbrs(cuts, 1), [1e-9, 0.01, 0.1, 0.3, 0.7, 0.99]]))
    band = mc.bands_acos(x)                                  # 0 tiny, 1 Taylor, 2 table, 3 1/sqrt, 4 |x| >= 1
    return (x,), np.where((band == 0) | (band == 4), SPECIAL, band)


def _atan2_operands():
    ys, xs = [], []

    def add(y, x):
        qy, qx = mc.quadrants(np.atleast_1d(np.asarray(y, np.float64)), np.atleast_1d(np.asarray(x, np.float64)))
        ys.append(qy)
        xs.append(qx)
    u = mc.nbrs([0.0625], 1)
    for d in (1.0, 3.0):
        add(u * d, np.full(3, d))                            # u on both sides of 1/16, |y| < |x|
        add(np.full(3, d), u * d)                            # ... and |x| < |y|
    add([0.3, 1.0, 1.0, 0.01, 1.0, np.nextafter(1.0, 0.0)], [1.0, 0.3, 1.0, 1.0, 0.01, 1.0])
    z = np.array([0.0, -0.0])
    for other in (1.0, -1.0, 0.0, -0.0):                     # a zero in either operand, every sign
        ys.extend([z, np.full(2, other)])
        xs.extend([np.full(2, other), z])
    for g in (56, 57, 58):                                   # exponent gaps around the 57 cut
        for m1, m2 in ((1.0, 1.0), (1.0, np.nextafter(2.0, 0.0)), (np.nextafter(2.0, 0.0), 1.0)):
            add(m1, m2 * 2.0 ** g)
            add(m1 * 2.0 ** g, m2)
    lo, hi = mc.nbrs([2.0 ** -500], 1), mc.nbrs([2.0 ** 500], 1)
    for e in (lo, hi):                                       # operands at, below and above the rescaling's bounds
        add(e, e * 3.0)
        add(e * 3.0, e)
        add(e * 0.02, e)
    add([2.0 ** -510, 2.0 ** -505, 2.0 ** 505, 2.0 ** 510, 2.0 ** -510, 1.0, 1.5 * 2.0 ** -560, 2.0 ** 560],
        [2.0 ** -505, 2.0 ** -510, 2.0 ** 510, 2.0 ** 505, 1.0, 2.0 ** 510, 2.0 ** -505, 1.25 * 2.0 ** 505])
    y, x = np.concatenate(ys), np.concatenate(xs)
    ey = ((mc.u64(y) >> np.uint64(52)) & np.uint64(0x7ff)).astype(np.int64)
    ex = ((mc.u64(x) >> np.uint64(52)) & np.uint64(0x7ff)).astype(np.int64)
    off = (ey < 523) | (ey >= 1523) | (ex < 523) | (ex >= 1523) | (np.abs(ey - ex) >= 57)   # rm_atan2's off_path
    return (y, x), np.where(off, SPECIAL, mc.bands_atan2(y, x))


def _sincos_operands():
    cuts = np.concatenate([mc.hiword([0x3e400000, 0x3e500000, 0x3feb6000, 0x400368fd]), [0.126, 0.855469, 2.426265]])
    k = np.arange(1, 17, dtype=np.float64)                   # up to 8 pi, n & 3 = 0..3 four times over
    far = np.concatenate([np.pi / 2 * k + d for d in (0.05, -0.05, 0.3, -0.3, 0.126, -0.126)])
    x = mc.both_signs(np.concatenate([mc.nbrs(cuts, 1), far, [0.05, 0.5, 1.0, 2.0, 8 * np.pi, 2.0e8, np.inf]]))
    hi = mc.hi32(x)
    rng, a = mc.sincos_reduced(np.where(np.isfinite(x), x, 0.0))
    n = np.rint(x[rng == 3] * (2.0 / np.pi)).astype(np.int64) & 3
    assert set(n) == {0, 1, 2, 3}
    cls = 2 * rng + (np.abs(a) < 0.126)                      # range, and which form do_sin selects
    return (x,), np.where((hi < 0x3e500000) | (hi >= 0x419921fb), SPECIAL, cls)


OPERANDS = {"ACOS_U": _acos_operands, "ATAN2_U": _atan2_operands, "SINCOS_U": _sincos_operands}
