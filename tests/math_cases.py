"""Argument sets of the device-math tests (tests/test_gpu_math_exact.py) and their host counterparts -- a plain module,
imported by the tests that need it.

Each family (pow, pow2, pow_half, sqrt, sincos, acos, atan2, log) has named sets:
  * `edges`: nextafter neighbours of every band boundary of csrc/rm_math_*.h (the high-word thresholds of the selects and
    of the wave-uniform skip predicates rm_band_needed<true>), specials, signed zeros, subnormals;
  * `rows`: both ends of every row of the family's tables (pow's log and exp tables, the log table, __sincostab, asncs,
    inroot, cij), so a mirror row that rm_load_tables() copies wrongly into LDS is read by some argument;
  * `random_*`: spread samples like those of tests/test_math_exact.py, `n` arguments each.
A set is a tuple (a,) or (a, b) of float64 arrays.  tests/test_math_cases.py checks, with the headers' own index formulas,
that the sets reach every band and row they are meant to reach.

`bands_*` / `rows_*` below are those formulas restated in NumPy (used by that check and by the sparse-wave layouts)."""
import ctypes
import functools

import numpy as np

N_RANDOM = 1_000_000        # arguments per random set (the host suite, tests/test_math_exact.py, uses 400 000)


# ---- bits ---------------------------------------------------------------------------------------------------------

def f64(bits):
    return np.asarray(bits, dtype=np.uint64).view(np.float64)


def u64(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def hiword(k):
    """the doubles whose high 32 bits are k (low word 0)"""
    return f64(np.asarray(k, dtype=np.uint64) << np.uint64(32))


def hi32(x):
    return (u64(x) >> np.uint64(32)).astype(np.int64) & 0x7fffffff


def nbrs(x, k=2):
    """x and its k nextafter neighbours on either side (every element, both directions)"""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    out, up, dn = [x], x, x
    with np.errstate(over="ignore"):
        for _ in range(k):
            up, dn = np.nextafter(up, np.inf), np.nextafter(dn, -np.inf)
            out += [up, dn]
    return np.concatenate(out)


def both_signs(x):
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    return np.concatenate([x, -x])


def quadrants(y, x):
    """(y, x) in all four sign combinations"""
    y, x = np.asarray(y, np.float64), np.asarray(x, np.float64)
    return np.concatenate([y, y, -y, -y]), np.concatenate([x, -x, x, -x])


SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 5e-324, -5e-324, 2.2250738585072014e-308,
                     1.7976931348623157e308])


def near_midpoint_roots(rng, n):
    """tests/test_math_exact.py's construction: x = RN((s + (0.5 + t) ulp)^2), square roots within ~0.03 ulp of a
    rounding midpoint -- where pow(x, 0.5) and the rounded root may differ and the guard must refuse"""
    s = rng.uniform(1.0, 2.0, n).astype(np.longdouble)
    t = rng.uniform(-0.03, 0.03, n).astype(np.longdouble)
    m = s + (np.longdouble(0.5) + t) * np.longdouble(2.0) ** -52
    return (m * m).astype(np.float64) * np.ldexp(1.0, 2 * rng.integers(-12, 12, n))


# ---- index formulas of the headers --------------------------------------------------------------------------------

POW_LOG_OFF = 0x3fe6955500000000
LOG_OFF = 0x3fe6000000000000
LOG_NEAR1_LO, LOG_NEAR1_SPAN = 0x3fee000000000000, 0x3090000000000


def _normal_bits(x):
    """rm_pow_norm_bits / the subnormal branch of rm_log: the bits of a positive x brought into the normal range"""
    x = np.asarray(x, np.float64)
    ix = u64(x)
    with np.errstate(over="ignore", invalid="ignore"):
        sx = (u64(x * 2.0 ** 52) & np.uint64(0x7fffffffffffffff)) - np.uint64(52 << 52)
    return np.where(ix < np.uint64(0x0010000000000000), sx, ix)


def rows_pow_log(x):
    """row of pow's log table (rm_pow_log_inline), for positive finite x"""
    return ((_normal_bits(x) - np.uint64(POW_LOG_OFF)) >> np.uint64(45)).astype(np.int64) & 127


def rows_exp(x, y):
    """row of the exp table (rm_pow_exp_inline: round(y log x * 128 / ln 2) mod 128), from the float64 value of y log x:
    the sets put it far from a rounding tie except where a tie is the point"""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        e = np.asarray(y, np.float64) * np.log(np.asarray(x, np.float64)) * (128.0 / np.log(2.0))
    ok = np.isfinite(e) & (np.abs(e) < 2.0 ** 50)
    return np.where(ok, np.rint(np.where(ok, e, 0.0)).astype(np.int64) & 127, -1)


def rows_log(x):
    """row of the log table (rm_log), -1 inside the near-one window, for non-special positive x"""
    ix = _normal_bits(x)
    near = (u64(x) - np.uint64(LOG_NEAR1_LO)) < np.uint64(LOG_NEAR1_SPAN)
    return np.where(near, -1, ((ix - np.uint64(LOG_OFF)) >> np.uint64(45)).astype(np.int64) & 127)


def rows_sincos(a):
    """row of __sincostab for the argument a of do_sin / do_cos (u = big + |a|, rm_sincos_row)"""
    u = np.float64(1.5 * 2.0 ** 45) + np.abs(np.asarray(a, np.float64))
    i = (u64(u) & np.uint64(0xffffffff)).astype(np.int64)
    return np.where(i > 109, 0, i)


def bands_acos(x):
    """0 tiny (|x| < 2^-55), 1 Taylor, 2 table, 3 1/sqrt, 4 |x| >= 1 (rm_acos's selects)"""
    k = hi32(x)
    return np.select([k < 0x3c880000, k < 0x3fc00000, k < 0x3fef0000, k < 0x3ff00000], [0, 1, 2, 3], 4)


def rows_asncs(x):
    """asncs row of the table band, -1 outside it"""
    k = hi32(x)
    r = np.where(k >= 0x3fe00000, 96 + ((k >> 13) & 0x7f), np.where(k >= 0x3fd00000, 32 + ((k >> 14) & 0x3f), (k >> 15) & 0x1f))
    return np.where((k >= 0x3fc00000) & (k < 0x3fef0000), np.minimum(r, 215), -1)


def rows_inroot(x):
    """inroot entry of the 1/sqrt band, -1 outside it"""
    ax = np.abs(np.asarray(x, np.float64))
    z = (1.0 - ax) * 0.5
    kz = (u64(z) >> np.uint64(32)).astype(np.int64)
    k = hi32(x)
    return np.where((k >= 0x3fef0000) & (k < 0x3ff00000), (kz >> 14) & 0x7f, -1)


def atan2_quotient(y, x):
    ay, ax = np.abs(np.asarray(y, np.float64)), np.abs(np.asarray(x, np.float64))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        up = np.where((ax < 2.0 ** -500) | (ay < 2.0 ** -500), 2.0 ** 500, 1.0)
        ax, ay = ax * up, ay * up
        dn = np.where((ax > 2.0 ** 500) | (ay > 2.0 ** 500), 2.0 ** -500, 1.0)
        ax, ay = ax * dn, ay * dn
        return np.where(ay < ax, ay / ax, ax / ay)


def bands_atan2(y, x):
    """0 series (u < 1/16), 1 table; + 2 when the quadrant case is not (i) (x > 0, |y| < |x|) -- the four bands that
    rm_atan2<true> gates with its ballots (finite, non-zero operands)"""
    u = atan2_quotient(y, x)
    ay, ax = np.abs(y), np.abs(x)
    case_i = (np.asarray(x) > 0) & (ay < ax)
    return np.where(u < 0.0625, 0, 1) + np.where(case_i, 0, 2)


def rows_cij(y, x):
    """cij row of the table forms (u >= 1/16), -1 for the series"""
    u = atan2_quotient(y, x)
    i = np.rint(u * 256.0).astype(np.int64) - 16     # fma(u, 256, 2^52) - 2^52: u * 256 is exact, then ties to even
    return np.where(u < 0.0625, -1, np.clip(i, 0, 240))


def sincos_reduced(x):
    """(range, a) of rm_sincos for |x| < 105414350: 1 |x| < 0.855469, 2 |x| < 2.426265, 3 reduced; `a` approximates the
    argument of do_sin (sin for range 1 and 3 with n even) -- good to ~1e-16, enough to tell bands and rows apart"""
    x = np.asarray(x, np.float64)
    k = hi32(x)
    rng = np.select([k < 0x3feb6000, k < 0x400368fd], [1, 2], 3)
    n = np.rint(x * (2.0 / np.pi))
    a = np.where(rng == 1, x, np.where(rng == 2, np.pi / 2 - np.abs(x), x - n * (np.pi / 2)))
    return rng, a


# ---- the sets -----------------------------------------------------------------------------------------------------

def _root_of_power_of_two(e, y):
    """2^(e / y) rounded to double (in long double: the rounded exponent e / y alone would be ~50 ulps off)"""
    return float(np.longdouble(2) ** (np.longdouble(e) / np.longdouble(y)))


def _pow_edges():
    xs, ys = [], []

    def add(x, y):
        x = np.asarray(x, np.float64).reshape(-1)
        xs.append(x)
        ys.append(np.broadcast_to(np.asarray(y, np.float64), x.shape))
    for y in (0.5, 2.0, 7.0, 8.0):
        add(nbrs([1.0], 8), y)                                                    # x next to 1
        add(SPECIALS, y)
        add(nbrs([2.0 ** -1022, 2.0 ** -1022 * 3, 1e-300, 1e300, 4.0, 0.25], 2), y)
        if y > 1:
            add(nbrs(_root_of_power_of_two(-1022, y), 4), y)                      # results next to 2^-1022
            add(nbrs(_root_of_power_of_two(1024, y), 4), y)                       # ... and next to overflow
            add(nbrs(np.exp(np.array([-512.0, 512.0, -1024.0, 1024.0, -708.0, 709.0]) / y), 2), y)   # |y log x| cuts
    add(nbrs([2.0 ** -60, 2.0 ** 60, 2.0 ** -59, 2.0 ** 61], 3), 0.5)             # the sparse guard's range
    sub = np.concatenate([f64([1, 2, 3, 0xfffffffffffff, 0x8000000000000, 0x10]), nbrs([1e-310, 1e-320], 2)])
    add(sub, 0.5)                                                                  # subnormal bases
    add(sub, 2.0)
    y_ed = nbrs([2.0 ** -65, 2.0 ** 63, 1.0, 0.5, 2.0], 1)                         # edges of the claimed y range
    for x in (0.5, 2.0, 1.5, 1.0000000000000002):
        add(np.full(len(y_ed), x), y_ed)
    return np.concatenate(xs), np.concatenate(ys)


def _pow_rows():
    """both ends (and the middle) of every row of pow's log table, for each exponent of the path; and every row of the
    exp table: 2^(j/128 + m) as the result, plus the rounding ties between rows"""
    i = np.arange(128, dtype=np.uint64)
    first = np.uint64(POW_LOG_OFF) + (i << np.uint64(45))
    ends = f64(np.concatenate([first, first + np.uint64((1 << 45) - 1), first + np.uint64(1 << 44)]))
    xs, ys = [], []
    for y in (0.5, 2.0, 7.0, 8.0):
        for sc in (1.0, 2.0 ** -3, 2.0 ** 5 if y < 7 else 2.0):
            xs.append(ends * sc)
            ys.append(np.full(len(ends), y))
        j = np.arange(128)
        for m in (-3, 0, 1, 5):
            for off in (0.0, 0.49, -0.49, 0.5):
                xs.append(2.0 ** ((128.0 * m + j + off) / (128.0 * y)))
                ys.append(np.full(128, y))
    return np.concatenate(xs), np.concatenate(ys)


@functools.lru_cache(maxsize=None)
def pow_sets(n=N_RANDOM, seed=21):
    rng = np.random.default_rng(seed)
    sets = {"edges": _pow_edges(), "rows": _pow_rows()}
    for y in (0.5, 2.0, 7.0, 8.0):
        hi = 4.0 if y >= 7 else 1e6
        v = rng.uniform(-4, 4, (n // 4, 3))
        s = (v * v).sum(1)
        x = np.concatenate([rng.uniform(0, hi, n // 4), np.exp(rng.uniform(-40 if y > 1 else -700, np.log(hi), n // 4)),
                            rng.uniform(0.99, 1.01, n // 4), np.minimum(np.sqrt(s), 4.0) if y >= 7 else s])
        sets[f"random_y{y:g}"] = (x, np.full(len(x), y))
    x = np.exp(rng.uniform(-40, 40, n))
    sets["random_xy"] = (x, rng.uniform(0.01, 16.0, n))                            # y off the path's four exponents
    return sets


@functools.lru_cache(maxsize=None)
def pow2_sets(n=N_RANDOM, seed=22):
    rng = np.random.default_rng(seed)
    i = np.arange(128, dtype=np.uint64)
    first = np.uint64(POW_LOG_OFF) + (i << np.uint64(45))
    ends = f64(np.concatenate([first, first + np.uint64((1 << 45) - 1)]))
    edges = np.concatenate([nbrs([1.0], 8), SPECIALS, nbrs([_root_of_power_of_two(-1022, 7), _root_of_power_of_two(-1022, 8)], 4),
                            nbrs([_root_of_power_of_two(1024, 7), _root_of_power_of_two(1024, 8)], 4), nbrs([1e-3, 4.0, 2.0 ** -60], 2),
                            f64([1, 0xfffffffffffff])])
    return {"edges": (edges,), "rows": (np.concatenate([ends, ends * 2.0, ends * 0.125]),),
            "random_uniform": (rng.uniform(0, 4.0, n),), "random_log": (np.exp(rng.uniform(-30, np.log(4.0), n)),)}


@functools.lru_cache(maxsize=None)
def pow_half_sets(n=N_RANDOM, seed=23):
    rng = np.random.default_rng(seed)
    v = rng.uniform(-4, 4, (n, 3))
    edges = np.concatenate([SPECIALS, nbrs([2.0 ** -60, 2.0 ** 60, 1.0, 4.0, 0.25, 2.0 ** -1022], 3),
                            f64([1, 2, 0xfffffffffffff]), nbrs([1e-310], 1), 4.0 ** np.arange(-20, 21)])
    return {"edges": (edges,), "rows": (_pow_rows()[0][:3 * 3 * 128],),
            "random_uniform": (rng.uniform(0, 40.0, n),), "random_squares": ((v * v).sum(1),),
            "random_log": (np.exp(rng.uniform(-60, 8, n)),), "near_midpoint": (near_midpoint_roots(rng, n),)}


@functools.lru_cache(maxsize=None)
def sqrt_sets(n=N_RANDOM, seed=24):
    rng = np.random.default_rng(seed)
    sub = f64(rng.integers(1, 1 << 52, n // 4, dtype=np.uint64))
    edges = np.concatenate([SPECIALS, f64([1, 2, 3, 4, 0xfffffffffffff, 0x7fefffffffffffff]), nbrs([2.0 ** -1022], 3),
                            nbrs([1.7976931348623157e308, 1.0, 4.0, 2.0], 2), 4.0 ** np.arange(-537, 512)])
    return {"edges": (edges,), "random_subnormal": (sub,), "random_log": (np.exp(rng.uniform(-745, 709, n)),),
            "near_midpoint": (near_midpoint_roots(rng, n),)}


SINCOS_THRESHOLDS = [0x3e400000, 0x3e500000, 0x3feb6000, 0x400368fd, 0x419921fb]   # 2^-27, 2^-26, 0.855469, 2.426265, huge


def _sincos_thresholds():
    return both_signs(np.concatenate([nbrs(hiword(SINCOS_THRESHOLDS), 3), SPECIALS,
                                      nbrs([0.126, 0.855469, 2.426265, 105414350.0, 105414300.0, np.pi, np.pi / 2, 1e-9], 3)]))


def _sincos_edges():
    xs = []
    j = np.arange(111, dtype=np.float64)
    xs.append(nbrs(np.concatenate([j / 128, (j + 0.5) / 128]), 1))                    # u = big + |a|: row centres and ties
    xs.append(nbrs(np.pi / 2 - np.concatenate([j / 128, (j + 0.5) / 128]), 1))        # ... as do_sin(hp0 - |x|) of range 2
    xs.append(nbrs(np.pi / 2 + np.concatenate([j / 128, (j + 0.5) / 128])[:219], 1))  # (hp0 - |x| < 0 up to -109.5 / 128)
    k = np.arange(1, 4096)
    xs.append(nbrs(np.pi / 2 * k, 1))                                                  # multiples of pi/2 (and below)
    xs.append(nbrs(np.pi / 4 * (2 * k + 1), 1))                                        # x hpinv + toint on a tie
    xs.append(nbrs(np.pi / 2 * k + 0.126, 1))                                          # reduced argument at the Taylor cut
    xs.append(nbrs(np.pi / 2 * k - 0.126, 1))
    return both_signs(np.concatenate(xs))


def _sincos_multiples():
    """k pi/2 for every k <= 2^20 and its neighbours (the reduction's cancellation), odd multiples of pi/4 up to 2^17
    (x hpinv + toint on a rounding tie)"""
    k = np.arange(1, 2 ** 20 + 1)
    return both_signs(np.concatenate([nbrs(np.pi / 2 * k, 1), nbrs(np.pi / 4 * (2 * k[:2 ** 16] + 1), 1)]))


@functools.lru_cache(maxsize=None)
def sincos_sets(n=N_RANDOM, seed=25):
    rng = np.random.default_rng(seed)
    return {"thresholds": (_sincos_thresholds(),), "edges": (_sincos_edges(),), "multiples": (_sincos_multiples(),),
            "random_8pi": (rng.uniform(-8 * np.pi, 8 * np.pi, n),), "random_small": (rng.uniform(-0.2, 0.2, n),),
            "random_3": (rng.uniform(-3, 3, n),), "random_400": (rng.uniform(-400, 400, n),),
            "random_1e8": (rng.uniform(-1.1e8, 1.1e8, n),),
            "random_log": (np.exp(rng.uniform(-40, 3, n)) * rng.choice([-1, 1], n),)}


ACOS_THRESHOLDS = [0x3c880000, 0x3fc00000, 0x3fd00000, 0x3fe00000, 0x3fef0000, 0x3ff00000]


def _acos_rows():
    ks = np.concatenate([0x3fc00000 + (np.arange(33) << 15), 0x3fd00000 + (np.arange(65) << 14),
                         0x3fe00000 + (np.arange(121) << 13)])
    first = hiword(ks)
    xs = [first, np.nextafter(first, 0), np.nextafter(first, 2), hiword(ks + 1)]      # both ends of every row
    # inroot: z = (1 - |x|) / 2 with bits 14..20 of its high word = the entry (bit 20: the exponent's parity)
    idx = np.arange(128)
    for e in (1014, 1008, 990):                   # biased exponents <= 1015: z < 2^-6, |x| > 0.96875
        kz = ((e + (idx >> 6)) << 20) | ((idx & 0x3f) << 14)
        z = hiword(kz)
        xs += [1.0 - 2.0 * z, 1.0 - 2.0 * np.nextafter(z, 1)]
    return both_signs(np.concatenate(xs))


@functools.lru_cache(maxsize=None)
def acos_sets(n=N_RANDOM, seed=26):
    rng = np.random.default_rng(seed)
    edges = both_signs(np.concatenate([nbrs(hiword(ACOS_THRESHOLDS), 3), nbrs([0.125, 0.25, 0.5, 0.96875, 1.0, 2.7e-17], 2),
                                       SPECIALS, [2.0, 1e300]]))
    v = rng.normal(size=(n, 3))
    return {"edges": (edges,), "rows": (_acos_rows(),), "random_uniform": (rng.uniform(-1, 1, n),),
            "random_near1": (both_signs(1.0 - np.exp(rng.uniform(-40, -3, n // 2))),),
            "random_eighth": (rng.uniform(-0.13, 0.13, n),),
            "random_log": (np.exp(rng.uniform(-60, 0, n)) * rng.choice([-1, 1], n),),
            "random_callsite": (np.clip(v[:, 2] / np.sqrt((v * v).sum(1)), -1, 1),)}


def _atan2_edges():
    ys, xs = [], []

    def add(y, x):
        y, x = np.broadcast_arrays(np.asarray(y, np.float64).reshape(-1), np.asarray(x, np.float64).reshape(-1))
        qy, qx = quadrants(y, x)
        ys.extend([qy, qx])                    # and swapped: |y| > |x| takes the pi/2 -+ atan cases
        xs.extend([qx, qy])
    add(nbrs([0.0625], 4), 1.0)                                                     # the quotient at 1/16
    add(nbrs([0.0625 * 3.0, 0.0625 * 1e-200, 0.0625 * 1e200], 2), np.tile([3.0, 1e-200, 1e200], 5))
    for g in (55, 56, 57, 58, 59):                                                  # exponent gaps around the 57 cut
        for m1, m2 in ((1.0, 1.0), (1.0, 1.9999999999999998), (1.9999999999999998, 1.0), (1.5, 1.25)):
            add(m1 * 2.0 ** np.array([0, -300, 400, -900]), m2 * 2.0 ** (np.array([0, -300, 400, -900]) + g))
    edge = nbrs([2.0 ** -500, 2.0 ** 500, 2.0 ** -499, 2.0 ** 499], 2)              # the rescaling of e_atan2.c
    for other in (1.0, 2.0 ** -500, 2.0 ** 500, 2.0 ** -560, 2.0 ** 560, 3.0 * 2.0 ** -520):
        add(edge, other)
    z = np.array([0.0, -0.0])
    add(np.repeat(z, 6), np.tile([0.0, -0.0, 1.0, -1.0, 1e-300, 1e300], 2))         # signed zeros
    add(np.array([1.0, 1e-300, 5e-324, 1e300]), 0.0)
    add(np.array([np.inf, np.nan, 1.0]), np.array([1.0, 1.0, np.nan]))               # non-finite: unclaimed, NaN
    return np.concatenate(ys), np.concatenate(xs)


def _atan2_rows():
    j = np.arange(241, dtype=np.float64)
    u = np.concatenate([(j + 16) / 256, nbrs((j + 15.5) / 256, 1), np.nextafter((j + 16.5) / 256, 0)])
    u = u[(u >= 0.0625) & (u <= 1.0)]
    ys, xs = [], []
    for d in (1.0, 3.0, 2.0 ** -40):
        qy, qx = quadrants(u * d, np.full(len(u), d))
        ys += [qy, qx]
        xs += [qx, qy]
    return np.concatenate(ys), np.concatenate(xs)


@functools.lru_cache(maxsize=None)
def atan2_sets(n=N_RANDOM, seed=27):
    rng = np.random.default_rng(seed)

    def sg(k):
        return rng.choice([-1, 1], k)
    return {"edges": _atan2_edges(), "rows": _atan2_rows(),
            "random_uniform": (rng.uniform(-4, 4, n), rng.uniform(-4, 4, n)),
            "random_normal": (rng.normal(size=n), rng.normal(size=n)),
            "random_log30": (np.exp(rng.uniform(-30, 30, n)) * sg(n), np.exp(rng.uniform(-30, 30, n)) * sg(n)),
            "random_log700": (np.exp(rng.uniform(-700, 700, n)) * sg(n), np.exp(rng.uniform(-700, 700, n)) * sg(n)),
            "random_small_y": (rng.uniform(-1, 1, n) * 1e-3, rng.uniform(-4, 4, n))}


def _log_rows():
    i = np.arange(128, dtype=np.uint64)
    xs = []
    for k in (1, -2, 40, -600):
        base = np.uint64(LOG_OFF) + (i << np.uint64(45))
        kk = np.uint64(abs(k) << 52)
        b = base + kk if k > 0 else base - kk
        xs += [f64(b), f64(b + np.uint64((1 << 45) - 1))]
    x = np.concatenate(xs)
    return np.concatenate([x, x[:256] * 2.0 ** -1040])         # the same rows reached through subnormal arguments


@functools.lru_cache(maxsize=None)
def log_sets(n=N_RANDOM, seed=28):
    rng = np.random.default_rng(seed)
    edges = np.concatenate([nbrs(f64([LOG_NEAR1_LO, LOG_NEAR1_LO + LOG_NEAR1_SPAN, LOG_OFF]), 3),
                            nbrs([1.0, 2.0 ** -1022, 0.9375, 1.0644, 1e-12, 4.0], 3), SPECIALS,
                            f64([1, 2, 3, 0xfffffffffffff, 0x8000000000000]), nbrs([1e-310, 1e-320], 2), [-2.0, -1e-300]])
    return {"edges": (edges,), "rows": (_log_rows(),), "random_uniform": (rng.uniform(1e-12, 7e4, n),),
            "random_log": (np.exp(rng.uniform(-740, 700, n)),), "random_near1": (rng.uniform(0.9, 1.1, n),),
            "random_subnormal": (f64(rng.integers(1, 1 << 52, n // 8, dtype=np.uint64)),)}


FAMILY_SETS = {"pow": pow_sets, "pow2": pow2_sets, "pow_half": pow_half_sets, "sqrt": sqrt_sets, "sincos": sincos_sets,
               "acos": acos_sets, "atan2": atan2_sets, "log": log_sets}
# the device routine (include/rm_hip.h RmMathFn) -> its argument family
FN_FAMILY = {"POW": "pow", "POW2": "pow2", "POW_HALF_DENSE": "pow_half", "POW_HALF_SPARSE": "pow_half",
             "POW_HALF_GUARD": "pow_half", "SQRT": "sqrt", "SIN": "sincos", "COS": "sincos", "SINCOS": "sincos",
             "SINCOS_U": "sincos", "ACOS": "acos", "ACOS_U": "acos", "ATAN2": "atan2", "ATAN2_U": "atan2", "LOG": "log"}


# ---- host counterparts (tests/native/math_check.cpp) --------------------------------------------------------------

_DP = ctypes.POINTER(ctypes.c_double)


def _p(a):
    return a.ctypes.data_as(_DP)


def host_eval(L, fn, a, b=None):
    """the host restatement of device routine `fn` (RmMathFn name): (out0, out1 or None).  POW_HALF_*: rm_pow(x, 0.5),
    which both device forms must return; POW_HALF_GUARD: the rounded root and the guard's verdict (1.0 / 0.0)."""
    a = np.ascontiguousarray(a, np.float64)
    n = len(a)
    o0, o1 = np.empty(n), None

    def one(name, *args):
        getattr(L, name)(*[_p(x) for x in args[:-1]], ctypes.c_size_t(n), _p(args[-1]))
    if fn == "POW":
        one("rmc_pow", a, np.ascontiguousarray(b, np.float64), o0)
    elif fn == "POW2":
        o1 = np.empty(n)
        L.rmc_pow2(_p(a), ctypes.c_size_t(n), ctypes.c_double(7.0), ctypes.c_double(8.0), _p(o0), _p(o1))
    elif fn in ("POW_HALF_DENSE", "POW_HALF_SPARSE"):
        one("rmc_pow", a, np.full(n, 0.5), o0)
    elif fn == "POW_HALF_GUARD":
        safe = np.empty(n, np.uint8)
        L.rmc_pow_half_guard(_p(a), ctypes.c_size_t(n), _p(o0), safe.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)))
        o1 = safe.astype(np.float64)
    elif fn in ("SINCOS", "SINCOS_U"):
        o1 = np.empty(n)
        getattr(L, "rmc_sincos" if fn == "SINCOS" else "rmc_sincos_u")(_p(a), ctypes.c_size_t(n), _p(o0), _p(o1))
    elif fn in ("ATAN2", "ATAN2_U"):
        one("rmc_atan2" if fn == "ATAN2" else "rmc_atan2_u", a, np.ascontiguousarray(b, np.float64), o0)
    else:
        one({"SQRT": "rmc_sqrt", "SIN": "rmc_sin", "COS": "rmc_cos", "ACOS": "rmc_acos", "ACOS_U": "rmc_acos_u",
             "LOG": "rmc_log"}[fn], a, o0)
    return o0, o1


# ---- claimed domains and a reference independent of glibc ---------------------------------------------------------

def claimed(fn, a, b=None):
    """where csrc/rm_math_*.h claims glibc's bits (STATUS comments) -- and so an error below 1 ulp"""
    a = np.asarray(a, np.float64)
    fin = np.isfinite(a)
    with np.errstate(all="ignore"):
        if fn in ("POW", "POW2"):
            y = np.asarray(b, np.float64) if fn == "POW" else None
            pos = fin & (a > 0)
            if fn == "POW2":
                return pos & (np.abs(8.0 * np.log(np.where(pos, a, 1.0))) < 512)
            ok = pos & (y >= 2.0 ** -65) & (y < 2.0 ** 63)
            return ok & (np.abs(y * np.log(np.where(pos, a, 1.0))) < 512)         # |y log x| < 512: results 2^-738 .. 2^738
        if fn.startswith("POW_HALF") or fn == "SQRT":
            return fin & (a >= 0) & ~np.signbit(a)
        if fn.startswith(("SIN", "COS")):
            return fin & (hi32(a) < 0x419921fb)                                     # |x| < 0x1.921fbp+26 = 105414336
        if fn.startswith("ACOS"):
            return np.abs(a) <= 1.0
        if fn.startswith("ATAN2"):
            y, x = a, np.asarray(b, np.float64)
            ok = np.isfinite(x) & np.isfinite(y) & (x != 0) & (y != 0)
            return ok & (np.abs(np.arctan2(y, x)) >= 2.0 ** -1021)                # subnormal quotients are unclaimed
        if fn == "LOG":
            return fin & (a > 0)
    raise KeyError(fn)


def true_values(fn, a, b=None, prec=200):
    """the exact value of the routine at each argument, to `prec` bits (mpmath): a list of mpf, or of (mpf, mpf) for the
    two-result routines"""
    import mpmath
    mp = mpmath.mp
    out = []
    with mpmath.workprec(prec):
        for i, ai in enumerate(np.asarray(a, np.float64)):
            x = mp.mpf(float(ai))
            if fn == "POW":
                out.append(mp.power(x, mp.mpf(float(b[i]))))
            elif fn == "POW2":
                out.append((mp.power(x, 7), mp.power(x, 8)))
            elif fn.startswith("POW_HALF") or fn == "SQRT":
                out.append(mp.sqrt(x))
            elif fn in ("SIN", "COS"):
                out.append(mp.sin(x) if fn == "SIN" else mp.cos(x))
            elif fn.startswith("SINCOS"):
                out.append((mp.sin(x), mp.cos(x)))
            elif fn.startswith("ACOS"):
                out.append(mp.acos(x))
            elif fn.startswith("ATAN2"):
                out.append(mp.atan2(x, mp.mpf(float(b[i]))))
            elif fn == "LOG":
                out.append(mp.log(x))
    return out


def bracket_errors(got, truth):
    """for each double in `got` and exact value in `truth`: (is it one of the two doubles around the exact value, its
    error in ulps of that value)"""
    import mpmath
    ok, err = np.zeros(len(got), bool), np.zeros(len(got))
    with mpmath.workprec(300):
        for i, (g, t) in enumerate(zip(np.asarray(got, np.float64), truth)):
            r = float(t)                               # nearest double
            if mpmath.mpf(r) == t:
                allowed = {r}
            elif mpmath.mpf(r) < t:
                allowed = {r, float(np.nextafter(r, np.inf))}
            else:
                allowed = {float(np.nextafter(r, -np.inf)), r}
            ok[i] = float(g) in allowed
            sp = float(np.spacing(abs(r))) if r != 0 else 5e-324
            err[i] = float(abs(mpmath.mpf(float(g)) - t) / sp) if np.isfinite(g) else np.inf
    return ok, err
