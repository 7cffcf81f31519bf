"""Inputs for the capture-scoring tests (csrc/rm_score.h): tests/test_score_host.py feeds them to the host build and
tests/test_gpu_score.py to the device.  Seeded NumPy, nothing larger than 65 x 17 or 48 x 36.

A case is (name, method, reference, band_k); a capture is a dict of "hit" (uint8, any non-zero byte = hit), "depth" and
optionally "normal" (H, W, 3), float32 or float64 -- the dtype is what the call is told (RmScoreMaps.fp64).  What the cases
cover is listed where they are built; cases() returns them all, built once.
"""
import collections
import struct

import numpy as np

Case = collections.namedtuple("Case", "name method reference band_k")

SHAPES = [(1, 1), (9, 1), (1, 9), (31, 7), (32, 8), (33, 9), (64, 16), (65, 17), (48, 36)]      # (W, H); tiles are 32 x 8
COHIT_COUNTS = [0, 1, 2, 20, 21, 22]
BANDS = [-1, 0, 1, 2, 8]


def capture(W, H, seed, dtype=np.float32, normal=True, fill=None):
    """a blob of hits with speckle (or a random mask of density `fill`), depths near 3, unit normals"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    if fill is None:
        cx, cy = W * rng.uniform(0.3, 0.7), H * rng.uniform(0.3, 0.7)
        hit = ((xx - cx) / (0.45 * W + 0.5)) ** 2 + ((yy - cy) / (0.45 * H + 0.5)) ** 2 < 1.0
        hit ^= rng.random((H, W)) < 0.04
    else:
        hit = rng.random((H, W)) < fill
    n = rng.normal(0.0, 1.0, (H, W, 3))
    c = {"hit": hit.astype(np.uint8), "depth": (3.0 + rng.normal(0.0, 0.2, (H, W))).astype(dtype)}
    if normal:
        c["normal"] = (n / np.linalg.norm(n, axis=2, keepdims=True)).astype(dtype)
    return c


def near(c, seed, scale=0.01):
    """a method capture close to `c`: a few flipped hits, perturbed depths and normals, same dtypes"""
    rng = np.random.default_rng(seed)
    H, W = c["hit"].shape
    m = {"hit": c["hit"] ^ (rng.random((H, W)) < 0.08).astype(np.uint8),
         "depth": (c["depth"].astype(np.float64) + rng.normal(0.0, scale, (H, W))).astype(c["depth"].dtype)}
    if "normal" in c:
        n = c["normal"].astype(np.float64) + rng.normal(0.0, 0.05, (H, W, 3))
        m["normal"] = (n / np.linalg.norm(n, axis=2, keepdims=True)).astype(c["normal"].dtype)
    return m


def with_gaps(W, H, gaps, seed, ref_depth=1.0):
    """(method, reference) in float64 whose co-hit pixels are len(gaps) random pixels with exactly these depth gaps, in
    random order; both also hit pixels the other misses"""
    rng = np.random.default_rng(seed)
    order = rng.permutation(W * H)
    n = len(gaps)
    spare = (W * H - n) // 3
    r_hit, m_hit = np.zeros(W * H, np.uint8), np.zeros(W * H, np.uint8)
    r_hit[order[:n + spare]] = 1
    m_hit[order[:n]] = 1
    m_hit[order[n + spare:n + 2 * spare]] = 1
    r_depth = np.full(W * H, ref_depth)
    m_depth = rng.uniform(1.0, 5.0, W * H)
    m_depth[order[:n]] = ref_depth + rng.permutation(np.asarray(gaps, np.float64))
    m_normal = np.tile([0.0, 0.6, 0.8], (W * H, 1))
    r_normal = np.tile([0.0, 0.0, 1.0], (W * H, 1))
    return ({"hit": m_hit.reshape(H, W), "depth": m_depth.reshape(H, W), "normal": m_normal.reshape(H, W, 3)},
            {"hit": r_hit.reshape(H, W), "depth": r_depth.reshape(H, W), "normal": r_normal.reshape(H, W, 3)})


def _build():
    out = []
    add = lambda name, m, r, k=2: out.append(Case(name, m, r, k))      # noqa: E731

    # every shape: a float32 method against a float64 reference (what a sweep frame against an oracle capture is)
    for i, (W, H) in enumerate(SHAPES):
        r = capture(W, H, 100 + i, np.float64)
        m = near(capture(W, H, 100 + i, np.float32), 200 + i)
        add(f"{W}x{H} blob", m, r)
        dense = capture(W, H, 300 + i, np.float64, fill=0.7)
        add(f"{W}x{H} random mask", near(dense, 400 + i), dense)

    # co-hit counts around the ranks of the 95th percentile (n = 21: g = 0; n = 22: j + 1 = n - 1), and every pixel
    W, H = 33, 9
    rng = np.random.default_rng(7)
    for n in COHIT_COUNTS:
        m, r = with_gaps(W, H, rng.uniform(-0.5, 0.5, n), 500 + n)
        add(f"{n} co-hit pixels", m, r)
    full = capture(W, H, 11, np.float64)
    full["hit"][:] = 1
    m = near(full, 12)
    m["hit"][:] = 1
    add("all pixels co-hit", m, full)

    # ties and zeros; n = 22: the p95 ranks are 19 / 20, the median's 10 / 11
    base = [0.01 * (i + 1) for i in range(22)]
    tie = lambda a, b: [base[a] if i == b else v for i, v in enumerate(base)]      # noqa: E731
    for name, gaps in (("all gaps equal", [0.25] * 22), ("tie at ranks 19 / 20", tie(19, 20)), ("tie at ranks 18 / 19", tie(18, 19)),
                       ("tie at ranks 20 / 21", tie(20, 21)), ("tie at ranks 10 / 11", tie(10, 11)),
                       ("ties on both sides of the ranks", [0.1] * 10 + [0.2] * 10 + [0.3] * 2),
                       ("tie of 21 pixels, g = 0", [0.5] * 20 + [0.75])):
        m, r = with_gaps(W, H, gaps, 600 + len(out))
        add(name, m, r)
    r = capture(W, H, 13, np.float64)
    add("method = reference", {k: v.copy() for k, v in r.items()}, r)
    m, r = with_gaps(W, H, [0.0] * 22, 14, ref_depth=0.0)
    m["depth"] = np.where(m["hit"] & r["hit"], -0.0, m["depth"])
    add("gaps of -0.0", m, r)

    # extreme values
    m, r = with_gaps(W, H, [5e-324, 1e-310, 2.5e-308, 1e300, 0.5, 0.25] + [0.125] * 16, 15, ref_depth=0.0)
    add("subnormals and 1e300", m, r)
    m, r = with_gaps(W, H, [0.1] * 20 + [np.inf, -np.inf], 16)
    add("infinite gaps", m, r)
    m, r = with_gaps(W, H, [0.1] * 22, 17)
    co = np.argwhere(m["hit"] & r["hit"])
    m["depth"][tuple(co[0])] = r["depth"][tuple(co[0])] = np.inf
    add("inf - inf", m, r)
    m, r = with_gaps(W, H, [0.1 * i for i in range(22)], 18)
    co = np.argwhere(m["hit"] & r["hit"])
    m["depth"][tuple(co[5])] = np.nan
    add("NaN depth on a co-hit pixel", m, r)
    m, r = with_gaps(W, H, [0.1 * i for i in range(22)], 19)
    m["depth"][tuple(np.argwhere(m["hit"] & ~r["hit"].astype(bool))[0])] = np.nan
    r["depth"][tuple(np.argwhere(r["hit"] & ~m["hit"].astype(bool))[0])] = np.nan
    r["depth"][tuple(np.argwhere((m["hit"] | r["hit"]) == 0)[0])] = np.nan
    add("NaN depth on pixels that are not co-hit", m, r)

    # normals
    r = capture(W, H, 21, np.float64)
    m = near(r, 22)
    co = np.argwhere(m["hit"] & r["hit"])
    m["normal"][tuple(co[3])] = [np.nan, 0.0, 1.0]
    add("NaN normal on a co-hit pixel", m, r)
    r = capture(W, H, 23, np.float64)
    m = near(r, 24)
    m["normal"] *= 3.0
    add("normals of length 3", m, r)
    m = near(r, 25)
    m["normal"] *= 0.5
    add("normals of length 1/2", m, r)
    one = np.zeros((H, W, 3))
    one[..., 0] = 1.0
    r = dict(capture(W, H, 26, np.float64), normal=one.copy())
    add("cosine exactly 1", dict(near(r, 27), normal=one.copy()), r)
    add("cosine exactly -1", dict(near(r, 28), normal=-one), r)
    add("cosine 1 + ulp", dict(near(r, 29), normal=one * np.nextafter(1.0, 2.0)), r)
    add("cosine 1 - ulp", dict(near(r, 30), normal=one * np.nextafter(1.0, 0.0)), r)
    add("cosine -1 - ulp", dict(near(r, 31), normal=-one * np.nextafter(1.0, 2.0)), r)
    r = capture(W, H, 32, np.float64, normal=False)
    add("no normals", near(r, 33), r)

    # any non-zero byte is a hit
    r = capture(W, H, 34, np.float64)
    m = near(r, 35)
    for byte in (1, 2, 255):
        add(f"hit byte {byte}", dict(m, hit=m["hit"] * np.uint8(byte)), dict(r, hit=r["hit"] * np.uint8(byte)))

    # masks: one reference hit in each corner and at each tile seam of a 64 x 16 image, against an all-hit method
    W, H = 64, 16
    everything = capture(W, H, 41, np.float32)
    everything["hit"][:] = 1
    for x, y in ((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (31, 7), (32, 7), (31, 8), (32, 8)):
        r = capture(W, H, 42, np.float64)
        r["hit"][:] = 0
        r["hit"][y, x] = 1
        add(f"one reference hit at ({x}, {y})", everything, r)
    yy, xx = np.mgrid[0:H, 0:W]
    board = ((xx + yy) % 2).astype(np.uint8)
    r = dict(capture(W, H, 43, np.float64), hit=board)
    add("checkerboard against its inverse", dict(near(r, 44), hit=1 - board), r)
    add("checkerboard against all hits", everything, r)
    add("checkerboard against itself", dict(near(r, 45), hit=board.copy()), r)
    add("all-hit reference", near(capture(W, H, 46, np.float64), 47), dict(capture(W, H, 46, np.float64), hit=np.ones((H, W), np.uint8)))
    add("all-miss reference", near(capture(W, H, 48, np.float64), 49), dict(capture(W, H, 48, np.float64), hit=np.zeros((H, W), np.uint8)))
    add("all-miss method", dict(near(capture(W, H, 50, np.float64), 51), hit=np.zeros((H, W), np.uint8)), capture(W, H, 50, np.float64))

    # band widths; 8 is wider than the 9 x 1 and 1 x 9 images and the height of 33 x 9
    for (W, H) in ((48, 36), (33, 9), (9, 1), (1, 9), (65, 17)):
        r = capture(W, H, 60 + W, np.float64)
        m = near(r, 61 + W)
        for k in BANDS:
            add(f"{W}x{H} band_k {k}", m, r, k)

    # float32 / float64 in every combination
    W, H = 33, 9
    r64 = capture(W, H, 71, np.float64)
    m64 = near(r64, 72)
    cast = lambda c, t: {k: (v if k == "hit" else v.astype(t)) for k, v in c.items()}      # noqa: E731
    for mt, rt in ((np.float32, np.float32), (np.float32, np.float64), (np.float64, np.float32), (np.float64, np.float64)):
        add(f"{np.dtype(mt).name} method, {np.dtype(rt).name} reference", cast(m64, mt), cast(r64, rt))
    return out


_cases = None


def cases():
    global _cases
    if _cases is None:
        _cases = _build()
    return _cases


def is_fp64(c):
    """the RmScoreMaps.fp64 flag of a capture: 0 only when depth and normal are both float32"""
    return not (c["depth"].dtype == np.float32 and ("normal" not in c or c["normal"].dtype == np.float32))


def raw_maps(c):
    """(depth, normal or None, hit, fp64) as contiguous arrays of the type the flag says"""
    t = np.float64 if is_fp64(c) else np.float32
    return (np.ascontiguousarray(c["depth"], t), np.ascontiguousarray(c["normal"], t) if "normal" in c else None,
            np.ascontiguousarray(c["hit"], np.uint8), int(is_fp64(c)))


def dump_cases(path):
    """the cases as the stand-alone build of tests/native/score_check.cpp (-DRM_SCORE_CHECK_MAIN) reads them"""
    with open(path, "wb") as f:
        for c in cases():
            H, W = c.reference["hit"].shape
            rd, rn, rh, r64 = raw_maps(c.reference)
            md, mn, mh, m64 = raw_maps(c.method)
            f.write(struct.pack("<7i", W, H, c.band_k, r64, m64, int(rn is not None), 0))
            for a in (rd, rn, rh, md, mn, mh):
                if a is not None:
                    f.write(a.tobytes())
