"""Readers of tests/golden/frames_config_<family>.npz and rays_config.npz (oracle/gen_golden.py --only config / rays):
frames and explicit rays the REFERENCE marched away from the default MarchConfig, camera and frame shape.  The frame
files are stored by column (one array per field, one row per case); this module hands them out case by case."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FAMILIES = ("A", "B", "C", "D", "E")
PARAM_ORDER = ["omega", "ar_omega_min", "ar_omega_max", "ar_smoothing", "ar_growth_rate", "ar_decay_rate", "beta",
               "overstep_min_step", "hybrid_stuck_step_ratio", "hybrid_min_step", "margin", "ar_omega_init",
               "overstep_bisection_steps", "hybrid_stuck_threshold", "segment_bisection_steps", "revaa_bisection_steps"]
INT_PARAMS = ("overstep_bisection_steps", "hybrid_stuck_threshold", "segment_bisection_steps", "revaa_bisection_steps")
REFSTATS = ("total_rays", "hit_count", "miss_count", "sample_count", "iteration_min", "iteration_max")
FILES = [f"frames_config_{f}.npz" for f in FAMILIES] + ["rays_config.npz", "frames_config_skipped.json"]

_cache = {}


def _prm(row):
    return {k: (int(v) if k in INT_PARAMS else float(v)) for k, v in zip(PARAM_ORDER, row)}


def family(fam):
    """The cases of one family, in file order: dicts with the frame record of conftest.GoldenFrames.get() (no `depth`)
    plus fam, n, tag, sid, kid, prm, view, t_bits (of the first min(64, rays) rays), sha_depth32 and refstats."""
    if fam in _cache:
        return _cache[fam]
    z = np.load(os.path.join(GOLDEN, f"frames_config_{fam}.npz"))
    cols = {k: z[k] for k in z.files}
    off = cols["off"]
    hit_all = np.unpackbits(cols["hitbits"])[:off[-1]]
    cases = []
    for n in range(len(cols["ids"])):
        meta = cols["meta"][n]
        W, H, row0, rows = (int(meta[i]) for i in range(4))
        assert off[n + 1] - off[n] == rows * W
        cases.append({
            "fam": fam, "n": n, "tag": str(cols["tag"][n]), "sid": int(cols["ids"][n][0]), "kid": int(cols["ids"][n][1]),
            "prm": _prm(cols["prm"][n]), "W": W, "H": H, "row0": row0, "rows": rows, "max_iterations": int(meta[4]),
            "hit_threshold": float(meta[5]), "max_distance": float(meta[6]), "lipschitz": float(meta[7]),
            "cam": cols["cam"][n].copy(), "view": cols["view"][n].copy(),
            "iters": cols["iters"][off[n]:off[n + 1]].astype(np.int32).reshape(rows, W),
            "hit": hit_all[off[n]:off[n + 1]].astype(np.uint8).reshape(rows, W),
            "sha_t": cols["sha_t"][n].tobytes(), "sha_fs": cols["sha_fs"][n].tobytes(),
            "sha_depth32": cols["sha_depth32"][n].tobytes(), "t_bits": cols["t_bits"][n][:min(64, rows * W)].copy(),
            "refstats": None if cols["refstats"][n][0] < 0 else dict(zip(REFSTATS, (int(v) for v in cols["refstats"][n]))),
        })
    _cache[fam] = cases
    return cases


def all_cases():
    return [c for fam in FAMILIES for c in family(fam)]


def label(c):
    return f"{c['fam']}{c['n']} {c['tag']} scene {c['sid']} strategy {c['kid']}"


def ray_pairs():
    """rays_config.npz: dicts with sid, kid, prm, max_iterations, hit_threshold, max_distance, lipschitz, the inputs o, d
    (n, 3) and the reference's hit, iters, t_bits, fs_bits."""
    z = np.load(os.path.join(GOLDEN, "rays_config.npz"))
    out = []
    for n in range(int(z["npairs"][0])):
        p = f"p{n}_"
        meta = z[p + "meta"]
        out.append({"n": n, "sid": int(z[p + "ids"][0]), "kid": int(z[p + "ids"][1]), "prm": _prm(z[p + "prm"]),
                    "max_iterations": int(meta[0]), "hit_threshold": float(meta[1]), "max_distance": float(meta[2]),
                    "lipschitz": float(meta[3]), "o": z[p + "o"], "d": z[p + "d"], "hit": z[p + "hit"], "iters": z[p + "iters"],
                    "t_bits": z[p + "t_bits"], "fs_bits": z[p + "fs_bits"]})
    return out


def skipped():
    with open(os.path.join(GOLDEN, "frames_config_skipped.json"), encoding="utf-8") as f:
        return json.load(f)


def sha_depth32(hit, t):
    """sha256 of the float32 depth map as the reference's RayMarchStats builds it: t where hit, else 0.0."""
    import hashlib
    return hashlib.sha256(np.where(np.asarray(hit).reshape(-1) > 0, np.asarray(t, dtype=np.float64).reshape(-1), 0.0)
                          .astype("<f4").tobytes()).digest()


def first_bad_ray(c, t):
    """Index of the first of the stored rays whose t differs from the reference's, or None."""
    got = np.ascontiguousarray(t, dtype=np.float64).reshape(-1)[:len(c["t_bits"])].view(np.uint64)
    bad = np.nonzero(got != c["t_bits"])[0]
    return int(bad[0]) if len(bad) else None
