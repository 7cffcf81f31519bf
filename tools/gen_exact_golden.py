#!/usr/bin/env python3
"""Generate the exact-first-hit fixture under tests/golden/ by RUNNING THE REFERENCE ITSELF.

Runs only in the build container (imports /root/reference, which never travels to the GPU box); writes data only.  The
reference's own gpu/analytic.py intersect_sphere, intersect_plane, intersect_box and intersect_torus are applied to the
library's camera rays (analytic.camera_rays of the camera whose 14 parameters the fixture records), so no reference code
is restated here.

  exact_reference.npz   per case c, key prefix "{c}_":
                        scene   int64 (1,)     catalogue id (0 Sphere, 1 Grazing Plane, 2 Cube, 3 Thin Torus)
                        shape   int64 (2,)     W, H
                        cam     float64 (14,)  position, forward, right, up, half_width, half_height (RmFrameDesc.cam)
                        hit     uint8          packbits of the W x H hit map (row 0 = top)
                        t       float64        depth at the hit pixels, in pixel order
                        n       float64 (., 3) the reference's normal at the hit pixels
                        "cases": the case names, one string joined by ';'.
Cases: the four scenes at 64 x 48 with the default camera ("s0_default" ...), Thin Torus at 128 x 96 ("s3_128x96") and
Thin Torus under each curated viewpoint at 64 x 48 ("s3_vp_<name>").

Usage:  python tools/gen_exact_golden.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

REF = "/root/reference"
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(0, ROOT)

from raymarching_benchmark.gpu import analytic as RA  # noqa: E402

from raymarch_algo_compare_amd import analytic, registry, viewpoints  # noqa: E402
from raymarch_algo_compare_amd.config import RenderConfig  # noqa: E402
from raymarch_algo_compare_amd.interval_oracle import _camera  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "exact_reference.npz")
INTERSECT = {
    0: lambda o, d: RA.intersect_sphere(o, d, 1.0),
    1: lambda o, d: RA.intersect_plane(o, d, (0.0, 1.0, 0.0), -0.5),
    2: lambda o, d: RA.intersect_box(o, d, (1.0, 1.0, 1.0)),
    3: lambda o, d: RA.intersect_torus(o, d, 1.5, 0.05),
}


def main():
    cases = [(f"s{s}_default", s, RenderConfig(width=64, height=48)) for s in range(4)]
    cases.append(("s3_128x96", 3, RenderConfig(width=128, height=96)))
    for vp in viewpoints.viewpoints_for(registry.SCENES[3]):
        cases.append((f"s3_vp_{vp.name}", 3, vp.render_config(64, 48)))
    out = {"cases": np.array(";".join(c[0] for c in cases))}
    for name, sid, rc in cases:
        cam = _camera(rc)
        o, d = analytic.camera_rays(cam)
        depth, hit, normal = INTERSECT[sid](o, d)
        hit = np.asarray(hit, bool)
        out[name + "_scene"] = np.array([sid], np.int64)
        out[name + "_shape"] = np.array([cam.width, cam.height], np.int64)
        out[name + "_cam"] = np.asarray(cam.params14(), np.float64)
        out[name + "_hit"] = np.packbits(hit.reshape(-1))
        out[name + "_t"] = np.asarray(depth, np.float64)[hit]
        out[name + "_n"] = np.asarray(normal, np.float64)[hit]
        print(f"{name}: {int(hit.sum())} hits")
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
