// rm_capture.h -- one pixel of a capture: the tetrahedron normal at the hit point of a marched ray, the shaded colour and
// the float maps GPURunner.capture returns (main.glsl:26-47, :79-110 of the reference's fragment shader, in the CPU
// path's fp64).  Shared by the gfx950 kernel (capture_kernel, rm_kernels.h), the C ABI (rm_capture, rm_shade_frames) and
// the host check build (tests/native/capture_check.cpp): the order of operations is written once, here, so a g++ build
// and the device give the same bits.  Everything is unfused binary64 (-ffp-contract=off); every result is rounded to
// binary32 once, at the end.
//
// Ray: (o, d) = camera_ray(cam, width, height, px, py) -- the very ray the march kernels shoot (rm_camera.h).
// Miss (hit == 0): normal (0, 0, 0); tb = 0.5 * (d.y + 1.0); colour_c = (1.0 - tb) * A_c + tb * B_c with
//   A = (0.06, 0.07, 0.09), B = (0.12, 0.14, 0.18) (the shader's background()).  The scene is not evaluated.
// Hit: p = o + t * d per component (one multiply, one add); f_i = sdf(p + e * k_i), e = 0.0005,
//   k = (1,-1,-1), (-1,-1,1), (-1,1,-1), (1,1,1) (e * k_i is exactly +-0.0005; Scene::sdf is called exactly four times);
//   g_c = ((f_0 k_0c + f_1 k_1c) + f_2 k_2c) + f_3 k_3c;  len = max(rm_sqrt((g_x g_x + g_y g_y) + g_z g_z), 1e-300);
//   n_c = g_c / len (a zero gradient gives the zero normal, never NaN);
//   diff = max((n_x L_x + n_y L_y) + n_z L_z, 0.0);  hemi = 0.5 + 0.5 * n_y;  s = 0.15 * hemi + 0.85 * diff;
//   colour_c = rm_pow(min(max(albedo_c * s, 0.0), 1.0), 0.4545), albedo = (0.82, 0.80, 0.78).
//   rm_pow is exact against glibc on this domain (x in [0, 1], y > 0, normal or zero result: rm_math_pow.h STATUS).
// L, the key light, holds the doubles CPython gives for c / math.sqrt(0.6**2 + 0.7**2 + 0.5**2), c = 0.6, 0.7, 0.5
// (tests/test_capture_host.py recomputes them).
#pragma once

#include <stdint.h>

#include "rm_camera.h"

namespace rm {

constexpr double kCaptureLightX = 0x1.24e7595e85edep-1;   // 0.5720775535473555
constexpr double kCaptureLightY = 0x1.55b892ee46eadp-1;   // 0.6674238124719146
constexpr double kCaptureLightZ = 0x1.e82c3f9d89e1dp-2;   // 0.47673129462279623
constexpr double kCaptureEps = 0.0005;

// normal[3] and color[3] of the pixel (px, py) whose ray ended at parameter t (read only on a hit)
template <class Scene>
RM_HD void capture_shade(const CameraParams& cam, int width, int height, int px, int py, bool hit, double t, float* normal,
                         float* color)
{
    vec3 o, d;
    camera_ray(cam, width, height, px, py, o, d);
    if (!hit) {
        const double tb = 0.5 * (d.y + 1.0);
        const double ta = 1.0 - tb;
        normal[0] = 0.0f; normal[1] = 0.0f; normal[2] = 0.0f;
        color[0] = (float)(ta * 0.06 + tb * 0.12);
        color[1] = (float)(ta * 0.07 + tb * 0.14);
        color[2] = (float)(ta * 0.09 + tb * 0.18);
        return;
    }
    const double e = kCaptureEps;
    const vec3 p = v3(o.x + t * d.x, o.y + t * d.y, o.z + t * d.z);
    const double f0 = Scene::sdf(v3(p.x + e, p.y - e, p.z - e));
    const double f1 = Scene::sdf(v3(p.x - e, p.y - e, p.z + e));
    const double f2 = Scene::sdf(v3(p.x - e, p.y + e, p.z - e));
    const double f3 = Scene::sdf(v3(p.x + e, p.y + e, p.z + e));
    const double gx = ((f0 * 1.0 + f1 * -1.0) + f2 * -1.0) + f3 * 1.0;
    const double gy = ((f0 * -1.0 + f1 * -1.0) + f2 * 1.0) + f3 * 1.0;
    const double gz = ((f0 * -1.0 + f1 * 1.0) + f2 * -1.0) + f3 * 1.0;
    const double len = py_max(rm_sqrt((gx * gx + gy * gy) + gz * gz), 1e-300);
    const double nx = gx / len, ny = gy / len, nz = gz / len;
    const double diff = py_max((nx * kCaptureLightX + ny * kCaptureLightY) + nz * kCaptureLightZ, 0.0);
    const double hemi = 0.5 + 0.5 * ny;
    const double s = 0.15 * hemi + 0.85 * diff;
    normal[0] = (float)nx; normal[1] = (float)ny; normal[2] = (float)nz;
    color[0] = (float)rm_pow(py_min(py_max(0.82 * s, 0.0), 1.0), 0.4545);
    color[1] = (float)rm_pow(py_min(py_max(0.80 * s, 0.0), 1.0), 0.4545);
    color[2] = (float)rm_pow(py_min(py_max(0.78 * s, 0.0), 1.0), 0.4545);
}

// The maps that restate the march result: geom[4] = [hit, iters / max_iterations, t / max_distance, final_sdf]
// (main.glsl:79-84; the divisions in binary64, then rounded), depth = t on a hit and 0 on a miss, the evaluation count.
RM_HD void capture_geom(bool hit, double t, int32_t iters, double final_sdf, int32_t evals, int32_t max_iterations,
                        double max_distance, float* geom, float* depth, float* evals_f)
{
    if (geom) {
        geom[0] = hit ? 1.0f : 0.0f;
        geom[1] = (float)((double)iters / (double)max_iterations);
        geom[2] = (float)(t / max_distance);
        geom[3] = (float)final_sdf;
    }
    if (depth) *depth = hit ? (float)t : 0.0f;
    if (evals_f) *evals_f = (float)evals;
}

}  // namespace rm
