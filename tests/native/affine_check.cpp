// Host-only check build of the affine range (csrc/rm_affine.h) -- compiled by g++ for tests ONLY, so the exact source the
// gfx950 kernels are built from can be compared with the reference's fixtures, with the interval oracle, with the
// pointwise interpreter and with the device in a container without a GPU.  Never loaded by the product.
#include <stddef.h>
#include <stdint.h>
#include "../../raymarch_algo_compare_amd/csrc/rm_affine.h"

using namespace rm;

namespace {
thread_local ProgramImage g_img;

int encode(const RmSceneOp* ops, int32_t nops, char* why, int why_len)
{
    return program_encode(ops, nops, &g_img, why, (size_t)why_len) ? 0 : -1;
}

int resolve(int mode, const RmIntervalConfig* cfg, double scene_bound, IntervalParams* P, char* why, int why_len)
{
    if (!affine_mode_ok(mode)) return snprintf(why, (size_t)why_len, "mode %d is no range mode", mode), -3;
    return interval_resolve(cfg, scene_bound, P, why, (size_t)why_len) ? 0 : -2;
}
}  // namespace

extern "C" {

// affine_range over n segments (segs: n x 8 = origin, direction, t0, t1; out_range: n x 2 = lo, hi; out_form: n x 3 = x0,
// x1, e, or NULL)
int rma_range(const RmSceneOp* ops, int32_t nops, int mode, const double* segs, size_t n, double* out_range, double* out_form,
              char* why, int why_len)
{
    if (encode(ops, nops, why, why_len)) return -1;
    if (!affine_mode_ok(mode)) return snprintf(why, (size_t)why_len, "mode %d is no range mode", mode), -3;
    const ProgSrc src{ &g_img };
    for (size_t i = 0; i < n; ++i) {
        const double* s = segs + 8 * i;
        Aff f;
        const Ival r = affine_range(src, mode, v3(s[0], s[1], s[2]), v3(s[3], s[4], s[5]), s[6], s[7], &f);
        out_range[2 * i] = r.lo; out_range[2 * i + 1] = r.hi;
        if (out_form) { out_form[3 * i] = f.x0; out_form[3 * i + 1] = f.x1; out_form[3 * i + 2] = f.e; }
    }
    return 0;
}

// program_eval_interval over the boxes of the same segments (out: n x 2)
int rma_interval(const RmSceneOp* ops, int32_t nops, const double* segs, size_t n, double* out, char* why, int why_len)
{
    if (encode(ops, nops, why, why_len)) return -1;
    const ProgSrc src{ &g_img };
    for (size_t i = 0; i < n; ++i) {
        const double* s = segs + 8 * i;
        const Ival r = program_eval_interval(src, seed_segment(v3(s[0], s[1], s[2]), v3(s[3], s[4], s[5]), s[6], s[7]));
        out[2 * i] = r.lo; out[2 * i + 1] = r.hi;
    }
    return 0;
}

// affine_first_hit over n rays; mode 0: interval_first_hit (the interval oracle's march, for the comparison)
int rma_march(const RmSceneOp* ops, int32_t nops, int mode, const RmIntervalConfig* cfg, const double* o, const double* d, size_t n,
              double* t, int32_t* steps, char* why, int why_len)
{
    if (encode(ops, nops, why, why_len)) return -1;
    IntervalParams P;
    if (int rc = resolve(mode == 0 ? RM_RANGE_AFFINE : mode, cfg, -1.0, &P, why, why_len)) return rc;
    const ProgSrc src{ &g_img };
    for (size_t i = 0; i < n; ++i) {
        const vec3 oo = v3(o[3 * i], o[3 * i + 1], o[3 * i + 2]), dd = v3(d[3 * i], d[3 * i + 1], d[3 * i + 2]);
        t[i] = mode == 0 ? interval_first_hit(src, oo, dd, P, &steps[i]) : affine_first_hit(src, mode, oo, dd, P, &steps[i]);
    }
    return 0;
}

// _capture of rows [row0, row0 + rows) with the library's camera; scene_bound as interval_scene_bound gives it; mode 0:
// the interval oracle's capture (interval_pixel without normals)
int rma_render(const RmSceneOp* ops, int32_t nops, int mode, const RmIntervalConfig* cfg, double scene_bound, const double* cam14,
               int width, int height, int row0, int rows, double* depth, uint8_t* hit, int32_t* steps, char* why, int why_len)
{
    if (encode(ops, nops, why, why_len)) return -1;
    IntervalParams P;
    if (int rc = resolve(mode == 0 ? RM_RANGE_AFFINE : mode, cfg, scene_bound, &P, why, why_len)) return rc;
    CameraParams cam;
    for (int i = 0; i < 14; ++i) cam.v[i] = cam14[i];
    const ProgSrc src{ &g_img };
    for (int y = 0; y < rows; ++y)
        for (int x = 0; x < width; ++x) {
            const size_t i = (size_t)y * width + x;
            if (mode == 0) {
                vec3 nv;
                interval_pixel(src, cam, width, height, x, row0 + y, P, false, &depth[i], &hit[i], &nv, &steps[i]);
            } else {
                affine_pixel(src, mode, cam, width, height, x, row0 + y, P, &depth[i], &hit[i], &steps[i]);
            }
        }
    return 0;
}

double rma_scene_bound(int id) { return interval_scene_bound(id); }

}
