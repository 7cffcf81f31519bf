// Host-only check build of the sound segment tracer (csrc/rm_segment.h) -- compiled by g++ for tests ONLY, so the exact
// source the gfx950 kernels are built from can be compared with the reference's fixtures, with the interval oracle and
// with the device in a container without a GPU.  Never loaded by the product.
#include <stddef.h>
#include <stdint.h>
#include "../../raymarch_algo_compare_amd/csrc/rm_segment.h"

using namespace rm;

namespace {
thread_local ProgramImage g_img;

int encode(const RmSceneOp* ops, int32_t nops, char* why, int why_len)
{
    return program_encode(ops, nops, &g_img, why, (size_t)why_len) ? 0 : -1;
}
}  // namespace

extern "C" {

// program_eval_dual over n segments (segs: n x 8 = origin, direction, t0, t1; out: n x 4 = val.lo, val.hi, der.lo, der.hi)
int rms_eval(const RmSceneOp* ops, int32_t nops, const double* segs, size_t n, double* out, char* why, int why_len)
{
    if (encode(ops, nops, why, why_len)) return -1;
    const ProgSrc src{ &g_img };
    for (size_t i = 0; i < n; ++i) {
        const double* s = segs + 8 * i;
        const vec3 o = v3(s[0], s[1], s[2]), d = v3(s[3], s[4], s[5]);
        const DIval r = program_eval_dual(src, seed_segment(o, d, s[6], s[7]), d);
        out[4 * i] = r.val.lo; out[4 * i + 1] = r.val.hi; out[4 * i + 2] = r.der.lo; out[4 * i + 3] = r.der.hi;
    }
    return 0;
}

// program_eval_interval over the boxes of the same segments (out: n x 2), and interval_point at o + t0 * d (pt: n)
int rms_eval_interval(const RmSceneOp* ops, int32_t nops, const double* segs, size_t n, double* out, double* pt, char* why,
                      int why_len)
{
    if (encode(ops, nops, why, why_len)) return -1;
    const ProgSrc src{ &g_img };
    for (size_t i = 0; i < n; ++i) {
        const double* s = segs + 8 * i;
        const vec3 o = v3(s[0], s[1], s[2]), d = v3(s[3], s[4], s[5]);
        const Ival r = program_eval_interval(src, seed_segment(o, d, s[6], s[7]));
        out[2 * i] = r.lo; out[2 * i + 1] = r.hi;
        pt[i] = interval_point(src, o.x + s[6] * d.x, o.y + s[6] * d.y, o.z + s[6] * d.z);
    }
    return 0;
}

// segment_trace over n rays
int rms_march(const RmSceneOp* ops, int32_t nops, const RmSegmentConfig* cfg, const double* o, const double* d, size_t n,
              double* t, int32_t* iters, double* cursor, char* why, int why_len)
{
    if (encode(ops, nops, why, why_len)) return -1;
    SegmentParams P;
    if (!segment_resolve(cfg, -1.0, &P, why, (size_t)why_len)) return -2;
    const ProgSrc src{ &g_img };
    for (size_t i = 0; i < n; ++i)
        t[i] = segment_trace(src, v3(o[3 * i], o[3 * i + 1], o[3 * i + 2]), v3(d[3 * i], d[3 * i + 1], d[3 * i + 2]), P, &iters[i],
                             &cursor[i]);
    return 0;
}

// faithful_capture of rows [row0, row0 + rows) with the library's camera; scene_bound as interval_scene_bound gives it
int rms_render(const RmSceneOp* ops, int32_t nops, const RmSegmentConfig* cfg, double scene_bound, const double* cam14, int width,
               int height, int row0, int rows, double* depth, uint8_t* hit, int32_t* iters, double* cursor, char* why, int why_len)
{
    if (encode(ops, nops, why, why_len)) return -1;
    SegmentParams P;
    if (!segment_resolve(cfg, scene_bound, &P, why, (size_t)why_len)) return -2;
    CameraParams cam;
    for (int i = 0; i < 14; ++i) cam.v[i] = cam14[i];
    const ProgSrc src{ &g_img };
    for (int y = 0; y < rows; ++y)
        for (int x = 0; x < width; ++x) {
            const size_t i = (size_t)y * width + x;
            segment_pixel(src, cam, width, height, x, row0 + y, P, &depth[i], &hit[i], &iters[i], &cursor[i]);
        }
    return 0;
}

// segment_resolve alone: 0, or -2 with the reason; the resolved constants in out[10] (budget last)
int rms_resolve(const RmSegmentConfig* cfg, double scene_bound, double* out, char* why, int why_len)
{
    SegmentParams P;
    if (!segment_resolve(cfg, scene_bound, &P, why, (size_t)why_len)) return -2;
    const double v[10] = { P.t_max, P.tol, P.h0, P.kappa, P.h_min, P.h_max, P.k_min, P.l_global, P.bound, (double)P.budget };
    for (int i = 0; i < 10; ++i) out[i] = v[i];
    return 0;
}

double rms_scene_bound(int id) { return interval_scene_bound(id); }

size_t rms_sizeof_config(void) { return sizeof(RmSegmentConfig); }
size_t rms_offsetof_config(int field)
{
    switch (field) {
        case 0: return offsetof(RmSegmentConfig, t_max);
        case 1: return offsetof(RmSegmentConfig, tol);
        case 2: return offsetof(RmSegmentConfig, h0);
        case 3: return offsetof(RmSegmentConfig, kappa);
        case 4: return offsetof(RmSegmentConfig, h_min);
        case 5: return offsetof(RmSegmentConfig, h_max);
        case 6: return offsetof(RmSegmentConfig, k_min);
        case 7: return offsetof(RmSegmentConfig, l_global);
        case 8: return offsetof(RmSegmentConfig, bound_radius);
        case 9: return offsetof(RmSegmentConfig, budget);
        case 10: return offsetof(RmSegmentConfig, reserved);
    }
    return (size_t)-1;
}

}
