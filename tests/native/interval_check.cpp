// Host-only check build of the interval oracle (csrc/rm_interval.h) -- compiled by g++ for tests ONLY, so the exact
// source the gfx950 kernels are built from can be compared with the reference's fixtures, with the pointwise
// interpreter and with the device in a container without a GPU.  Never loaded by the product.
#include <stddef.h>
#include <stdint.h>
#include "../../raymarch_algo_compare_amd/csrc/rm_interval.h"
#include "../../raymarch_algo_compare_amd/csrc/rm_interval_catalogue.h"

using namespace rm;

namespace {
thread_local ProgramImage g_img;

int encode(const RmSceneOp* ops, int32_t nops, char* why, int why_len)
{
    return program_encode(ops, nops, &g_img, why, (size_t)why_len) ? 0 : -1;
}

int params(const RmIntervalConfig* cfg, double scene_bound, IntervalParams* P, char* why, int why_len)
{
    return interval_resolve(cfg, scene_bound, P, why, (size_t)why_len) ? 0 : -1;
}
}  // namespace

extern "C" {

// the catalogue table: the program of scene `id` copied to ops (room for cap ops); its length, 0 without one
int rmi_catalogue(int id, RmSceneOp* ops, int cap)
{
    int32_t n = 0;
    const RmSceneOp* src = interval_catalogue_ops(id, &n);
    if (!src) return 0;
    for (int i = 0; i < n && i < cap; ++i) ops[i] = src[i];
    return n;
}

// program_eval_interval over n boxes (lo, hi: n x 3)
int rmi_eval(const RmSceneOp* ops, int32_t nops, const double* lo, const double* hi, size_t n, double* out_lo, double* out_hi,
             char* why, int why_len)
{
    if (encode(ops, nops, why, why_len)) return -1;
    const ProgSrc src{ &g_img };
    for (size_t i = 0; i < n; ++i) {
        const Ival r = program_eval_interval(
            src, ivec3(iv(lo[3 * i], hi[3 * i]), iv(lo[3 * i + 1], hi[3 * i + 1]), iv(lo[3 * i + 2], hi[3 * i + 2])));
        out_lo[i] = r.lo;
        out_hi[i] = r.hi;
    }
    return 0;
}

// interval_first_hit (+ normals, optional) over n rays; scene_bound is unused by the march
int rmi_march(const RmSceneOp* ops, int32_t nops, const RmIntervalConfig* cfg, const double* o, const double* d, size_t n,
              double* t, int32_t* steps, double* normals, char* why, int why_len)
{
    if (encode(ops, nops, why, why_len)) return -1;
    IntervalParams P;
    if (params(cfg, -1.0, &P, why, why_len)) return -2;
    const ProgSrc src{ &g_img };
    for (size_t i = 0; i < n; ++i) {
        const vec3 oi = v3(o[3 * i], o[3 * i + 1], o[3 * i + 2]), di = v3(d[3 * i], d[3 * i + 1], d[3 * i + 2]);
        int32_t s = 0;
        t[i] = interval_first_hit(src, oi, di, P, &s);
        if (steps) steps[i] = s;
        if (normals) {
            const vec3 nv = t[i] < __builtin_inf() ? interval_normal(src, oi, di, t[i], P.normal_eps) : v3(0.0, 0.0, 0.0);
            normals[3 * i] = nv.x; normals[3 * i + 1] = nv.y; normals[3 * i + 2] = nv.z;
        }
    }
    return 0;
}

// interval_capture of rows [row0, row0 + rows) with the library's camera; scene_bound as interval_scene_bound gives it
int rmi_render(const RmSceneOp* ops, int32_t nops, const RmIntervalConfig* cfg, double scene_bound, const double* cam14, int width,
               int height, int row0, int rows, double* depth, uint8_t* hit, double* normal, int32_t* steps, char* why, int why_len)
{
    if (encode(ops, nops, why, why_len)) return -1;
    IntervalParams P;
    if (params(cfg, scene_bound, &P, why, why_len)) return -2;
    CameraParams cam;
    for (int i = 0; i < 14; ++i) cam.v[i] = cam14[i];
    const ProgSrc src{ &g_img };
    for (int y = 0; y < rows; ++y)
        for (int x = 0; x < width; ++x) {
            const size_t i = (size_t)y * width + x;
            vec3 nv;
            interval_pixel(src, cam, width, height, x, row0 + y, P, true, &depth[i], &hit[i], &nv, &steps[i]);
            normal[3 * i] = nv.x; normal[3 * i + 1] = nv.y; normal[3 * i + 2] = nv.z;
        }
    return 0;
}

// the library's prune radius of catalogue scene `id` (SCENE_BOUND; -1: none)
double rmi_scene_bound(int id) { return interval_scene_bound(id); }

size_t rmi_sizeof_config(void) { return sizeof(RmIntervalConfig); }
size_t rmi_offsetof_config(int field)
{
    switch (field) {
        case 0: return offsetof(RmIntervalConfig, t_max);
        case 1: return offsetof(RmIntervalConfig, tol);
        case 2: return offsetof(RmIntervalConfig, h0);
        case 3: return offsetof(RmIntervalConfig, growth);
        case 4: return offsetof(RmIntervalConfig, h_max);
        case 5: return offsetof(RmIntervalConfig, normal_eps);
        case 6: return offsetof(RmIntervalConfig, bound_radius);
        case 7: return offsetof(RmIntervalConfig, max_steps);
        case 8: return offsetof(RmIntervalConfig, reserved);
    }
    return (size_t)-1;
}

}
