// Host-only check build of the two placement ops of scene programs (RM_SOP_ROTATE, RM_SOP_MIRROR) in all five evaluations:
// the point walk of csrc/rm_scene_program.h, the interval extension of csrc/rm_interval.h, the dual interval of
// csrc/rm_segment.h, the affine range of csrc/rm_affine.h and the exact first hit of csrc/rm_exact.h -- compiled by g++ for tests
// ONLY, so the exact source the gfx950 kernels are built from can be checked against NumPy, against itself and against the
// device in a container without a GPU.  Never loaded by the product.
#include <stddef.h>
#include <stdint.h>
#include "../../raymarch_algo_compare_amd/csrc/rm_affine.h"
#include "../../raymarch_algo_compare_amd/csrc/rm_exact.h"
#include "../../raymarch_algo_compare_amd/csrc/rm_segment.h"

using namespace rm;

namespace {
thread_local ProgramImage g_img;

int encode(const RmSceneOp* ops, int32_t nops, char* why, int why_len)
{
    return program_encode(ops, nops, &g_img, why, (size_t)why_len) ? 0 : -1;
}

// 0, or -1 (malformed program), -2 (no exact form), -3 (bad configuration) with the reason in why
int open_exact(const RmSceneOp* ops, int32_t nops, const RmExactConfig* cfg, ExactParams* P, char* why, int why_len)
{
    if (encode(ops, nops, why, why_len)) return -1;
    if (!exact_supported(g_img, why, (size_t)why_len)) return -2;
    if (P && !exact_resolve(cfg, P, why, (size_t)why_len)) return -3;
    return 0;
}
}  // namespace

extern "C" {

// program_encode alone: 0, or -1 with the reason in why; the encoded words (room for cap) and their number for a good program
int rmp_encode(const RmSceneOp* ops, int32_t nops, uint32_t* words, int cap, int32_t* nwords, char* why, int why_len)
{
    if (encode(ops, nops, why, why_len)) return -1;
    if (nwords) *nwords = g_img.nops;
    for (int i = 0; words && i < g_img.nops && i < cap; ++i) words[i] = g_img.code[i];
    return 0;
}

// program_eval over n points (xyz: n x 3)
int rmp_point(const RmSceneOp* ops, int32_t nops, const double* xyz, size_t n, double* out, char* why, int why_len)
{
    if (encode(ops, nops, why, why_len)) return -1;
    const ProgSrc src{ &g_img };
    for (size_t i = 0; i < n; ++i) out[i] = program_eval(src, v3(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]));
    return 0;
}

// program_eval_interval over n boxes (lo, hi: n x 3; out: n x 2)
int rmp_interval(const RmSceneOp* ops, int32_t nops, const double* lo, const double* hi, size_t n, double* out, char* why,
                 int why_len)
{
    if (encode(ops, nops, why, why_len)) return -1;
    const ProgSrc src{ &g_img };
    for (size_t i = 0; i < n; ++i) {
        const Ival r = program_eval_interval(
            src, ivec3(iv(lo[3 * i], hi[3 * i]), iv(lo[3 * i + 1], hi[3 * i + 1]), iv(lo[3 * i + 2], hi[3 * i + 2])));
        out[2 * i] = r.lo; out[2 * i + 1] = r.hi;
    }
    return 0;
}

// over n segments (segs: n x 8 = origin, direction, t0, t1): program_eval_dual (dual: n x 4 = val.lo, val.hi, der.lo, der.hi)
// and program_eval_interval over the box of the same segment (box: n x 2)
int rmp_dual(const RmSceneOp* ops, int32_t nops, const double* segs, size_t n, double* dual, double* box, char* why, int why_len)
{
    if (encode(ops, nops, why, why_len)) return -1;
    const ProgSrc src{ &g_img };
    for (size_t i = 0; i < n; ++i) {
        const double* s = segs + 8 * i;
        const vec3 o = v3(s[0], s[1], s[2]), d = v3(s[3], s[4], s[5]);
        const IVec3 b = seed_segment(o, d, s[6], s[7]);
        const DIval r = program_eval_dual(src, b, d);
        const Ival v = program_eval_interval(src, b);
        dual[4 * i] = r.val.lo; dual[4 * i + 1] = r.val.hi; dual[4 * i + 2] = r.der.lo; dual[4 * i + 3] = r.der.hi;
        box[2 * i] = v.lo; box[2 * i + 1] = v.hi;
    }
    return 0;
}

// affine_range in `mode` over n segments (out: n x 2; form, optional: n x 3 = x0, x1, e of the affine form)
int rmp_affine(const RmSceneOp* ops, int32_t nops, int mode, const double* segs, size_t n, double* out, double* form, char* why,
               int why_len)
{
    if (encode(ops, nops, why, why_len)) return -1;
    if (!affine_mode_ok(mode)) return -3;
    const ProgSrc src{ &g_img };
    for (size_t i = 0; i < n; ++i) {
        const double* s = segs + 8 * i;
        Aff f;
        const Ival r = affine_range(src, mode, v3(s[0], s[1], s[2]), v3(s[3], s[4], s[5]), s[6], s[7], &f);
        out[2 * i] = r.lo; out[2 * i + 1] = r.hi;
        if (form) { form[3 * i] = f.x0; form[3 * i + 1] = f.x1; form[3 * i + 2] = f.e; }
    }
    return 0;
}

// exact_supported of the encoded program: 1, 0 with the reason, -1 for a malformed program
int rmp_exact_supported(const RmSceneOp* ops, int32_t nops, char* why, int why_len)
{
    const int rc = open_exact(ops, nops, nullptr, nullptr, why, why_len);
    return rc == 0 ? 1 : (rc == -2 ? 0 : -1);
}

// exact_first_hit over n rays (directions as given)
int rmp_exact_march(const RmSceneOp* ops, int32_t nops, const RmExactConfig* cfg, const double* o, const double* d, size_t n, double* t,
                    double* normals, int32_t* leaf, char* why, int why_len)
{
    ExactParams P;
    const int rc = open_exact(ops, nops, cfg, &P, why, why_len);
    if (rc) return rc;
    const ProgSrc src{ &g_img };
    for (size_t i = 0; i < n; ++i) {
        const ExactHit h = exact_first_hit(src, v3(o[3 * i], o[3 * i + 1], o[3 * i + 2]), v3(d[3 * i], d[3 * i + 1], d[3 * i + 2]),
                                           P.t_min, P.t_max);
        t[i] = h.t;
        normals[3 * i] = h.normal.x; normals[3 * i + 1] = h.normal.y; normals[3 * i + 2] = h.normal.z;
        leaf[i] = h.leaf;
    }
    return 0;
}

// exact_pixel over a whole frame with the library's camera
int rmp_exact_render(const RmSceneOp* ops, int32_t nops, const RmExactConfig* cfg, const double* cam14, int width, int height,
                     double* depth, uint8_t* hit, double* normal, int32_t* leaf, char* why, int why_len)
{
    ExactParams P;
    const int rc = open_exact(ops, nops, cfg, &P, why, why_len);
    if (rc) return rc;
    CameraParams cam;
    for (int i = 0; i < 14; ++i) cam.v[i] = cam14[i];
    const ProgSrc src{ &g_img };
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) {
            const size_t i = (size_t)y * width + x;
            vec3 nv;
            exact_pixel(src, cam, width, height, x, y, P, &depth[i], &hit[i], &nv, &leaf[i]);
            normal[3 * i] = nv.x; normal[3 * i + 1] = nv.y; normal[3 * i + 2] = nv.z;
        }
    return 0;
}

// interval_capture (no normals) of a whole frame with the library's camera and no prune
int rmp_interval_render(const RmSceneOp* ops, int32_t nops, const RmIntervalConfig* cfg, const double* cam14, int width, int height,
                        double* depth, uint8_t* hit, int32_t* steps, char* why, int why_len)
{
    if (encode(ops, nops, why, why_len)) return -1;
    IntervalParams P;
    if (!interval_resolve(cfg, -1.0, &P, why, (size_t)why_len)) return -2;
    CameraParams cam;
    for (int i = 0; i < 14; ++i) cam.v[i] = cam14[i];
    const ProgSrc src{ &g_img };
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) {
            const size_t i = (size_t)y * width + x;
            vec3 nv;
            interval_pixel(src, cam, width, height, x, y, P, false, &depth[i], &hit[i], &nv, &steps[i]);
        }
    return 0;
}

// _capture of gpu/affine.py (affine_pixel) of a whole frame in `mode`, no prune
int rmp_affine_render(const RmSceneOp* ops, int32_t nops, int mode, const RmIntervalConfig* cfg, const double* cam14, int width,
                      int height, double* depth, uint8_t* hit, int32_t* steps, char* why, int why_len)
{
    if (encode(ops, nops, why, why_len)) return -1;
    if (!affine_mode_ok(mode)) return -3;
    IntervalParams P;
    if (!interval_resolve(cfg, -1.0, &P, why, (size_t)why_len)) return -2;
    CameraParams cam;
    for (int i = 0; i < 14; ++i) cam.v[i] = cam14[i];
    const ProgSrc src{ &g_img };
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) {
            const size_t i = (size_t)y * width + x;
            affine_pixel(src, mode, cam, width, height, x, y, P, &depth[i], &hit[i], &steps[i]);
        }
    return 0;
}

}
