// Host-only check build of the certified first hit (csrc/rm_certify.h) -- compiled by g++ for tests ONLY, so the exact
// source the gfx950 kernels are built from can be compared with the exact caster, the interval oracle, the pointwise
// interpreter and the device in a container without a GPU.  Never loaded by the product.
#include <stddef.h>
#include <stdint.h>
#include "../../raymarch_algo_compare_amd/csrc/rm_certify.h"

using namespace rm;

namespace {
thread_local ProgramImage g_img;

int encode(const RmSceneOp* ops, int32_t nops, char* why, int why_len)
{
    return program_encode(ops, nops, &g_img, why, (size_t)why_len) ? 0 : -1;
}
}  // namespace

extern "C" {

// certify_first_hit over n rays
int rmc_march(const RmSceneOp* ops, int32_t nops, const RmCertifyConfig* cfg, const double* o, const double* d, size_t n,
              double* t_lo, double* t_hi, uint8_t* status, int32_t* steps, char* why, int why_len)
{
    if (encode(ops, nops, why, why_len)) return -1;
    CertifyParams P;
    if (!certify_resolve(cfg, -1.0, &P, why, (size_t)why_len)) return -2;
    const ProgSrc src{ &g_img };
    for (size_t i = 0; i < n; ++i)
        certify_first_hit(src, v3(o[3 * i], o[3 * i + 1], o[3 * i + 2]), v3(d[3 * i], d[3 * i + 1], d[3 * i + 2]), P, &t_lo[i],
                          &t_hi[i], &status[i], &steps[i]);
    return 0;
}

// certify_pixel over rows [row0, row0 + rows) with the library's camera; scene_bound as interval_scene_bound gives it
int rmc_render(const RmSceneOp* ops, int32_t nops, const RmCertifyConfig* cfg, double scene_bound, const double* cam14, int width,
               int height, int row0, int rows, double* t_lo, double* t_hi, uint8_t* status, int32_t* steps, char* why, int why_len)
{
    if (encode(ops, nops, why, why_len)) return -1;
    CertifyParams P;
    if (!certify_resolve(cfg, scene_bound, &P, why, (size_t)why_len)) return -2;
    CameraParams cam;
    for (int i = 0; i < 14; ++i) cam.v[i] = cam14[i];
    const ProgSrc src{ &g_img };
    for (int y = 0; y < rows; ++y)
        for (int x = 0; x < width; ++x) {
            const size_t i = (size_t)y * width + x;
            certify_pixel(src, cam, width, height, x, row0 + y, P, &t_lo[i], &t_hi[i], &status[i], &steps[i]);
        }
    return 0;
}

// certify_resolve alone: 0, or -2 with the reason; the resolved constants in out[11] (max_steps last)
int rmc_resolve(const RmCertifyConfig* cfg, double scene_bound, double* out, char* why, int why_len)
{
    CertifyParams P;
    if (!certify_resolve(cfg, scene_bound, &P, why, (size_t)why_len)) return -2;
    const double v[11] = { P.t_max, P.tol, P.h0, P.growth, P.h_max, P.bound, P.width, P.width_rel, P.l_global, P.k_min,
                           (double)P.max_steps };
    for (int i = 0; i < 11; ++i) out[i] = v[i];
    return 0;
}

double rmc_scene_bound(int id) { return interval_scene_bound(id); }

size_t rmc_sizeof_config(void) { return sizeof(RmCertifyConfig); }
size_t rmc_offsetof_config(int field)
{
    switch (field) {
        case 0: return offsetof(RmCertifyConfig, t_max);
        case 1: return offsetof(RmCertifyConfig, tol);
        case 2: return offsetof(RmCertifyConfig, h0);
        case 3: return offsetof(RmCertifyConfig, growth);
        case 4: return offsetof(RmCertifyConfig, h_max);
        case 5: return offsetof(RmCertifyConfig, bound_radius);
        case 6: return offsetof(RmCertifyConfig, width);
        case 7: return offsetof(RmCertifyConfig, l_global);
        case 8: return offsetof(RmCertifyConfig, k_min);
        case 9: return offsetof(RmCertifyConfig, max_steps);
        case 10: return offsetof(RmCertifyConfig, reserved);
    }
    return (size_t)-1;
}

}
