// Host-only check build of the exact first hit (csrc/rm_exact.h) -- compiled by g++ for tests ONLY, so the exact source
// the gfx950 kernels are built from can be compared with analytic.py, with the reference's fixtures, with the host
// interval oracle and with the device in a container without a GPU.  Never loaded by the product.
#include <stddef.h>
#include <stdint.h>
#include "../../raymarch_algo_compare_amd/csrc/rm_exact.h"
#include "../../raymarch_algo_compare_amd/csrc/rm_interval_catalogue.h"

using namespace rm;

namespace {
thread_local ProgramImage g_img;

// 0, or -1 (malformed program), -2 (no exact form), -3 (bad configuration) with the reason in why
int open(const RmSceneOp* ops, int32_t nops, const RmExactConfig* cfg, ExactParams* P, char* why, int why_len)
{
    if (!program_encode(ops, nops, &g_img, why, (size_t)why_len)) return -1;
    if (!exact_supported(g_img, why, (size_t)why_len)) return -2;
    if (P && !exact_resolve(cfg, P, why, (size_t)why_len)) return -3;
    return 0;
}
}  // namespace

extern "C" {

// the catalogue table: the program of scene `id` copied to ops (room for cap ops); its length, 0 without one
int rme_catalogue(int id, RmSceneOp* ops, int cap)
{
    int32_t n = 0;
    const RmSceneOp* src = interval_catalogue_ops(id, &n);
    if (!src) return 0;
    for (int i = 0; i < n && i < cap; ++i) ops[i] = src[i];
    return n;
}

// exact_supported of the encoded program: 1, 0 with the reason, -1 for a malformed program
int rme_supported(const RmSceneOp* ops, int32_t nops, char* why, int why_len)
{
    const int rc = open(ops, nops, nullptr, nullptr, why, why_len);
    return rc == 0 ? 1 : (rc == -2 ? 0 : -1);
}

// exact_first_hit over n rays; normals and leaf optional
int rme_march(const RmSceneOp* ops, int32_t nops, const RmExactConfig* cfg, const double* o, const double* d, size_t n, double* t,
              double* normals, int32_t* leaf, char* why, int why_len)
{
    ExactParams P;
    const int rc = open(ops, nops, cfg, &P, why, why_len);
    if (rc) return rc;
    const ProgSrc src{ &g_img };
    for (size_t i = 0; i < n; ++i) {
        const ExactHit h = exact_first_hit(src, v3(o[3 * i], o[3 * i + 1], o[3 * i + 2]), v3(d[3 * i], d[3 * i + 1], d[3 * i + 2]),
                                           P.t_min, P.t_max);
        t[i] = h.t;
        if (normals) { normals[3 * i] = h.normal.x; normals[3 * i + 1] = h.normal.y; normals[3 * i + 2] = h.normal.z; }
        if (leaf) leaf[i] = h.leaf;
    }
    return 0;
}

// exact_pixel over rows [row0, row0 + rows) with the library's camera
int rme_render(const RmSceneOp* ops, int32_t nops, const RmExactConfig* cfg, const double* cam14, int width, int height, int row0,
               int rows, double* depth, uint8_t* hit, double* normal, int32_t* leaf, char* why, int why_len)
{
    ExactParams P;
    const int rc = open(ops, nops, cfg, &P, why, why_len);
    if (rc) return rc;
    CameraParams cam;
    for (int i = 0; i < 14; ++i) cam.v[i] = cam14[i];
    const ProgSrc src{ &g_img };
    for (int y = 0; y < rows; ++y)
        for (int x = 0; x < width; ++x) {
            const size_t i = (size_t)y * width + x;
            vec3 nv;
            exact_pixel(src, cam, width, height, x, row0 + y, P, &depth[i], &hit[i], &nv, &leaf[i]);
            normal[3 * i] = nv.x; normal[3 * i + 1] = nv.y; normal[3 * i + 2] = nv.z;
        }
    return 0;
}

size_t rme_sizeof_config(void) { return sizeof(RmExactConfig); }
size_t rme_offsetof_config(int field)
{
    switch (field) {
        case 0: return offsetof(RmExactConfig, t_min);
        case 1: return offsetof(RmExactConfig, t_max);
        case 2: return offsetof(RmExactConfig, reserved);
    }
    return (size_t)-1;
}

}
