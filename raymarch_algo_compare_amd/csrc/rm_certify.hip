// rm_certify.hip -- the certified first hit on the device (rm_certify.h; rm_certify_* in include/rm_hip.h).
//
// As rm_segment.hip: one ray per lane, 256-thread workgroups, the scene program in LDS and every instruction word moved
// to a scalar register, so the opcode dispatch is a chain of scalar branches.  Each trip of the march is two dependent
// passes over the instruction words: the dual-interval program over the probe, then the interval program at the probe's
// end (a degenerate box).  The loop is per lane; a wave runs as long as its longest ray, at most `max_steps` trips
// (RM_INTERVAL_MAX_STEPS).
#include "rm_kernels.h"
#include "rm_certify.h"
#include "rm_capi_internal.h"

namespace rm {

constexpr int kCertifyBlock = 256;

__global__ __launch_bounds__(kCertifyBlock) void certify_march_kernel(const void* prog, CertifyParams P,
                                                                     const double* __restrict__ origins,
                                                                     const double* __restrict__ dirs, size_t n,
                                                                     double* __restrict__ t_lo, double* __restrict__ t_hi,
                                                                     uint8_t* __restrict__ status, int32_t* __restrict__ steps)
{
    SceneProgram::load(prog);
    rm_load_tables<SceneExtProgram>();      // the pow tables and, for RM_SOP_GYROID, sin / cos
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const vec3 o = v3(origins[3 * i], origins[3 * i + 1], origins[3 * i + 2]);
    const vec3 d = v3(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]);      // as given: the march does not normalise
    double lo, hi;
    uint8_t st;
    int32_t s;
    certify_first_hit(ProgSrc{}, o, d, P, &lo, &hi, &st, &s);
    t_lo[i] = lo;
    t_hi[i] = hi;
    status[i] = st;
    if (steps) steps[i] = s;
}

__global__ __launch_bounds__(kCertifyBlock) void certify_render_kernel(const void* prog, CertifyParams P, CameraParams cam,
                                                                      int width, int height, int row0, size_t n,
                                                                      double* __restrict__ t_lo, double* __restrict__ t_hi,
                                                                      uint8_t* __restrict__ status, int32_t* __restrict__ steps)
{
    SceneProgram::load(prog);
    rm_load_tables<SceneExtProgram>();      // the pow tables and, for RM_SOP_GYROID, sin / cos
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;      // a frame has fewer than 2^31 pixels (check_slice)
    if (i >= n) return;
    const int py = row0 + (int)(i / (size_t)width), px = (int)(i % (size_t)width);
    double lo, hi;
    uint8_t st;
    int32_t s;
    certify_pixel(ProgSrc{}, cam, width, height, px, py, P, &lo, &hi, &st, &s);
    t_lo[i] = lo;
    t_hi[i] = hi;
    status[i] = st;
    if (steps) steps[i] = s;
}

static unsigned grid_of(size_t n) { return (unsigned)((n + kCertifyBlock - 1) / kCertifyBlock); }

}  // namespace rm

// ---- rm_certify_* of the C ABI: scenes and programs as the interval oracle ------------------------------------------------
// (every launch below: the arguments are validated, `prog` is the device copy of the scene's ProgramImage, n > 0)
using namespace rm::capi;

namespace {

int certify_params(int id, const RmCertifyConfig* cfg, rm::CertifyParams* P)
{
    char why[160];
    if (!rm::certify_resolve(cfg, rm::interval_scene_bound(id), P, why, sizeof why))
        return fail(RM_E_BAD_ARG, "RmCertifyConfig: %s", why);
    return RM_OK;
}

}  // namespace

extern "C" {

int rm_certify_supported(int scene_id) { return rm_segment_supported(scene_id); }

int rm_certify_march_rays(int scene_id, const RmCertifyConfig* cfg, const double* origins, const double* dirs, size_t n,
                          double* t_lo, double* t_hi, uint8_t* status, int32_t* steps)
{
    rm::CertifyParams P;
    SoundCall c;
    int rc = c.open(scene_id, [&] { return certify_params(scene_id, cfg, &P); }, nullptr, nullptr, n,
                    origins && dirs && t_lo && t_hi && status, "NULL buffer");
    if (rc || !c.prog) return rc;
    Staged st(*c.e);
    const double* d_origins = st.in(stage_in[0], origins, n * 24);
    const double* d_dirs = st.in(stage_in[1], dirs, n * 24);
    double* d_lo = st.out(stage_out[0], t_lo, n * 8);
    double* d_hi = st.out(stage_out[1], t_hi, n * 8);
    uint8_t* d_status = st.out(stage_out[2], status, n);
    int32_t* d_steps = st.out(stage_out[3], steps, n * 4);
    if ((rc = st.begin())) return rc;
    hipLaunchKernelGGL(rm::certify_march_kernel, dim3(rm::grid_of(n)), dim3(rm::kCertifyBlock), 0, lib_stream(), c.prog, P, d_origins,
                       d_dirs, n, d_lo, d_hi, d_status, d_steps);
    HIP_TRY(hipGetLastError());
    return st.finish();
}

int rm_certify_render(const RmFrameDesc* d, const RmCertifyConfig* cfg, double* t_lo, double* t_hi, uint8_t* status, int32_t* steps,
                      RmTiming* timing)
{
    if (!d) return fail(RM_E_BAD_ARG, "desc is NULL");
    rm::CertifyParams P;
    const size_t n = (size_t)d->width * (size_t)d->rows;
    SoundCall c;
    int rc = c.open(d->scene_id, [&] { return certify_params(d->scene_id, cfg, &P); }, d, timing, n, t_lo && t_hi && status,
                    "t_lo, t_hi and status are required");
    if (rc || !c.prog) return rc;
    Staged st(*c.e);
    double* d_lo = st.out(stage_out[0], t_lo, n * 8);
    double* d_hi = st.out(stage_out[1], t_hi, n * 8);
    uint8_t* d_status = st.out(stage_out[2], status, n);
    int32_t* d_steps = st.out(stage_out[3], steps, n * 4);
    if ((rc = st.begin())) return rc;
    const rm::CameraParams cam = camera_of(d->cam);
    rc = once_or_timed(*c.e, timing, lib_stream(), [&] {
        hipLaunchKernelGGL(rm::certify_render_kernel, dim3(rm::grid_of(n)), dim3(rm::kCertifyBlock), 0, lib_stream(), c.prog, P, cam,
                           d->width, d->height, d->row0, n, d_lo, d_hi, d_status, d_steps);
        HIP_TRY(hipGetLastError());
        return (int)RM_OK;
    });
    return rc ? rc : st.finish();
}

}  // extern "C"
