// rm_affine.hip -- the affine range and its march on the device (rm_affine.h; rm_affine_* in include/rm_hip.h).
//
// As rm_interval.hip: one ray (or one segment) per lane, 256-thread workgroups, the scene program in LDS and every
// instruction word moved to a scalar register, so the opcode dispatch is a chain of scalar branches.  `mode` is a kernel
// argument, so the second walk of RM_RANGE_MEET (the interval program over the same segment) sits behind a wave-uniform
// branch.  The march loop is per lane; a wave runs as long as its longest ray.
#include "rm_kernels.h"
#include "rm_affine.h"
#include "rm_capi_internal.h"

namespace rm {

constexpr int kAffineBlock = 256;

__global__ __launch_bounds__(kAffineBlock) void affine_range_kernel(const void* prog, int mode, const double* __restrict__ segs,
                                                                   size_t n, double* __restrict__ out_range,
                                                                   double* __restrict__ out_form)
{
    SceneProgram::load(prog);
    rm_load_tables<SceneExtProgram>();      // the pow tables and, for RM_SOP_GYROID, sin / cos
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* s = segs + 8 * i;
    Aff f;
    const Ival r = affine_range(ProgSrc{}, mode, v3(s[0], s[1], s[2]), v3(s[3], s[4], s[5]), s[6], s[7], &f);
    out_range[2 * i] = r.lo;
    out_range[2 * i + 1] = r.hi;
    if (out_form) {
        out_form[3 * i] = f.x0;
        out_form[3 * i + 1] = f.x1;
        out_form[3 * i + 2] = f.e;
    }
}

__global__ __launch_bounds__(kAffineBlock) void affine_march_kernel(const void* prog, int mode, IntervalParams P,
                                                                   const double* __restrict__ origins,
                                                                   const double* __restrict__ dirs, size_t n,
                                                                   double* __restrict__ t_out, int32_t* __restrict__ steps)
{
    SceneProgram::load(prog);
    rm_load_tables<SceneExtProgram>();      // the pow tables and, for RM_SOP_GYROID, sin / cos
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const vec3 o = v3(origins[3 * i], origins[3 * i + 1], origins[3 * i + 2]);
    const vec3 d = v3(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]);      // as given: march_count does not normalise
    int32_t s = 0;
    t_out[i] = affine_first_hit(ProgSrc{}, mode, o, d, P, &s);
    if (steps) steps[i] = s;
}

__global__ __launch_bounds__(kAffineBlock) void affine_render_kernel(const void* prog, int mode, IntervalParams P, CameraParams cam,
                                                                    int width, int height, int row0, size_t n,
                                                                    double* __restrict__ depth, uint8_t* __restrict__ hit,
                                                                    int32_t* __restrict__ steps)
{
    SceneProgram::load(prog);
    rm_load_tables<SceneExtProgram>();      // the pow tables and, for RM_SOP_GYROID, sin / cos
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int py = row0 + (int)(i / (size_t)width), px = (int)(i % (size_t)width);
    double dp;
    uint8_t h;
    int32_t s;
    affine_pixel(ProgSrc{}, mode, cam, width, height, px, py, P, &dp, &h, &s);
    depth[i] = dp;
    hit[i] = h;
    if (steps) steps[i] = s;
}

static unsigned grid_of(size_t n) { return (unsigned)((n + kAffineBlock - 1) / kAffineBlock); }

}  // namespace rm

// ---- rm_affine_* of the C ABI: scenes and programs as the interval oracle -------------------------------------------------
// (every launch below: the arguments are validated, `prog` is the device copy of the scene's ProgramImage, n > 0)
using namespace rm::capi;

namespace {

int affine_mode(int mode)
{
    if (!rm::affine_mode_ok(mode))
        return fail(RM_E_BAD_ARG, "mode %d is neither RM_RANGE_AFFINE (%d) nor RM_RANGE_MEET (%d)", mode, RM_RANGE_AFFINE, RM_RANGE_MEET);
    return RM_OK;
}

// the mode, then the march's constants
int affine_params(int id, int mode, const RmIntervalConfig* cfg, rm::IntervalParams* P)
{
    int rc = affine_mode(mode);
    return rc ? rc : interval_params(id, cfg, P);
}

}  // namespace

extern "C" {

int rm_affine_supported(int scene_id) { return rm_interval_supported(scene_id); }

int rm_affine_range_eval(int scene_id, int mode, const double* segs, size_t n, double* out_range, double* out_form)
{
    SoundCall c;
    int rc = c.open(scene_id, [&] {
        int r = affine_mode(mode);
        if (!r && mode == RM_RANGE_MEET && out_form) r = fail(RM_E_BAD_ARG, "out_form must be NULL in RM_RANGE_MEET: the meet is no form's range");
        return r;
    }, nullptr, nullptr, n, segs && out_range, "NULL buffer");
    if (rc || !c.prog) return rc;
    Staged st(*c.e);
    const double* d_segs = st.in(stage_in[0], segs, n * 64);
    double* d_range = st.out(stage_out[0], out_range, n * 16);
    double* d_form = st.out(stage_out[1], out_form, n * 24);
    if ((rc = st.begin())) return rc;
    hipLaunchKernelGGL(rm::affine_range_kernel, dim3(rm::grid_of(n)), dim3(rm::kAffineBlock), 0, lib_stream(), c.prog, mode, d_segs, n,
                       d_range, d_form);
    HIP_TRY(hipGetLastError());
    return st.finish();
}

int rm_affine_march_rays(int scene_id, int mode, const RmIntervalConfig* cfg, const double* origins, const double* dirs, size_t n,
                         double* t, int32_t* steps)
{
    rm::IntervalParams P;
    SoundCall c;
    int rc = c.open(scene_id, [&] { return affine_params(scene_id, mode, cfg, &P); }, nullptr, nullptr, n, origins && dirs && t, "NULL buffer");
    if (rc || !c.prog) return rc;
    Staged st(*c.e);
    const double* d_origins = st.in(stage_in[0], origins, n * 24);
    const double* d_dirs = st.in(stage_in[1], dirs, n * 24);
    double* d_t = st.out(stage_out[0], t, n * 8);
    int32_t* d_steps = st.out(stage_out[1], steps, n * 4);
    if ((rc = st.begin())) return rc;
    hipLaunchKernelGGL(rm::affine_march_kernel, dim3(rm::grid_of(n)), dim3(rm::kAffineBlock), 0, lib_stream(), c.prog, mode, P, d_origins,
                       d_dirs, n, d_t, d_steps);
    HIP_TRY(hipGetLastError());
    return st.finish();
}

int rm_affine_render(const RmFrameDesc* d, int mode, const RmIntervalConfig* cfg, double* depth, uint8_t* hit, int32_t* steps,
                     RmTiming* timing)
{
    if (!d) return fail(RM_E_BAD_ARG, "desc is NULL");
    rm::IntervalParams P;
    const size_t n = (size_t)d->width * (size_t)d->rows;
    SoundCall c;
    int rc = c.open(d->scene_id, [&] { return affine_params(d->scene_id, mode, cfg, &P); }, d, timing, n, depth && hit,
                    "depth and hit are required");
    if (rc || !c.prog) return rc;
    Staged st(*c.e);
    double* d_depth = st.out(stage_out[0], depth, n * 8);
    uint8_t* d_hit = st.out(stage_out[1], hit, n);
    int32_t* d_steps = st.out(stage_out[2], steps, n * 4);
    if ((rc = st.begin())) return rc;
    const rm::CameraParams cam = camera_of(d->cam);
    rc = once_or_timed(*c.e, timing, lib_stream(), [&] {
        hipLaunchKernelGGL(rm::affine_render_kernel, dim3(rm::grid_of(n)), dim3(rm::kAffineBlock), 0, lib_stream(), c.prog, mode, P, cam,
                           d->width, d->height, d->row0, n, d_depth, d_hit, d_steps);
        HIP_TRY(hipGetLastError());
        return (int)RM_OK;
    });
    return rc ? rc : st.finish();
}

}  // extern "C"
