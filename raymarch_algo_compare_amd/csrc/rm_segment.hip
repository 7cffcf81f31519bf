// rm_segment.hip -- the sound segment tracer on the device (rm_segment.h; rm_segment_* in include/rm_hip.h).
//
// As rm_interval.hip: one ray (or one segment) per lane, 256-thread workgroups, the scene program in LDS and every
// instruction word moved to a scalar register, so the opcode dispatch is a chain of scalar branches.  Each trip of the
// trace is two dependent passes over the instruction words: the interval program at the cursor (a degenerate box), then
// the dual-interval program over the probe segment.  The loop is per lane; a wave runs as long as its longest ray, at
// most `budget` trips (RM_SEGMENT_MAX_STEPS).
#include "rm_kernels.h"
#include "rm_segment.h"
#include "rm_capi_internal.h"

namespace rm {

constexpr int kSegmentBlock = 256;

__global__ __launch_bounds__(kSegmentBlock) void segment_sdf_kernel(const void* prog, const double* __restrict__ segs, size_t n,
                                                                   double* __restrict__ out)
{
    SceneProgram::load(prog);
    rm_load_tables<SceneExtProgram>();      // the pow tables and, for RM_SOP_GYROID, sin / cos
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* s = segs + 8 * i;
    const vec3 o = v3(s[0], s[1], s[2]), d = v3(s[3], s[4], s[5]);
    const DIval r = program_eval_dual(ProgSrc{}, seed_segment(o, d, s[6], s[7]), d);
    out[4 * i] = r.val.lo;
    out[4 * i + 1] = r.val.hi;
    out[4 * i + 2] = r.der.lo;
    out[4 * i + 3] = r.der.hi;
}

__global__ __launch_bounds__(kSegmentBlock) void segment_march_kernel(const void* prog, SegmentParams P,
                                                                     const double* __restrict__ origins,
                                                                     const double* __restrict__ dirs, size_t n,
                                                                     double* __restrict__ t_out, int32_t* __restrict__ iters,
                                                                     double* __restrict__ cursor)
{
    SceneProgram::load(prog);
    rm_load_tables<SceneExtProgram>();      // the pow tables and, for RM_SOP_GYROID, sin / cos
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const vec3 o = v3(origins[3 * i], origins[3 * i + 1], origins[3 * i + 2]);
    const vec3 d = v3(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]);      // as given: segment_trace does not normalise
    int32_t s = 0;
    double c = 0.0;
    t_out[i] = segment_trace(ProgSrc{}, o, d, P, &s, &c);
    if (iters) iters[i] = s;
    if (cursor) cursor[i] = c;
}

__global__ __launch_bounds__(kSegmentBlock) void segment_render_kernel(const void* prog, SegmentParams P, CameraParams cam,
                                                                      int width, int height, int row0, size_t n,
                                                                      double* __restrict__ depth, uint8_t* __restrict__ hit,
                                                                      int32_t* __restrict__ iters, double* __restrict__ cursor)
{
    SceneProgram::load(prog);
    rm_load_tables<SceneExtProgram>();      // the pow tables and, for RM_SOP_GYROID, sin / cos
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int py = row0 + (int)(i / (size_t)width), px = (int)(i % (size_t)width);
    double dp, c;
    uint8_t h;
    int32_t s;
    segment_pixel(ProgSrc{}, cam, width, height, px, py, P, &dp, &h, &s, &c);
    depth[i] = dp;
    hit[i] = h;
    if (iters) iters[i] = s;
    if (cursor) cursor[i] = c;
}

static unsigned grid_of(size_t n) { return (unsigned)((n + kSegmentBlock - 1) / kSegmentBlock); }

}  // namespace rm

// ---- rm_segment_* of the C ABI: scenes and programs as the interval oracle ------------------------------------------------
// (every launch below: the arguments are validated, `prog` is the device copy of the scene's ProgramImage, n > 0)
using namespace rm::capi;

namespace {

int segment_params(int id, const RmSegmentConfig* cfg, rm::SegmentParams* P)
{
    char why[160];
    if (!rm::segment_resolve(cfg, rm::interval_scene_bound(id), P, why, sizeof why))
        return fail(RM_E_BAD_ARG, "RmSegmentConfig: %s", why);
    return RM_OK;
}

}  // namespace

extern "C" {

int rm_segment_supported(int scene_id) { return rm_interval_supported(scene_id); }

int rm_segment_sdf_eval(int scene_id, const double* segs, size_t n, double* out)
{
    SoundCall c;
    int rc = c.open(scene_id, no_config, nullptr, nullptr, n, segs && out, "NULL buffer");
    if (rc || !c.prog) return rc;
    Staged st(*c.e);
    const double* d_segs = st.in(stage_in[0], segs, n * 64);
    double* d_out = st.out(stage_out[0], out, n * 32);
    if ((rc = st.begin())) return rc;
    hipLaunchKernelGGL(rm::segment_sdf_kernel, dim3(rm::grid_of(n)), dim3(rm::kSegmentBlock), 0, lib_stream(), c.prog, d_segs, n, d_out);
    HIP_TRY(hipGetLastError());
    return st.finish();
}

int rm_segment_march_rays(int scene_id, const RmSegmentConfig* cfg, const double* origins, const double* dirs, size_t n,
                          double* t, int32_t* iters, double* cursor)
{
    rm::SegmentParams P;
    SoundCall c;
    int rc = c.open(scene_id, [&] { return segment_params(scene_id, cfg, &P); }, nullptr, nullptr, n, origins && dirs && t, "NULL buffer");
    if (rc || !c.prog) return rc;
    Staged st(*c.e);
    const double* d_origins = st.in(stage_in[0], origins, n * 24);
    const double* d_dirs = st.in(stage_in[1], dirs, n * 24);
    double* d_t = st.out(stage_out[0], t, n * 8);
    int32_t* d_iters = st.out(stage_out[1], iters, n * 4);
    double* d_cursor = st.out(stage_out[2], cursor, n * 8);
    if ((rc = st.begin())) return rc;
    hipLaunchKernelGGL(rm::segment_march_kernel, dim3(rm::grid_of(n)), dim3(rm::kSegmentBlock), 0, lib_stream(), c.prog, P, d_origins,
                       d_dirs, n, d_t, d_iters, d_cursor);
    HIP_TRY(hipGetLastError());
    return st.finish();
}

int rm_segment_render(const RmFrameDesc* d, const RmSegmentConfig* cfg, double* depth, uint8_t* hit, int32_t* iters,
                      double* cursor, RmTiming* timing)
{
    if (!d) return fail(RM_E_BAD_ARG, "desc is NULL");
    rm::SegmentParams P;
    const size_t n = (size_t)d->width * (size_t)d->rows;
    SoundCall c;
    int rc = c.open(d->scene_id, [&] { return segment_params(d->scene_id, cfg, &P); }, d, timing, n, depth && hit,
                    "depth and hit are required");
    if (rc || !c.prog) return rc;
    Staged st(*c.e);
    double* d_depth = st.out(stage_out[0], depth, n * 8);
    uint8_t* d_hit = st.out(stage_out[1], hit, n);
    int32_t* d_iters = st.out(stage_out[2], iters, n * 4);
    double* d_cursor = st.out(stage_out[3], cursor, n * 8);
    if ((rc = st.begin())) return rc;
    const rm::CameraParams cam = camera_of(d->cam);
    rc = once_or_timed(*c.e, timing, lib_stream(), [&] {
        hipLaunchKernelGGL(rm::segment_render_kernel, dim3(rm::grid_of(n)), dim3(rm::kSegmentBlock), 0, lib_stream(), c.prog, P, cam,
                           d->width, d->height, d->row0, n, d_depth, d_hit, d_iters, d_cursor);
        HIP_TRY(hipGetLastError());
        return (int)RM_OK;
    });
    return rc ? rc : st.finish();
}

}  // extern "C"
