// rm_segment.hip -- the sound segment tracer on the device (rm_segment.h; rm_segment_* in include/rm_hip.h).
//
// As rm_interval.hip: one ray (or one segment) per lane, 256-thread workgroups, the scene program in LDS and every
// instruction word moved to a scalar register, so the opcode dispatch is a chain of scalar branches.  Each trip of the
// trace is two dependent passes over the instruction words: the interval program at the cursor (a degenerate box), then
// the dual-interval program over the probe segment.  The loop is per lane; a wave runs as long as its longest ray, at
// most `budget` trips (RM_SEGMENT_MAX_STEPS).
#include "rm_kernels.h"
#include "rm_segment.h"

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

// rm_capi.hip has validated the arguments; `prog` is the device copy of the scene's ProgramImage, n > 0
hipError_t launch_segment_sdf(const void* prog, const double* segs, size_t n, double* out, hipStream_t s)
{
    hipLaunchKernelGGL(segment_sdf_kernel, dim3(grid_of(n)), dim3(kSegmentBlock), 0, s, prog, segs, n, out);
    return hipGetLastError();
}

hipError_t launch_segment_march(const void* prog, const SegmentParams& P, const double* origins, const double* dirs, size_t n,
                                double* t, int32_t* iters, double* cursor, hipStream_t s)
{
    hipLaunchKernelGGL(segment_march_kernel, dim3(grid_of(n)), dim3(kSegmentBlock), 0, s, prog, P, origins, dirs, n, t, iters,
                       cursor);
    return hipGetLastError();
}

hipError_t launch_segment_render(const void* prog, const SegmentParams& P, const CameraParams& cam, int width, int height,
                                 int row0, int rows, double* depth, uint8_t* hit, int32_t* iters, double* cursor, hipStream_t s)
{
    const size_t n = (size_t)width * (size_t)rows;
    hipLaunchKernelGGL(segment_render_kernel, dim3(grid_of(n)), dim3(kSegmentBlock), 0, s, prog, P, cam, width, height, row0, n,
                       depth, hit, iters, cursor);
    return hipGetLastError();
}

}  // namespace rm
