// rm_interval.hip -- the interval first-hit oracle on the device (rm_interval.h; rm_interval_* in include/rm_hip.h).
//
// One ray (or one point box) per lane, 256-thread workgroups.  The prologue copies the scene program into LDS and the
// pow tables (pow_half, rm_pow of the extensions and of the camera's normalisation) into their mirrors; every
// instruction word is then read at a wave-uniform address and moved to a scalar register (SceneProgram, ProgSrc), so
// the opcode dispatch is a chain of scalar branches.  The march loop itself is per lane: the lanes of a wave leave it
// after different numbers of steps.
#include "rm_kernels.h"
#include "rm_interval.h"

namespace rm {

constexpr int kIntervalBlock = 256;

__global__ __launch_bounds__(kIntervalBlock) void interval_sdf_kernel(const void* prog, const double* __restrict__ lo,
                                                                     const double* __restrict__ hi, size_t n,
                                                                     double* __restrict__ out_lo, double* __restrict__ out_hi)
{
    SceneProgram::load(prog);
    rm_load_tables<SceneExtProgram>();      // the pow tables and, for RM_SOP_GYROID, sin / cos
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const IVec3 box = ivec3(iv(lo[3 * i], hi[3 * i]), iv(lo[3 * i + 1], hi[3 * i + 1]), iv(lo[3 * i + 2], hi[3 * i + 2]));
    const Ival r = program_eval_interval(ProgSrc{}, box);
    out_lo[i] = r.lo;
    out_hi[i] = r.hi;
}

__global__ __launch_bounds__(kIntervalBlock) void interval_march_kernel(const void* prog, IntervalParams P,
                                                                       const double* __restrict__ origins,
                                                                       const double* __restrict__ dirs, size_t n,
                                                                       double* __restrict__ t_out, int32_t* __restrict__ steps,
                                                                       double* __restrict__ normals)
{
    SceneProgram::load(prog);
    rm_load_tables<SceneExtProgram>();      // the pow tables and, for RM_SOP_GYROID, sin / cos
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const vec3 o = v3(origins[3 * i], origins[3 * i + 1], origins[3 * i + 2]);
    const vec3 d = v3(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]);      // as given: first_hit does not normalise
    int32_t s = 0;
    const double t = interval_first_hit(ProgSrc{}, o, d, P, &s);
    t_out[i] = t;
    if (steps) steps[i] = s;
    if (normals) {
        const vec3 nv = t < __builtin_inf() ? interval_normal(ProgSrc{}, o, d, t, P.normal_eps) : v3(0.0, 0.0, 0.0);
        normals[3 * i] = nv.x;
        normals[3 * i + 1] = nv.y;
        normals[3 * i + 2] = nv.z;
    }
}

__global__ __launch_bounds__(kIntervalBlock) void interval_render_kernel(const void* prog, IntervalParams P, CameraParams cam,
                                                                        int width, int height, int row0, size_t n,
                                                                        double* __restrict__ depth, uint8_t* __restrict__ hit,
                                                                        double* __restrict__ normal, int32_t* __restrict__ steps)
{
    SceneProgram::load(prog);
    rm_load_tables<SceneExtProgram>();      // the pow tables and, for RM_SOP_GYROID, sin / cos
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int py = row0 + (int)(i / (size_t)width), px = (int)(i % (size_t)width);
    double dp;
    uint8_t h;
    vec3 nv;
    int32_t s;
    interval_pixel(ProgSrc{}, cam, width, height, px, py, P, normal != nullptr, &dp, &h, &nv, &s);
    depth[i] = dp;
    hit[i] = h;
    if (normal) {
        normal[3 * i] = nv.x;
        normal[3 * i + 1] = nv.y;
        normal[3 * i + 2] = nv.z;
    }
    if (steps) steps[i] = s;
}

static unsigned grid_of(size_t n) { return (unsigned)((n + kIntervalBlock - 1) / kIntervalBlock); }

// rm_capi.hip has validated the arguments; `prog` is the device copy of the scene's ProgramImage, n > 0
hipError_t launch_interval_sdf(const void* prog, const double* lo, const double* hi, size_t n, double* out_lo, double* out_hi,
                               hipStream_t s)
{
    hipLaunchKernelGGL(interval_sdf_kernel, dim3(grid_of(n)), dim3(kIntervalBlock), 0, s, prog, lo, hi, n, out_lo, out_hi);
    return hipGetLastError();
}

hipError_t launch_interval_march(const void* prog, const IntervalParams& P, const double* origins, const double* dirs, size_t n,
                                 double* t, int32_t* steps, double* normals, hipStream_t s)
{
    hipLaunchKernelGGL(interval_march_kernel, dim3(grid_of(n)), dim3(kIntervalBlock), 0, s, prog, P, origins, dirs, n, t, steps,
                       normals);
    return hipGetLastError();
}

hipError_t launch_interval_render(const void* prog, const IntervalParams& P, const CameraParams& cam, int width, int height,
                                  int row0, int rows, double* depth, uint8_t* hit, double* normal, int32_t* steps, hipStream_t s)
{
    const size_t n = (size_t)width * (size_t)rows;
    hipLaunchKernelGGL(interval_render_kernel, dim3(grid_of(n)), dim3(kIntervalBlock), 0, s, prog, P, cam, width, height, row0, n,
                       depth, hit, normal, steps);
    return hipGetLastError();
}

}  // namespace rm
