// rm_affine.hip -- the affine range and its march on the device (rm_affine.h; rm_affine_* in include/rm_hip.h).
//
// As rm_interval.hip: one ray (or one segment) per lane, 256-thread workgroups, the scene program in LDS and every
// instruction word moved to a scalar register, so the opcode dispatch is a chain of scalar branches.  `mode` is a kernel
// argument, so the second walk of RM_RANGE_MEET (the interval program over the same segment) sits behind a wave-uniform
// branch.  The march loop is per lane; a wave runs as long as its longest ray.
#include "rm_kernels.h"
#include "rm_affine.h"

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

// rm_capi.hip has validated the arguments; `prog` is the device copy of the scene's ProgramImage, n > 0
hipError_t launch_affine_range(const void* prog, int mode, const double* segs, size_t n, double* out_range, double* out_form,
                               hipStream_t s)
{
    hipLaunchKernelGGL(affine_range_kernel, dim3(grid_of(n)), dim3(kAffineBlock), 0, s, prog, mode, segs, n, out_range, out_form);
    return hipGetLastError();
}

hipError_t launch_affine_march(const void* prog, int mode, const IntervalParams& P, const double* origins, const double* dirs,
                               size_t n, double* t, int32_t* steps, hipStream_t s)
{
    hipLaunchKernelGGL(affine_march_kernel, dim3(grid_of(n)), dim3(kAffineBlock), 0, s, prog, mode, P, origins, dirs, n, t, steps);
    return hipGetLastError();
}

hipError_t launch_affine_render(const void* prog, int mode, const IntervalParams& P, const CameraParams& cam, int width, int height,
                                int row0, int rows, double* depth, uint8_t* hit, int32_t* steps, hipStream_t s)
{
    const size_t n = (size_t)width * (size_t)rows;
    hipLaunchKernelGGL(affine_render_kernel, dim3(grid_of(n)), dim3(kAffineBlock), 0, s, prog, mode, P, cam, width, height, row0, n,
                       depth, hit, steps);
    return hipGetLastError();
}

}  // namespace rm
