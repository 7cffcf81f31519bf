// rm_certify.hip -- the certified first hit on the device (rm_certify.h; rm_certify_* in include/rm_hip.h).
//
// As rm_segment.hip: one ray per lane, 256-thread workgroups, the scene program in LDS and every instruction word moved
// to a scalar register, so the opcode dispatch is a chain of scalar branches.  Each trip of the march is two dependent
// passes over the instruction words: the dual-interval program over the probe, then the interval program at the probe's
// end (a degenerate box).  The loop is per lane; a wave runs as long as its longest ray, at most `max_steps` trips
// (RM_INTERVAL_MAX_STEPS).
#include "rm_kernels.h"
#include "rm_certify.h"

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

// rm_capi.hip has validated the arguments; `prog` is the device copy of the scene's ProgramImage, n > 0
hipError_t launch_certify_march(const void* prog, const CertifyParams& P, const double* origins, const double* dirs, size_t n,
                                double* t_lo, double* t_hi, uint8_t* status, int32_t* steps, hipStream_t s)
{
    hipLaunchKernelGGL(certify_march_kernel, dim3(grid_of(n)), dim3(kCertifyBlock), 0, s, prog, P, origins, dirs, n, t_lo, t_hi,
                       status, steps);
    return hipGetLastError();
}

hipError_t launch_certify_render(const void* prog, const CertifyParams& P, const CameraParams& cam, int width, int height,
                                 int row0, int rows, double* t_lo, double* t_hi, uint8_t* status, int32_t* steps, hipStream_t s)
{
    const size_t n = (size_t)width * (size_t)rows;
    hipLaunchKernelGGL(certify_render_kernel, dim3(grid_of(n)), dim3(kCertifyBlock), 0, s, prog, P, cam, width, height, row0, n,
                       t_lo, t_hi, status, steps);
    return hipGetLastError();
}

}  // namespace rm
