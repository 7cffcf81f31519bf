// rm_exact.hip -- the exact first hit on the device (rm_exact.h; rm_exact_* in include/rm_hip.h).
//
// One ray per lane, 256-thread workgroups, launched as rm_interval.hip launches: the prologue copies the scene program
// into LDS and the pow tables (the camera's normalisation) into their mirror; every instruction word is then read at a
// wave-uniform address and moved to a scalar register (ProgSrc), so both walks over the program -- the leaves and their
// roots, and the germ of the whole program at one root -- are chains of scalar branches.  Only the existence of a root
// and whether it beats the lane's best so far differ per lane, and those are predicated.  No per-lane memory: the germ
// stack is one 32-bit word, the saved points are register slots (Slots, rm_scene_program.h).
#include "rm_kernels.h"
#include "rm_exact.h"

namespace rm {

constexpr int kExactBlock = 256;

__global__ __launch_bounds__(kExactBlock) void exact_march_kernel(const void* prog, ExactParams P, const double* __restrict__ origins,
                                                                 const double* __restrict__ dirs, size_t n, double* __restrict__ t_out,
                                                                 double* __restrict__ normals, int32_t* __restrict__ leaf)
{
    SceneProgram::load(prog);
    rm_load_tables<SceneProgram>();
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const vec3 o = v3(origins[3 * i], origins[3 * i + 1], origins[3 * i + 2]);
    const vec3 d = v3(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]);      // as given
    const ExactHit h = exact_first_hit(ProgSrc{}, o, d, P.t_min, P.t_max);
    t_out[i] = h.t;
    if (normals) {
        normals[3 * i] = h.normal.x;
        normals[3 * i + 1] = h.normal.y;
        normals[3 * i + 2] = h.normal.z;
    }
    if (leaf) leaf[i] = h.leaf;
}

__global__ __launch_bounds__(kExactBlock) void exact_render_kernel(const void* prog, ExactParams P, CameraParams cam, int width,
                                                                  int height, int row0, size_t n, double* __restrict__ depth,
                                                                  uint8_t* __restrict__ hit, double* __restrict__ normal,
                                                                  int32_t* __restrict__ leaf)
{
    SceneProgram::load(prog);
    rm_load_tables<SceneProgram>();
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int py = row0 + (int)(i / (size_t)width), px = (int)(i % (size_t)width);
    double dp;
    uint8_t h;
    vec3 nv;
    int32_t lf;
    exact_pixel(ProgSrc{}, cam, width, height, px, py, P, &dp, &h, &nv, &lf);
    depth[i] = dp;
    hit[i] = h;
    if (normal) {
        normal[3 * i] = nv.x;
        normal[3 * i + 1] = nv.y;
        normal[3 * i + 2] = nv.z;
    }
    if (leaf) leaf[i] = lf;
}

static unsigned grid_of(size_t n) { return (unsigned)((n + kExactBlock - 1) / kExactBlock); }

// rm_capi.hip has validated the arguments; `prog` is the device copy of the scene's ProgramImage, n > 0
hipError_t launch_exact_march(const void* prog, const ExactParams& P, const double* origins, const double* dirs, size_t n, double* t,
                              double* normals, int32_t* leaf, hipStream_t s)
{
    hipLaunchKernelGGL(exact_march_kernel, dim3(grid_of(n)), dim3(kExactBlock), 0, s, prog, P, origins, dirs, n, t, normals, leaf);
    return hipGetLastError();
}

hipError_t launch_exact_render(const void* prog, const ExactParams& P, const CameraParams& cam, int width, int height, int row0,
                               int rows, double* depth, uint8_t* hit, double* normal, int32_t* leaf, hipStream_t s)
{
    const size_t n = (size_t)width * (size_t)rows;
    hipLaunchKernelGGL(exact_render_kernel, dim3(grid_of(n)), dim3(kExactBlock), 0, s, prog, P, cam, width, height, row0, n, depth,
                       hit, normal, leaf);
    return hipGetLastError();
}

}  // namespace rm
