// rm_strategy_tu.hip -- the strategy-program interpreter's kernels, one object per scene (compile with
// -DRM_SCENE_ID=<0..19>, -DRM_SCENE_PROGRAM or -DRM_SCENE_PROGRAM -DRM_SCENE_PROGRAM_EXT like rm_scene_tu.hip).
// Instantiates exactly three kernels for StratProgram (rm_strategy_program.h) -- render_kernel for one frame and for a
// batch, whole evaluations, 64x4 tiles, and march_rays_kernel -- and exports their launchers through
// rm::strategy_launchers_<id>() / _program() / _program_ext().  No resume, team, interleaved or single-launch form: a
// frame with a program strategy is one plain render pass (rm_launch_plan.h).
#include "rm_kernels.h"
#if defined(RM_SCENE_PROGRAM)
#include "rm_scene_program.h"
#endif
#include "rm_strategy_program.h"

#if !defined(RM_SCENE_ID) && !defined(RM_SCENE_PROGRAM)
#error "compile with -DRM_SCENE_ID=<scene id> or -DRM_SCENE_PROGRAM"
#endif

namespace rm {

#if defined(RM_SCENE_PROGRAM_EXT)
using SceneT = SceneExtProgram;
#elif defined(RM_SCENE_PROGRAM)
using SceneT = SceneProgram;
#else
template <int ID> struct SceneById;
#define RM_X(id, S) template <> struct SceneById<id> { using type = S; };
RM_SCENE_LIST(RM_X)
#undef RM_X
using SceneT = SceneById<RM_SCENE_ID>::type;
#endif

using FrameKernel = void (*)(KernelArgs);

static FrameKernel render_fn(int batch)
{
    return batch ? render_kernel<SceneT, StratProgram, 4, false, true> : render_kernel<SceneT, StratProgram, 4, false, false>;
}

static hipError_t render(const KernelArgs& a, int grid, hipStream_t s)
{
    if (!a.strategy_data || a.interleave || a.tile_h != 4 || a.suspend_after != 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(render_fn(a.frames != nullptr), dim3(grid), dim3(64 * kWavesPerWG), sp_register_bytes(64 * kWavesPerWG), s, a);
    return hipGetLastError();
}

static hipError_t occupancy(int batch, int* blocks)
{
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks, render_fn(batch), 64 * kWavesPerWG, sp_register_bytes(64 * kWavesPerWG));
}

static hipError_t march_rays(const MarchCfg& cfg, const double* o, const double* d, size_t n, uint8_t* hit, double* t,
                             int32_t* iters, double* fs, const void* scene_data, const void* strategy_data, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    if (!strategy_data) return hipErrorInvalidValue;
    hipLaunchKernelGGL((march_rays_kernel<SceneT, StratProgram>), dim3((unsigned)((n + 63) / 64)), dim3(64), sp_register_bytes(64), s, cfg, o, d, n, hit,
                       t, iters, fs, scene_data, strategy_data);
    return hipGetLastError();
}

#if defined(RM_SCENE_PROGRAM_EXT)
#define RM_LAUNCHERS_FN strategy_launchers_program_ext
#elif defined(RM_SCENE_PROGRAM)
#define RM_LAUNCHERS_FN strategy_launchers_program
#else
#define RM_CAT2(a, b) a##b
#define RM_CAT(a, b) RM_CAT2(a, b)
#define RM_LAUNCHERS_FN RM_CAT(strategy_launchers_, RM_SCENE_ID)
#endif
// a host function (not a const global: hipcc would try to emit that for the device too)
const StrategyProgramLaunchers* RM_LAUNCHERS_FN()
{
    static const StrategyProgramLaunchers l = { render, occupancy, march_rays };
    return &l;
}

}  // namespace rm
