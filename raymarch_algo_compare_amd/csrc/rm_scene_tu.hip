// rm_scene_tu.hip -- one translation unit per scene (compile with -DRM_SCENE_ID=<0..19>).
// Instantiates render / march_rays kernels for every strategy and the sdf_eval and capture
// kernels of that scene, and exports their launchers through rm::scene_launchers_<id>().
// With -DRM_SCENE_PROGRAM instead: the same kernels for the scene-program interpreter (rm_scene_program.h), exported
// through rm::scene_launchers_program(); no single-launch pipeline and no team forms.  With -DRM_SCENE_PROGRAM_EXT as
// well: the interpreter with the four ops beyond primitives.py (SceneExtProgram), exported through rm::scene_launchers_program_ext().
#include "rm_kernels.h"
#if defined(RM_SCENE_PROGRAM)
#include "rm_scene_program.h"
#else
#include "rm_pipeline.h"
#endif

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

constexpr bool kIter = SceneIterative<SceneT>::value;

// ---- choosing an instantiation: written once per kernel family, as the kernel's address.  A launch and the occupancy
// query that sizes its grid go through the same function, so they cannot name different instantiations.
template <class S> struct Tag { using type = S; };

// f(Tag<Strat>()) for the strategy with this id; `none` for an id this build has no kernels for
template <class R, class F>
static R with_strategy(int strategy, R none, F f)
{
    switch (strategy) {
#define RM_X(id, S) \
    case id: return f(Tag<S>());
        RM_STRATEGY_LIST(RM_X)
#undef RM_X
    }
    return none;
}

// f(INTERLEAVE, BATCH) as compile-time constants; a scene without a resumable SDF has no INTERLEAVE form
template <class F>
static auto with_mode(int interleave, int batch, F f)
{
    using I = std::integral_constant<bool, kIter>;
    using N = std::false_type;
    if (batch) return kIter && interleave ? f(I(), std::true_type()) : f(N(), std::true_type());
    return kIter && interleave ? f(I(), N()) : f(N(), N());
}

using FrameKernel = void (*)(KernelArgs);        // render_kernel, pipeline_kernel
using PassKernel = void (*)(KernelArgs, int);    // resume_kernel, resume_team_kernel

static FrameKernel render_fn(int strategy, int interleave, int batch)      // 64x4 tiles always
{
    return with_strategy(strategy, FrameKernel(), [&](auto t) {
        using S = typename decltype(t)::type;
        return with_mode(interleave, batch, [](auto il, auto b) -> FrameKernel { return render_kernel<SceneT, S, 4, il(), b()>; });
    });
}

static PassKernel resume_fn(int strategy, int interleave, int batch)
{
    return with_strategy(strategy, PassKernel(), [&](auto t) {
        using S = typename decltype(t)::type;
        return with_mode(interleave, batch, [](auto il, auto b) -> PassKernel { return resume_kernel<SceneT, S, il(), b()>; });
    });
}

static PassKernel resume_team_fn(int strategy, int batch)      // nullptr: the scene has no team form
{
    return with_strategy(strategy, PassKernel(), [&](auto t) -> PassKernel {
        using S = typename decltype(t)::type;
        if constexpr (kIter) return batch ? resume_team_kernel<SceneT, S, true> : resume_team_kernel<SceneT, S, false>;
        return nullptr;
    });
}

template <class K, class... A>
static hipError_t launch(K kernel, int grid, int block, hipStream_t s, const A&... args)
{
    if (!kernel) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, s, args...);
    return hipGetLastError();
}

template <class K>
static hipError_t blocks_per_cu(K kernel, int block, int* blocks)
{
    if (!kernel) return hipErrorInvalidValue;
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks, kernel, block, 0);
}

static hipError_t render(int strategy, const KernelArgs& a, int grid, hipStream_t s)
{
    return launch(render_fn(strategy, a.interleave, a.frames != nullptr), grid, 64 * kWavesPerWG, s, a);
}

static hipError_t occupancy(int strategy, int interleave, int batch, int* blocks)
{
    return blocks_per_cu(render_fn(strategy, interleave, batch), 64 * kWavesPerWG, blocks);
}

static hipError_t resume(int strategy, int level, const KernelArgs& a, int grid, hipStream_t s)
{
    return launch(resume_fn(strategy, a.interleave, a.frames != nullptr), grid, 64 * kWavesPerWG, s, a, level);
}

static hipError_t resume_team(int strategy, int level, const KernelArgs& a, int grid, hipStream_t s)
{
    return launch(resume_team_fn(strategy, a.frames != nullptr), grid, 64 * kTeam, s, a, level);
}

#if defined(RM_SCENE_PROGRAM)
#define RM_PIPELINE_FNS nullptr, nullptr
#define RM_SPLIT_FNS nullptr, nullptr, nullptr
#else
#define RM_PIPELINE_FNS pipeline, occupancy_pipeline
// One-row tiles (TILE_H = 1) are built for the scenes with a team form only: there a frame ends with its longest
// ray, and with 64x4 tiles that ray may sit in its tile's pixel pool for milliseconds behind lanes that older rays hold.
static FrameKernel pipeline_fn(int strategy, int tile_h, int interleave, int batch)
{
    return with_strategy(strategy, FrameKernel(), [&](auto t) -> FrameKernel {
        using S = typename decltype(t)::type;
        if constexpr (kIter) {
            if (tile_h == 1)
                return with_mode(interleave, batch, [](auto il, auto b) -> FrameKernel { return pipeline_kernel<SceneT, S, 1, il(), b()>; });
        }
        if (tile_h != 4) return nullptr;
        return with_mode(interleave, batch, [](auto il, auto b) -> FrameKernel { return pipeline_kernel<SceneT, S, 4, il(), b()>; });
    });
}

static hipError_t pipeline(int strategy, const KernelArgs& a, int grid, hipStream_t s)
{
    return launch(pipeline_fn(strategy, a.tile_h, a.interleave, a.frames != nullptr), grid, 64 * kPipeWaves, s, a);
}

static hipError_t occupancy_pipeline(int strategy, int interleave, int batch, int* blocks)
{
    // the TILE_H = 4 instantiation is asked about for one-row launches too: the grids the launch plan computes rest on it
    return blocks_per_cu(pipeline_fn(strategy, 4, interleave, batch), 64 * kPipeWaves, blocks);
}

// The split form of the single launch (rm_pipeline.h): producers and teams as two kernels.  Scenes with a team form only;
// the team kernel does not depend on the tile height or on the producers' evaluation mode.
static FrameKernel pipeline_producer_fn(int strategy, int tile_h, int interleave, int batch)
{
    return with_strategy(strategy, FrameKernel(), [&](auto t) -> FrameKernel {
        using S = typename decltype(t)::type;
        if constexpr (kIter) {
            if (tile_h == 1)
                return with_mode(interleave, batch, [](auto il, auto b) -> FrameKernel { return pipeline_producer_kernel<SceneT, S, 1, il(), b()>; });
            if (tile_h == 4)
                return with_mode(interleave, batch, [](auto il, auto b) -> FrameKernel { return pipeline_producer_kernel<SceneT, S, 4, il(), b()>; });
        }
        return nullptr;
    });
}

static FrameKernel pipeline_team_fn(int strategy, int batch)
{
    return with_strategy(strategy, FrameKernel(), [&](auto t) -> FrameKernel {
        using S = typename decltype(t)::type;
        if constexpr (kIter) return batch ? pipeline_team_kernel<SceneT, S, true> : pipeline_team_kernel<SceneT, S, false>;
        return nullptr;
    });
}

static hipError_t pipeline_producers(int strategy, const KernelArgs& a, int grid, hipStream_t s)
{
    return launch(pipeline_producer_fn(strategy, a.tile_h, a.interleave, a.frames != nullptr), grid, 64 * kPipeWaves, s, a);
}

static hipError_t pipeline_teams(int strategy, const KernelArgs& a, int grid, hipStream_t s)
{
    return launch(pipeline_team_fn(strategy, a.frames != nullptr), grid, 64 * kTeam, s, a);
}

// workgroups per compute unit of each of the two kernels (the launch's own instantiations)
static hipError_t occupancy_split(int strategy, int tile_h, int interleave, int batch, int* producers, int* teams)
{
    const hipError_t e = blocks_per_cu(pipeline_producer_fn(strategy, tile_h, interleave, batch), 64 * kPipeWaves, producers);
    return e != hipSuccess ? e : blocks_per_cu(pipeline_team_fn(strategy, batch), 64 * kTeam, teams);
}
#define RM_SPLIT_FNS (kIter ? pipeline_producers : nullptr), (kIter ? pipeline_teams : nullptr), (kIter ? occupancy_split : nullptr)
#endif

static int entry_bytes(int strategy)
{
    return with_strategy(strategy, 0, [](auto t) { return (int)sizeof(QEntry<typename decltype(t)::type>); });
}

static hipError_t sdf_eval(const double* xyz, size_t n, double* out, const void* scene_data, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    return launch(sdf_eval_kernel<SceneT>, (int)((n + 255) / 256), 256, s, xyz, n, out, scene_data);
}

static hipError_t march_rays(int strategy, const MarchCfg& cfg, const double* o, const double* d, size_t n,
                             uint8_t* hit, double* t, int32_t* iters, double* fs, const void* scene_data, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    return with_strategy(strategy, hipErrorInvalidValue, [&](auto tag) {
        return launch(march_rays_kernel<SceneT, typename decltype(tag)::type>, (int)((n + 63) / 64), 64, s, cfg, o, d, n, hit, t, iters, fs, scene_data, (const void*)nullptr);
    });
}

static hipError_t march_rays_team(int strategy, const MarchCfg& cfg, const double* o, const double* d, size_t n,
                                  uint8_t* hit, double* t, int32_t* iters, double* fs, unsigned long long* busy, int fillers,
                                  hipStream_t s)
{
    if (kIter && n == 0) return hipSuccess;
    return with_strategy(strategy, hipErrorInvalidValue, [&](auto tag) {
        if constexpr (kIter) {
            const int grid = (int)((unsigned)((n + 63) / 64) + (unsigned)(busy ? fillers : 0));
            return launch(march_rays_team_kernel<SceneT, typename decltype(tag)::type>, grid, 64 * kTeam, s, cfg, o, d, n, hit, t, iters, fs, busy);
        }
        return hipErrorInvalidValue;
    });
}

static hipError_t capture(const CaptureArgs& a, int nframes, hipStream_t s)
{
    const size_t n = (size_t)a.rows * (size_t)a.width;
    if (n == 0) return hipSuccess;
    if (nframes < 1 || nframes > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(capture_kernel<SceneT>, dim3((unsigned)((n + 255) / 256), (unsigned)nframes), dim3(256), 0, s, a);
    return hipGetLastError();
}

#if defined(RM_SCENE_PROGRAM)
static_assert(!kIter, "a scene program has no resumable evaluation");
#if defined(RM_SCENE_PROGRAM_EXT)
#define RM_LAUNCHERS_FN scene_launchers_program_ext
#else
#define RM_LAUNCHERS_FN scene_launchers_program
#endif
#else
#define RM_CAT2(a, b) a##b
#define RM_CAT(a, b) RM_CAT2(a, b)
#define RM_LAUNCHERS_FN RM_CAT(scene_launchers_, RM_SCENE_ID)
#endif
// a host function (not a const global: hipcc would try to emit that for the device too)
const SceneLaunchers* RM_LAUNCHERS_FN()
{
    static const SceneLaunchers l = { render, resume, kIter ? resume_team : nullptr, RM_PIPELINE_FNS, kIter,
                                      entry_bytes, occupancy, sdf_eval, march_rays, kIter ? march_rays_team : nullptr, capture,
                                      RM_SPLIT_FNS };
    return &l;
}

}  // namespace rm
