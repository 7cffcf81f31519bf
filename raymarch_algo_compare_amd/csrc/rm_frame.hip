// rm_frame.hip -- the march's host side: the frame engine that performs a launch plan (rm_launch_plan.h) and the entry
// points of the C ABI (include/rm_hip.h) that go through it -- frames, batches, per-ray calls, capture, pass timing and the
// debug trace.
//
// The policy of a launch is the plan's; this file owns what the plan is performed WITH.  Every cache below is one small
// struct that holds its device buffers, its key (PerSession: forgotten by rm_shutdown) and the one or two functions that
// may touch them; launch_frame is the list of steps that calls them in order.  Frames share one workspace, so they are
// serialised on the device (launch).  Lock, device, stream, staging and timed() come from rm_capi.hip through
// rm_capi_internal.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/rm_hip.h"
#include "rm_kernels.h"
#include "rm_launch_plan.h"
#include "rm_pipeline.h"
#include "rm_scene_program.h"
#include "rm_strategy_program.h"
#include "rm_capi_internal.h"

#include <map>
#include <memory>
#include <mutex>

static_assert(RM_HIST_BINS == rm::kHistBins, "histogram size mismatch between ABI and kernels");

using namespace rm::capi;

// The strategy-program interpreter's kernels, one table per scene object (rm_strategy_tu.hip).
namespace rm {
#if defined(RM_DEV_STRATEGIES)
#define RM_SP_DECL(name) const StrategyProgramLaunchers* name() __attribute__((weak));
#else
#define RM_SP_DECL(name) const StrategyProgramLaunchers* name();
#endif
#define RM_X(id, S) RM_SP_DECL(strategy_launchers_##id)
RM_SCENE_LIST(RM_X)
#undef RM_X
RM_SP_DECL(strategy_launchers_program)
RM_SP_DECL(strategy_launchers_program_ext)
#undef RM_SP_DECL
}  // namespace rm

namespace {

// ---- strategy programs (rm_strategy_program.h) --------------------------------------------------------------------------
// A registered program: its validated image on the host, and the device copy the first launch that runs it makes (under
// the library's lock; freed by rm_strategy_program_destroy and at the end of the session).  Nothing else is kept per
// program id: a program frame plans without the caches that are keyed by strategy (rm_launch_plan.h).
struct StrategyProgram {
    std::unique_ptr<rm::StrategyImage> img;
    void* dev = nullptr;
};
std::mutex g_sp_mu;                                   // guards the three below; taken after the library's lock where both are held
std::map<int32_t, StrategyProgram> g_strategy_programs;
int32_t g_next_strategy_program = RM_STRATEGY_PROGRAM_BASE;      // ids are never reused
struct StrategyProgramCopies final : SessionItem {
    void end() override      // programs stay registered; their device copies are made again after the next rm_init
    {
        std::lock_guard<std::mutex> lk(g_sp_mu);
        for (auto& kv : g_strategy_programs)
            if (kv.second.dev) { (void)hipFree(kv.second.dev); kv.second.dev = nullptr; }
    }
} g_strategy_program_copies;

int no_such_strategy_program(int id)
{
    return fail(RM_E_BAD_STRATEGY, "strategy program %d does not exist (never created, or destroyed)", id);
}

// A compiled strategy kernel, or a live strategy program.
int check_strategy(int id)
{
    if (rm::is_strategy_program(id)) {
        std::lock_guard<std::mutex> lk(g_sp_mu);
        return g_strategy_programs.count(id) ? RM_OK : no_such_strategy_program(id);
    }
    if (id < 0 || id >= RM_NUM_STRATEGY_KERNELS) return fail(RM_E_BAD_STRATEGY, "strategy_id %d out of range", id);
    return RM_OK;
}

// The launch data of strategy `id` (KernelArgs.strategy_data; under the library's lock with the device selected): a
// program's device image, copied by its first launch; nullptr for a compiled strategy.
int strategy_data(int id, const void** data)
{
    *data = nullptr;
    if (!rm::is_strategy_program(id)) return RM_OK;
    std::lock_guard<std::mutex> lk(g_sp_mu);
    auto it = g_strategy_programs.find(id);
    if (it == g_strategy_programs.end()) return no_such_strategy_program(id);
    StrategyProgram& p = it->second;
    if (!p.dev) {
        void* dev = nullptr;
        HIP_TRY(hipMalloc(&dev, sizeof(rm::StrategyImage)));
        const hipError_t e = hipMemcpy(dev, p.img.get(), sizeof(rm::StrategyImage), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(dev);
            return fail(RM_E_HIP, "strategy program %d: copy to the device failed: %s", id, hipGetErrorString(e));
        }
        p.dev = dev;
    }
    *data = p.dev;
    return RM_OK;
}

// The interpreter's kernels of scene `id` (check_scene has accepted it); nullptr in a development library without them.
const rm::StrategyProgramLaunchers* strategy_launchers(int scene_id)
{
#if defined(RM_DEV_STRATEGIES)
#define RM_SP_GET(name) (rm::name ? rm::name() : nullptr)
#else
#define RM_SP_GET(name) rm::name()
#endif
    if (is_program_id(scene_id)) {
        bool ext = false;
        (void)program_exists(scene_id, &ext);
        return ext ? RM_SP_GET(strategy_launchers_program_ext) : RM_SP_GET(strategy_launchers_program);
    }
    switch (scene_id) {
#define RM_X(id, S) case id: return RM_SP_GET(strategy_launchers_##id);
        RM_SCENE_LIST(RM_X)
#undef RM_X
    }
#undef RM_SP_GET
    return nullptr;
}

constexpr size_t kStatsBlockBytes = sizeof(unsigned long long) * rm::kStatsWords;   // the canonical block (what the host reads)
constexpr size_t kStatsBytes = kStatsBlockBytes * rm::kStatsBlocks;                 // + the partial blocks (device buffer size)

rm::MarchCfg to_cfg(const RmMarchConfig& m)
{
    rm::MarchCfg c;
    c.hit_threshold = m.hit_threshold;
    c.max_distance = m.max_distance;
    c.lipschitz = m.lipschitz;
    c.max_iterations = m.max_iterations;
    c.full = m.full ? 1 : 0;
    c.prm = rm::default_strat_params();
    if (m.use_params) {
        static_assert(sizeof(RmStrategyParams) == sizeof(rm::StratParams), "RmStrategyParams and rm::StratParams must match");
        memcpy(&c.prm, &m.params, sizeof c.prm);
    }
    return c;
}

// The launch plan of `d` (rm_launch_plan.h) with this device's and this scene's facts.
rm::LaunchPlan plan_for(const RmFrameDesc* d, int batch_frames = 0, const RmMarchConfig* configs = nullptr)
{
    const rm::SceneLaunchers* const sc = launchers(d->scene_id);
    const int strategy = d->strategy_id;
    rm::DeviceFacts f;
    f.cus = device_prop().multiProcessorCount;
    if (rm::is_strategy_program(strategy)) {      // the interpreter has a render kernel and nothing else (plan_strategy_program)
        const rm::StrategyProgramLaunchers* const sp = strategy_launchers(d->scene_id);
        f.per_cu = [sp](rm::OccKernel, int, int, int batch) {
            int n = 0;
            return sp && sp->occupancy(batch, &n) == hipSuccess ? n : 0;
        };
        return rm::plan_launch(*d, f, batch_frames, configs);
    }
    f.has_teams = sc->has_teams;
    f.has_split = sc->pipeline_teams && sc->pipeline_producers;
    f.has_resume_team = sc->resume_team != nullptr;
    f.entry_bytes = sc->entry_bytes(strategy);
    int split[2] = { -1, -1 };      // the split form's two kernels answer in one query
    f.per_cu = [sc, strategy, &split](rm::OccKernel k, int tile_h /*render and pipeline answer for 64x4 tiles*/, int interleave, int batch) {
        if (k == rm::OccKernel::split_producers || k == rm::OccKernel::split_teams) {
            if (split[0] < 0 && sc->occupancy_split(strategy, tile_h, interleave, batch, &split[0], &split[1]) != hipSuccess)
                split[0] = split[1] = 0;
            return split[k == rm::OccKernel::split_teams];
        }
        int n = 0;
        const hipError_t e = k == rm::OccKernel::pipeline ? sc->occupancy_pipeline(strategy, interleave, batch, &n)
                                                          : sc->occupancy(strategy, interleave, batch, &n);
        return e == hipSuccess ? n : 0;
    };
    return rm::plan_launch(*d, f, batch_frames, configs);
}

// The workspace of the frame calls: the maps of a frame (or a batch) that is staged back to the host, ...
struct FrameBufs {
    WsBuf depth, iters, hit, traw, fs, bvar, evals;
    WsBuf frames;                 // rm_render_batch: the device frame table
    WsBuf busy;                   // rm_march_rays_team: the counter its filler workgroups watch (its own word: a frame in flight owns the control block)
    WsBuf cap_out[5], cap_cams;   // rm_capture / rm_shade_frames: geom, normal, depth, color, evals maps; the frames' cameras
    Events<2> batch_ev;           // rm_render_batch: around the batch
} g;

// ... and the library's own statistics buffer, which frames without a caller's buffer count into.
struct OwnStats {
    WsBuf buf;
    struct Key { bool clean = false; };      // left zeroed by a fused-reduce frame (reset)
    PerSession<Key> key;
    int get(unsigned long long** p)
    {
        if (int rc = buf.ensure(kStatsBytes)) return rc;
        *p = (unsigned long long*)buf.p;
        return RM_OK;
    }
    // A fused-reduce frame leaves the statistics buffer zeroed where the next frame needs it: no reduce launch, and --
    // for the library's own buffer, which nobody else writes -- no memset either.  A caller's buffer is always cleared
    // (its contents are not ours to trust).
    int reset(const rm::KernelArgs& a, hipStream_t s)
    {
        const bool own = a.stats == (unsigned long long*)buf.p;
        if (!(own && key.clean)) HIP_TRY(hipMemsetAsync(a.stats, 0, kStatsBytes, s));
        if (own) key.clean = a.fused_reduce != 0;
        return RM_OK;
    }
} g_stats;

// Kernel arguments of one frame of `d` (a batch sets frames / nframes / full / evals itself): pointers and plan fields.
// stats: the caller's statistics buffer, or NULL for the library's own.
int make_args(const RmFrameDesc* d, const rm::LaunchPlan& p, float* depth, int32_t* iters, uint8_t* hit, double* traw, double* fs,
              long long* bvar, unsigned long long* stats, rm::KernelArgs* a)
{
    memset(a, 0, sizeof *a);
    if (int rc = scene_data(d->scene_id, &a->scene_data)) return rc;
    if (int rc = strategy_data(d->strategy_id, &a->strategy_data)) return rc;
    if (!stats)
        if (int rc = g_stats.get(&stats)) return rc;
    a->single.cam = camera_of(d->cam);
    a->single.cfg = to_cfg(d->march);
    a->frames = nullptr;
    a->nframes = 1;
    a->full = d->march.full ? 1 : 0;
    a->width = d->width; a->height = d->height; a->row0 = d->row0; a->rows = d->rows;
    a->tiles_x = p.tiles_x;
    a->tiles_y = p.tiles_y;
    a->tiles_per_frame = a->tiles_x * a->tiles_y;
    a->tile_h = p.tile_h;
    a->refill_min = p.refill_min;
    a->hist_bins = rm::kHistBins;
    a->interleave = p.interleave;
    a->age_prio = d->age_priority > 0 ? d->age_priority : 0;
    if (d->band_rows > 0 && d->band_stride > 1) {
        a->band_rows = d->band_rows; a->band_stride = d->band_stride; a->band_offset = d->band_offset;
    }
    a->depth = depth; a->iters = iters; a->hit = hit; a->t_raw = traw; a->final_sdf = fs;
    a->block_var = bvar; a->stats = stats;
    a->fused_reduce = p.fused_reduce;
    if (p.park[0] > 0) {
        a->suspend_after = p.park[0];
        a->suspend_queue = 0;
    }
    if (p.single) {
        a->team_wgs = p.team_wgs;
        a->producer_waves = p.producer_waves;
        a->late_team_first = p.late_team_first;
        a->early_exit_wgs = p.early_exit_wgs;
        a->exit_backlog = p.exit_backlog;
        a->keep_busy = p.keep_busy;
        a->early_trips = p.early_trips;
        a->early_handover = p.early_handover;
        a->suspend_after2 = p.suspend_after2;
        a->q0_detach = p.q0_detach;
        a->q0_first = p.q0_first;
        a->q0_refill_min = p.q0_refill_min;
        a->q0_retry = p.q0_retry;
        a->team_retry = p.team_retry;
        a->team_steal = p.team_steal;
        a->max_spins = p.max_spins;
        a->team_prio = p.team_prio;
    }
    return RM_OK;
}

// Longest-first tile order from last frame's per-tile cost: a counting sort by descending cost
// (one workgroup; ties keep no particular order -- the order only affects the schedule).
__global__ __launch_bounds__(1024) void order_tiles_kernel(const int32_t* __restrict__ cost, int32_t* __restrict__ order, int n)
{
    constexpr int BINS = 1024;
    __shared__ int hist[BINS];
    for (int b = threadIdx.x; b < BINS; b += blockDim.x) hist[b] = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += blockDim.x) atomicAdd(&hist[min(max(cost[i], 0), BINS - 1)], 1);
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int b = BINS - 1; b >= 0; --b) { const int c = hist[b]; hist[b] = run; run += c; }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int pos = atomicAdd(&hist[min(max(cost[i], 0), BINS - 1)], 1);
        order[pos] = i;
    }
}

// Static priorities: tiles nearer the image centre (where the camera looks) get a higher cost.  xweight = 1: centre-out
// (a disc grows from the middle); xweight < 1 flattens the disc into an ellipse -- at 1/16 the middle ROWS go first, centre
// columns leading: where the geometry runs to the horizon (planes, pillar grids) the long rays lie along the horizon line.
__global__ void center_cost_kernel(int32_t* __restrict__ cost, int tiles_x, int tiles_y, int nframes, int tile_h, int width, int height,
                                   int row0, int band_rows, int band_stride, int band_offset, float xweight)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= tiles_x * tiles_y * nframes) return;
    const int tf = t % (tiles_x * tiles_y);               // tile ids run frame-major: every frame of a batch centre-out
    const int tx = tf % tiles_x, ty = tf / tiles_x;
    const int y0 = ty * tile_h;
    const int gy = band_rows > 0 ? row0 + ((y0 / band_rows) * band_stride + band_offset) * band_rows + (y0 % band_rows) : row0 + y0;
    const float cx = (tx * 64 + 32 - 0.5f * width) / (0.5f * height);      // both axes in units of half the image height
    const float cy = (gy + 0.5f * tile_h - 0.5f * height) / (0.5f * height);
    const float r = sqrtf(xweight * cx * cx + cy * cy);
    cost[t] = max(0, 1023 - (int)(r * 256.0f));
}

// 8x4-block variance numerators 32*sum(x^2) - sum(x)^2 of the finished iteration map (core/types.py:125-133),
// one thread per full block: used instead of the in-flush reduction when rays were parked (their
// pixels are not in the tile when it is flushed).
__global__ void block_var_kernel(const int32_t* __restrict__ iters, int width, int rows, int nframes,
                                 long long* __restrict__ out)
{
    const int bw = width >> 3, bh = rows >> 2;
    const long long n = (long long)bw * bh * nframes;
    const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n) return;
    const int f = (int)(b / ((long long)bw * bh));
    const int r = (int)(b - (long long)f * bw * bh);
    const int by = r / bw, bx = r - by * bw;
    const int32_t* p = iters + (size_t)f * (size_t)rows * (size_t)width + (size_t)(by * 4) * (size_t)width + (size_t)(bx * 8);
    long long S = 0, Q = 0;
#pragma unroll
    for (int y = 0; y < 4; ++y)
#pragma unroll
        for (int x = 0; x < 8; ++x) {
            const long long v = p[(size_t)y * (size_t)width + x];
            S += v; Q += v * v;
        }
    out[b] = 32 * Q - S * S;
}

// Sum the partial stats blocks into the canonical block 0 (totals: add; iter_max and the complemented iter_min: max).
__global__ void stats_reduce_kernel(unsigned long long* __restrict__ stats)
{
    const int w = blockIdx.x * blockDim.x + threadIdx.x;      // word index within a block
    if (w >= rm::kStatsWords || w == 0 || (w >= 6 && w < 10) || (w > 10 && w < rm::kStatsHead)) return;   // counters live in block 0 only
    unsigned long long acc = 0;
    const bool is_max = (w == 3 || w == 4);
    for (int p = 1; p <= rm::kStatsParts; ++p) {
        const unsigned long long v = stats[(size_t)p * rm::kStatsWords + w];
        acc = is_max ? (v > acc ? v : acc) : acc + v;
    }
    stats[w] = acc;
}
// ---- the frame engine's caches ---------------------------------------------------------------------------------------------

int order_tiles(const WsBuf& cost, WsBuf& order, int ntiles, hipStream_t s)
{
    hipLaunchKernelGGL(order_tiles_kernel, dim3(1), dim3(1024), 0, s, (const int32_t*)cost.p, (int32_t*)order.p, ntiles);
    HIP_TRY(hipGetLastError());
    return RM_OK;
}

// Tile order 1, longest first: every frame leaves its per-tile costs, and a frame of the same shape (frame_key) is
// ordered by them.
struct DynamicOrder {
    WsBuf cost, order;
    struct Key { long long shape[10] = { -1 }; bool valid = false; };
    PerSession<Key> key;
    // a.tile_cost: where this frame's costs go; a.tile_order: set when the previous frame's costs fit this one
    int apply(const RmFrameDesc* d, const rm::LaunchPlan& p, int ntiles, rm::KernelArgs& a, hipStream_t s)
    {
        int rc;
        if ((rc = cost.ensure((size_t)ntiles * 4)) || (rc = order.ensure((size_t)ntiles * 4))) return rc;
        long long shape[10];
        rm::frame_key(*d, p.tile_h, shape);
        if (key.valid && memcmp(shape, key.shape, sizeof shape) == 0) {
            if ((rc = order_tiles(cost, order, ntiles, s))) return rc;
            a.tile_order = (const int32_t*)order.p;
        }
        a.tile_cost = (int32_t*)cost.p;      // this frame's costs feed the next frame's order
        memcpy(key.shape, shape, sizeof shape);
        key.valid = true;
        return RM_OK;
    }
} g_dynamic_order;

// Tile orders 2 and 4: a static permutation of the frame shape (static_order_key), computed once and kept until the shape
// changes: no extra launch per frame.
struct StaticOrder {
    WsBuf cost, order;
    struct Key { long long shape[12] = { -1 }; bool valid = false; };
    PerSession<Key> key;
    int apply(const RmFrameDesc* d, const rm::LaunchPlan& p, int which, int ntiles, rm::KernelArgs& a, hipStream_t s)
    {
        long long shape[12];
        rm::static_order_key(*d, p.tile_h, a.nframes, which, shape);
        int rc;
        if ((rc = order.ensure((size_t)ntiles * 4))) return rc;
        if (!key.valid || memcmp(shape, key.shape, sizeof shape) != 0) {
            if ((rc = cost.ensure((size_t)ntiles * 4))) return rc;
            hipLaunchKernelGGL(center_cost_kernel, dim3((ntiles + 255) / 256), dim3(256), 0, s, (int32_t*)cost.p, a.tiles_x,
                               a.tiles_y, a.nframes, p.tile_h, a.width, a.height, a.row0, a.band_rows, a.band_stride, a.band_offset,
                               which == 4 ? 1.0f / 16.0f : 1.0f);
            if ((rc = order_tiles(cost, order, ntiles, s))) return rc;
            memcpy(key.shape, shape, sizeof shape);
            key.valid = true;
        }
        a.tile_order = (const int32_t*)order.p;
        return RM_OK;
    }
} g_static_order;

// Long-ray suspension: the queues of the parked rays.  What is cleared before a launch, and what is remembered of the
// launch, is queue_step's (rm_launch_plan.h); nothing else writes a key.
constexpr long long kQueueCapMax = 1ll << 22;   // default entries per suspended-ray queue (a full queue leaves rays in place)
struct Queues {
    WsBuf buf[rm::kQueues];
    struct Key { rm::QueueKey of[rm::kQueues]; long long cap = kQueueCapMax; /* rm_set_queue_capacity */ };
    PerSession<Key> key;
    int step(int q, int writer, int stride, size_t need, hipStream_t s)
    {
        const size_t before = buf[q].cap;
        if (int rc = buf[q].ensure(need)) return rc;
        const rm::QueueStep st = rm::queue_step(key.of[q], writer, stride, need, before, buf[q].cap);
        if (st.clear) HIP_TRY(hipMemsetAsync(buf[q].p, 0, st.clear, s));
        key.of[q] = st.key;
        return RM_OK;
    }
    int prepare(const rm::LaunchPlan& p, rm::KernelArgs& a, hipStream_t s)
    {
        const long long total = (long long)a.rows * a.width * a.nframes;
        const long long cap = std::min<long long>(total, key.cap);
        const int stride = p.queue_entry_bytes;
        for (int q = 0; q < (p.park[1] > 0 ? 2 : 1); ++q) {
            if (int rc = step(q, p.single ? 2 : 1, stride, (size_t)cap * (size_t)stride, s)) return rc;
            a.queue[q] = (unsigned char*)buf[q].p;
        }
        a.queue_cap = (int32_t)cap;
        a.queue_stride = stride;
        return RM_OK;
    }
    // rm_debug_poison_queues: every word of the queues becomes `word`, written by nobody the next launch knows (writer 3)
    int poison(uint32_t word)
    {
        for (int q = 0; q < rm::kQueues; ++q) {
            if (!buf[q].p || buf[q].cap == 0) continue;
            HIP_TRY(hipMemsetD32((hipDeviceptr_t)buf[q].p, (int)word, buf[q].cap / 4));
            if (int rc = step(q, 3, key.of[q].stride, buf[q].cap, nullptr)) return rc;      // (clears nothing: not grown, not writer 2)
        }
        return RM_OK;
    }
} g_queues;

// Optional per-pass timing of the last frame (rm_set_pass_timing): events around the passes, and what rm_get_pass_ms
// decodes of a single launch's in-kernel marks.
struct PassTiming {
    Events<RM_MAX_PASSES + 1> ev;
    struct Key {
        bool on = false;
        int count = 0;
        bool last_was_pipeline = false;                  // rm_get_pass_ms decodes the in-kernel marks of `last_stats`
        const unsigned long long* last_stats = nullptr;
        float long_marks[4] = { 0.f, 0.f, 0.f, 0.f };    // longest rays: earliest / latest push, shortest / longest stay with a team
        float last_push_ms = 0.f, last_pop_ms = 0.f;     // queue-1 marks of the last single-launch frame decoded by rm_get_pass_ms
    };
    PerSession<Key> key;
    int start(hipStream_t s)
    {
        key.count = 0;
        key.last_was_pipeline = false;
        if (key.on) HIP_TRY(hipEventRecord(ev[0], s));
        return RM_OK;
    }
    int pass_done(hipStream_t s)
    {
        if (key.on) HIP_TRY(hipEventRecord(ev[++key.count], s));
        return RM_OK;
    }
} g_passes;

// The single launch (rm_pipeline.h): its control block, the generation tag of its queue entries, the development trace
// (rm_debug_set_trace) and, for the split form, the side stream.
struct SingleLaunch {
    WsBuf ctl;                                  // the hot counters, one per 128-byte line
    WsBuf trace, trace_start, trace_detach;
    struct Key { uint32_t generation = 0; bool tracing = false; size_t trace_pix = 0; };
    PerSession<Key> key;
    // The split form: the team kernel runs on a stream of the library's own, next to the producer kernel on the caller's.
    // Created by the first split frame; split_ev[0] = "the frame's set-up is enqueued" (the side stream waits for it),
    // split_ev[1] = "the team kernel has ended" (the caller's stream waits for it).
    SideStream team_stream;
    Events<2> split_ev{ hipEventDisableTiming };

    // control block, generation tag, marks and trace buffers of one launch
    int set_up(rm::KernelArgs& a, int ntiles, hipStream_t s)
    {
        int rc;
        if ((rc = ctl.ensure(sizeof(unsigned long long) * rm::kCtlWords))) return rc;
        HIP_TRY(hipMemsetAsync(ctl.p, 0, sizeof(unsigned long long) * rm::kCtlWords, s));
        a.ctl = (unsigned long long*)ctl.p;
        if (++key.generation == 0) key.generation = 1;
        a.generation = key.generation;
        a.marks = (g_passes.key.on || key.tracing) ? 1 : 0;      // device-clock marks only when somebody will read them (rm_get_pass_ms)
        if (key.tracing) {
            constexpr size_t kTraceRecords = 1u << 20;
            const size_t npix = (size_t)a.rows * a.width * a.nframes;
            if ((rc = trace.ensure((8 + 8 * kTraceRecords) * 4)) || (rc = trace_start.ensure(npix * 4)) || (rc = trace_detach.ensure(npix * 4)))
                return rc;
            HIP_TRY(hipMemsetAsync(trace.p, 0, 32, s));
            HIP_TRY(hipMemsetAsync(trace_start.p, 0, npix * 4, s));
            HIP_TRY(hipMemsetAsync(trace_detach.p, 0, npix * 4, s));
            a.trace = (uint32_t*)trace.p;
            a.trace_cap = (uint32_t)kTraceRecords;
            a.trace_start = (uint32_t*)trace_start.p;
            a.trace_detach = (uint32_t*)trace_detach.p;
            key.trace_pix = npix;
        }
        if (a.tile_cost) HIP_TRY(hipMemsetAsync(a.tile_cost, 0, (size_t)ntiles * 4, s));   // resumed rays may report before the tile flush
        return RM_OK;
    }
    // the launch in the plan's form: the fused kernel, or producers and teams as two
    int enqueue(const RmFrameDesc* d, const rm::LaunchPlan& p, const rm::KernelArgs& a, const rm::SceneLaunchers* sc, hipStream_t s)
    {
        if (p.form == 1) {
            HIP_TRY(sc->pipeline(d->strategy_id, a, p.pipeline_grid, s));
            return RM_OK;
        }
        // PRODUCERS FIRST: they never wait for a team, so whatever the device makes of the two kernels -- side by side, or
        // the teams only once the producers have left -- the frame is correct and ends.  A team that starts before any
        // producer polls (bounded) until the producer waves have reported their exit.
        hipStream_t ts = s;
        if (p.form == 2) {
            int rc;
            if ((rc = team_stream.ensure()) || (rc = split_ev.ensure())) return rc;
            ts = team_stream.s;
            HIP_TRY(hipEventRecord(split_ev[0], s));            // control block, queues and statistics are reset
            HIP_TRY(hipStreamWaitEvent(ts, split_ev[0], 0));
        }
        HIP_TRY(sc->pipeline_producers(d->strategy_id, a, p.pipeline_grid - p.team_wgs, s));
        HIP_TRY(sc->pipeline_teams(d->strategy_id, a, p.team_wgs, ts));
        if (p.form == 2) {
            // the caller's stream goes on when both kernels have ended: its events and the statistics fold cover the teams
            HIP_TRY(hipEventRecord(split_ev[1], ts));
            HIP_TRY(hipStreamWaitEvent(s, split_ev[1], 0));
        }
        return RM_OK;
    }
} g_single;

// The parked-ray queues, tile costs / orders, the control block and the pass events are ONE workspace: frames are
// serialised on the device.  The end of the latest frame is an event on its stream; a frame enqueued on another stream
// first waits for it (callers may still overlap their own copies and other kernels with a frame).
struct FrameSerial {
    Events<1> ev{ hipEventDisableTiming };
    struct Key { hipStream_t stream = nullptr; };
    PerSession<Key> key;
    int begin(hipStream_t s)
    {
        if (ev.made && key.stream != s) HIP_TRY(hipStreamWaitEvent(s, ev[0], 0));
        return RM_OK;
    }
    int end(hipStream_t s)
    {
        if (int rc = ev.ensure()) return rc;
        HIP_TRY(hipEventRecord(ev[0], s));
        key.stream = s;
        return RM_OK;
    }
} g_serial;

int launch_frame(const RmFrameDesc* d, const rm::LaunchPlan& p, rm::KernelArgs a, hipStream_t s);

// One frame, after the one before it.
int launch(const RmFrameDesc* d, const rm::LaunchPlan& p, const rm::KernelArgs& a, hipStream_t s)
{
    int rc;
    if ((rc = g_serial.begin(s)) || (rc = launch_frame(d, p, a, s))) return rc;
    return g_serial.end(s);
}

// Passes 2 and 3 of a frame with one launch per pass: the parked rays of queue 0, then those parked again in queue 1.
int resume_passes(const RmFrameDesc* d, const rm::LaunchPlan& p, const rm::KernelArgs& a, const rm::SceneLaunchers* sc, hipStream_t s)
{
    rm::KernelArgs b = a;
    b.suspend_after = p.park[1];
    b.suspend_queue = 1;
    b.refill_min = p.resume_refill_min;
    b.team_wgs = p.resume_grid;
    b.keep_busy = p.pass_keep_busy;
    for (int level = 0; level < (p.park[1] > 0 ? 2 : 1); ++level) {
        if (level == 1) {
            b.suspend_after = 0;
            b.interleave = 0;       // a sparse pass of very long rays is latency-bound: whole evaluations per turn
        }
        if (p.pass_team[level])
            HIP_TRY(sc->resume_team(d->strategy_id, level, b, p.team_pass_grid, s));
        else
            HIP_TRY(sc->resume(d->strategy_id, level, b, p.resume_grid, s));
        if (int rc = g_passes.pass_done(s)) return rc;
    }
    return RM_OK;
}

// Performs the plan `p` (rm_launch_plan.h) of one launch: the steps in the order it dictates.
int launch_frame(const RmFrameDesc* d, const rm::LaunchPlan& p, rm::KernelArgs a, hipStream_t s)
{
    a.raw_outputs = (a.t_raw || a.final_sdf || a.evals) ? 1 : 0;
    int rc;
    if ((rc = g_stats.reset(a, s))) return rc;                                           // 1. statistics
    if (d->rows == 0) return RM_OK;
    if (p.refuse) return fail(RM_E_BAD_ARG, "%s", p.refuse);                             // 2. a launch form that does not exist
    const rm::SceneLaunchers* const sc = launchers(d->scene_id);
    const int ntiles = a.tiles_per_frame * a.nframes;
    int order = p.tile_order;                                                            // 3. tile order
    if (order == 1) {
        if ((rc = g_dynamic_order.apply(d, p, ntiles, a, s))) return rc;
        if (!a.tile_order) order = p.static_order;    // no costs yet: the first frame takes the static order
    }
    if ((order == 2 || order == 4) && (rc = g_static_order.apply(d, p, order, ntiles, a, s))) return rc;
    long long* const block_var = a.block_var;
    if (p.park[0] > 0) {                                                                 // 4. the parked rays' queues
        if ((rc = g_queues.prepare(p, a, s))) return rc;
        a.block_var = nullptr;      // parked pixels are missing at flush time: reduced from the finished map below
    }
    if ((rc = g_passes.start(s))) return rc;                                             // 5. pass timing
    if (p.single) {                                                                      // 6. the whole frame in ONE launch (rm_pipeline.h) ...
        if ((rc = g_single.set_up(a, ntiles, s)) || (rc = g_single.enqueue(d, p, a, sc, s)) || (rc = g_passes.pass_done(s))) return rc;
        g_passes.key.last_was_pipeline = true;
        g_passes.key.last_stats = a.stats;
    } else {                                                                             //    ... or render and the resume passes
        if (rm::is_strategy_program(d->strategy_id)) HIP_TRY(strategy_launchers(d->scene_id)->render(a, p.render_grid, s));
        else HIP_TRY(sc->render(d->strategy_id, a, p.render_grid, s));
        if ((rc = g_passes.pass_done(s))) return rc;
        if (p.park[0] > 0 && (rc = resume_passes(d, p, a, sc, s))) return rc;
    }
    if (p.park[0] > 0 && block_var) {                                                    // 7. block variance of a frame that parked rays
        const long long nb = (long long)(a.width >> 3) * (a.rows >> 2) * a.nframes;
        if (nb > 0) {
            hipLaunchKernelGGL(block_var_kernel, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, s, a.iters, a.width,
                               a.rows, a.nframes, block_var);
            HIP_TRY(hipGetLastError());
        }
    }
    if (!a.fused_reduce) {                                                               // 8. statistics reduce
        hipLaunchKernelGGL(stats_reduce_kernel, dim3((rm::kStatsWords + 255) / 256), dim3(256), 0, s, a.stats);
        HIP_TRY(hipGetLastError());
    }
    return RM_OK;
}

// a single-launch frame whose queue protocol ran into one of its wait bounds (rm_pipeline.h) reports it here
int check_pipeline_error(const unsigned long long* w)
{
    if (w[rm::kWError] != 0)
        return fail(RM_E_HIP, "single-launch pipeline: a wait of the queue protocol hit its bound (code %llu); results are incomplete", w[rm::kWError]);
    return RM_OK;
}

void decode_stats(const unsigned long long* w, RmStats* out)
{
    out->hit_count = w[1];
    out->sum_iters = w[2];
    out->iter_max = (int32_t)w[3];
    out->total_rays = w[5];
    out->sum_evals = w[10];
    out->iter_min = w[5] ? (int32_t)(0x7fffffffull - w[4]) : 0;
    for (int b = 0; b < RM_HIST_BINS; ++b) out->iter_hist[b] = w[rm::kStatsHead + b];
}

// The events of timed() bracket one whole frame: stats reset, optional tile ordering, render kernel.
int timed_launches(const Entry& e, const RmFrameDesc* d, const rm::LaunchPlan& p, const rm::KernelArgs& a, RmTiming* t)
{
    return timed(e, t, lib_stream(), [&] { return launch(d, p, a, lib_stream()); });
}

// The canonical statistics block at `dev`, read once `s` has run dry: the pipeline's error word, then the counters.
int read_stats(const Entry&, const void* dev, hipStream_t s, RmStats* out)
{
    unsigned long long w[rm::kStatsWords];
    HIP_TRY(hipMemcpyAsync(w, dev, kStatsBlockBytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (int rc = check_pipeline_error(w)) return rc;
    if (out) decode_stats(w, out);
    return RM_OK;
}

// ---- store-path probe: the flush of render_kernel without the march --------------------
__global__ __launch_bounds__(64) void store_path_kernel(float* depth, int32_t* iters, uint8_t* hit, int width,
                                                        int rows, int tiles_x, int ntiles)
{
    constexpr int TILE_H = 4;
    __shared__ float s_depth[64 * TILE_H];
    __shared__ int32_t s_iters[64 * TILE_H];
    __shared__ uint8_t s_hit[64 * TILE_H];
    const int lane = threadIdx.x;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int x0 = (tile % tiles_x) * 64, y0 = (tile / tiles_x) * TILE_H;
        for (int r = 0; r < TILE_H; ++r) {
            s_depth[r * 64 + lane] = (float)(tile + r);
            s_iters[r * 64 + lane] = tile ^ lane;
            s_hit[r * 64 + lane] = (uint8_t)((tile + lane) & 1);
        }
        __syncthreads();
        const int gx = x0 + lane;
        for (int r = 0; r < TILE_H; ++r)
            if (gx < width && y0 + r < rows) {
                const size_t gi = (size_t)(y0 + r) * width + gx;
                depth[gi] = s_depth[r * 64 + lane];
                iters[gi] = s_iters[r * 64 + lane];
                hit[gi] = s_hit[r * 64 + lane];
            }
        __syncthreads();
    }
}

}  // namespace

void rm::capi::frame_stream_destroyed(hipStream_t s)
{
    if (g_serial.key.stream == s) g_serial.key.stream = nullptr;      // its last frame has completed: nothing runs there to wait for
}

int rm::capi::check_desc(const RmFrameDesc* d)
{
    if (!d) return fail(RM_E_BAD_ARG, "desc is NULL");
    if (int rc = check_scene(d->scene_id)) return rc;
    if (int rc = check_strategy(d->strategy_id)) return rc;
    if (rm::is_strategy_program(d->strategy_id) && !strategy_launchers(d->scene_id))
        return fail(RM_E_BAD_STRATEGY, "the strategy-program kernels of scene %d are not built into this (development) library", d->scene_id);
    if (int rc = check_slice(d, d->band_rows > 0 && d->band_stride > 1)) return rc;
    if (d->tile_rows != 0 && d->tile_rows != 4 && d->tile_rows != 1) return fail(RM_E_BAD_ARG, "tile_rows must be 0, 4 or 1");
    if (d->tile_order_mode < 0 || d->tile_order_mode > 4) return fail(RM_E_BAD_ARG, "tile_order_mode must be 0 .. 4");
    if (d->eval_mode < 0 || d->eval_mode > 2) return fail(RM_E_BAD_ARG, "eval_mode must be 0, 1 or 2");
    if (d->resume_mode < 0 || d->resume_mode > 3) return fail(RM_E_BAD_ARG, "resume_mode must be 0..3");
    if (d->resume_grid < 0) return fail(RM_E_BAD_ARG, "negative resume_grid");
    if (d->pipeline < 0 || d->pipeline > 2) return fail(RM_E_BAD_ARG, "pipeline must be 0, 1 or 2");
    if (d->pipeline_form < 0 || d->pipeline_form > 3) return fail(RM_E_BAD_ARG, "pipeline_form must be 0 .. 3");
    if (d->team_grid < 0 || d->queue_first < 0 || d->queue_first > 3 || d->team_steal < 0 || d->team_steal > 2 ||
        d->queue_refill_min < 0 || d->queue_refill_min > 64 || d->queue_retry < 0 || d->team_retry < 0 || d->age_priority < 0)
        return fail(RM_E_BAD_ARG, "bad single-launch tuning field");
    if (d->exit_backlog < 0 || d->late_teams > 65536) return fail(RM_E_BAD_ARG, "bad late-team field");
    if (d->keep_busy > (1 << 20)) return fail(RM_E_BAD_ARG, "keep_busy out of range");
    if (d->early_handover > (1 << 20)) return fail(RM_E_BAD_ARG, "early_handover out of range");
    if (d->early_trips < 0 || d->early_trips > 64) return fail(RM_E_BAD_ARG, "early_trips out of range");
    if (d->band_rows < 0 || d->band_stride < 0 || d->band_offset < 0) return fail(RM_E_BAD_ARG, "negative band parameter");
    if (d->band_rows > 0 && d->band_stride > 1) {
        const int th = d->tile_rows ? d->tile_rows : 4;
        if (d->band_rows % th) return fail(RM_E_BAD_ARG, "band_rows must be a multiple of the tile height %d", th);
        if (d->band_offset >= d->band_stride) return fail(RM_E_BAD_ARG, "band_offset must be < band_stride");
        if (d->rows > 0) {
            const long long y = d->rows - 1;
            const long long last = d->row0 + ((y / d->band_rows) * d->band_stride + d->band_offset) * d->band_rows + y % d->band_rows;
            if (last >= d->height) return fail(RM_E_BAD_DIMS, "band-cyclic slice maps row %lld beyond height %d", last, d->height);
        }
    }
    return RM_OK;
}

extern "C" {

size_t rm_stats_device_bytes(void) { return kStatsBytes; }

int rm_sdf_eval(int scene_id, const double* xyz, size_t n, double* out)
{
    Entry e;
    int rc = e.rc();
    if (rc || (rc = check_scene(scene_id))) return rc;
    if (n == 0) return RM_OK;
    if (!xyz || !out) return fail(RM_E_BAD_ARG, "NULL buffer");
    const void* data = nullptr;
    if ((rc = scene_data(scene_id, &data))) return rc;
    Staged st(e);
    const double* d_xyz = st.in(stage_in[0], xyz, n * 24);
    double* d_out = st.out(stage_out[0], out, n * 8);
    if ((rc = st.begin())) return rc;
    HIP_TRY(launchers(scene_id)->sdf_eval(d_xyz, n, d_out, data, lib_stream()));
    return st.finish();
}

static int march_rays_impl(bool team, int scene_id, int strategy_id, const RmMarchConfig* cfg, const double* origins,
                           const double* dirs, size_t n, uint8_t* hit, double* t, int32_t* iters, double* final_sdf)
{
    Entry e;
    int rc = e.rc();
    if (rc || (rc = check_scene(scene_id))) return rc;
    if ((rc = check_strategy(strategy_id))) return rc;
    const bool program = rm::is_strategy_program(strategy_id);
    if (program && team) return fail(RM_E_BAD_STRATEGY, "strategy program %d: a strategy program has no wavefront-team form", strategy_id);
    if (program && !strategy_launchers(scene_id))
        return fail(RM_E_BAD_STRATEGY, "the strategy-program kernels of scene %d are not built into this (development) library", scene_id);
    if (!cfg) return fail(RM_E_BAD_ARG, "cfg is NULL");
    if (team && !launchers(scene_id)->march_rays_team) return fail(RM_E_BAD_SCENE, "scene %d has no wavefront-team form", scene_id);
    if (n == 0) return RM_OK;
    if (!origins || !dirs || !hit || !t || !iters || !final_sdf) return fail(RM_E_BAD_ARG, "NULL buffer");
    const void* data = nullptr;
    if ((rc = scene_data(scene_id, &data))) return rc;
    const void* sdata = nullptr;
    if ((rc = strategy_data(strategy_id, &sdata))) return rc;
    Staged st(e);
    const double* d_origins = st.in(stage_in[0], origins, n * 24);
    const double* d_dirs = st.in(stage_in[1], dirs, n * 24);
    uint8_t* d_hit = st.out(stage_out[0], hit, n);
    double* d_t = st.out(stage_out[1], t, n * 8);
    int32_t* d_iters = st.out(stage_out[2], iters, n * 4);
    double* d_fs = st.out(stage_out[3], final_sdf, n * 8);
    if ((rc = st.begin())) return rc;
    rm::MarchCfg c = to_cfg(*cfg);
    c.full = 1;   // per-ray API always returns final_sdf, like MarchResult
    if (team) {
        // with filler workgroups (team_fillers): rm_march_rays_team is how bench.py measures a chain
        if ((rc = g.busy.ensure(128))) return rc;
        HIP_TRY(hipMemsetAsync(g.busy.p, 0, sizeof(unsigned long long), lib_stream()));
        const long long nteams = (long long)((n + 63) / 64);
        const int fillers = rm::team_fillers(device_prop().multiProcessorCount, nteams);
        HIP_TRY(launchers(scene_id)->march_rays_team(strategy_id, c, d_origins, d_dirs, n, d_hit, d_t, d_iters, d_fs,
                                                     (unsigned long long*)g.busy.p, fillers, lib_stream()));
    } else if (program) {
        HIP_TRY(strategy_launchers(scene_id)->march_rays(c, d_origins, d_dirs, n, d_hit, d_t, d_iters, d_fs, data, sdata, lib_stream()));
    } else {
        HIP_TRY(launchers(scene_id)->march_rays(strategy_id, c, d_origins, d_dirs, n, d_hit, d_t, d_iters, d_fs, data, lib_stream()));
    }
    return st.finish();
}

int rm_strategy_program_create(const RmStrategyOp* ops, int32_t nops, int32_t* strategy_id)
{
    if (!strategy_id) return fail(RM_E_BAD_ARG, "strategy_id is NULL");
    std::unique_ptr<rm::StrategyImage> img(new rm::StrategyImage());
    char why[256];
    if (!rm::strategy_encode(ops, nops, img.get(), why, sizeof why)) return fail(RM_E_BAD_ARG, "strategy program: %s", why);
    std::lock_guard<std::mutex> lk(g_sp_mu);
    if (g_next_strategy_program == INT32_MAX) return fail(RM_E_BAD_ARG, "strategy program ids exhausted");
    const int32_t id = g_next_strategy_program++;
    g_strategy_programs[id].img = std::move(img);
    *strategy_id = id;
    return RM_OK;
}

int rm_strategy_program_destroy(int32_t strategy_id)
{
    Lock lk;                                    // no call of this library is enqueueing a frame of the program meanwhile
    void* dev = nullptr;
    {
        std::lock_guard<std::mutex> lp(g_sp_mu);
        auto it = g_strategy_programs.find(strategy_id);
        if (it == g_strategy_programs.end()) return no_such_strategy_program(strategy_id);
        dev = it->second.dev;
        g_strategy_programs.erase(it);
    }
    if (dev && lk.select_device()) HIP_TRY(hipFree(dev));      // (hipFree waits for the device: no launch still reads the copy)
    return RM_OK;
}

int rm_march_rays(int scene_id, int strategy_id, const RmMarchConfig* cfg, const double* origins, const double* dirs,
                  size_t n, uint8_t* hit, double* t, int32_t* iters, double* final_sdf)
{
    return march_rays_impl(false, scene_id, strategy_id, cfg, origins, dirs, n, hit, t, iters, final_sdf);
}

int rm_march_rays_team(int scene_id, int strategy_id, const RmMarchConfig* cfg, const double* origins, const double* dirs,
                       size_t n, uint8_t* hit, double* t, int32_t* iters, double* final_sdf)
{
    return march_rays_impl(true, scene_id, strategy_id, cfg, origins, dirs, n, hit, t, iters, final_sdf);
}

int rm_render_outputs(const RmFrameDesc* d, const RmOutputs* o, RmStats* stats, RmTiming* timing)
{
    Entry e;
    int rc = e.rc();
    if (rc || (rc = check_desc(d))) return rc;
    if (!o || !o->depth || !o->iters || !o->hit) return fail(RM_E_BAD_ARG, "depth, iters and hit are required");
    if (o->final_sdf && !d->march.full) return fail(RM_E_BAD_ARG, "final_sdf requires march.full = 1");
    if (o->block_var && (d->row0 % 4) != 0) return fail(RM_E_BAD_ARG, "block_var requires row0 %% 4 == 0");
    const size_t n = (size_t)d->rows * (size_t)d->width;
    const size_t nblk = (size_t)(d->rows / 4) * (size_t)(d->width / 8);
    Staged st(e);
    float* d_depth = st.out(g.depth, o->depth, n * 4, 16);
    int32_t* d_iters = st.out(g.iters, o->iters, n * 4, 16);
    uint8_t* d_hit = st.out(g.hit, o->hit, n, 16);
    double* d_traw = st.out(g.traw, o->t_raw, n * 8, 16);
    double* d_fs = st.out(g.fs, o->final_sdf, n * 8, 16);
    long long* d_bvar = (long long*)st.out(g.bvar, o->block_var, nblk * 8, 16);
    int32_t* d_evals = st.out(g.evals, o->evals, n * 4, 16);
    if ((rc = st.begin())) return rc;
    const rm::LaunchPlan p = plan_for(d);
    rm::KernelArgs a;
    if ((rc = make_args(d, p, d_depth, d_iters, d_hit, d_traw, d_fs, d_bvar, nullptr, &a))) return rc;
    a.evals = d_evals;
    if ((rc = timing ? timed_launches(e, d, p, a, timing) : launch(d, p, a, lib_stream()))) return rc;
    if ((rc = st.download())) return rc;
    return read_stats(e, g_stats.buf.p, lib_stream(), stats);
}

int rm_render(const RmFrameDesc* d, float* depth, int32_t* iters, uint8_t* hit, double* t_raw, double* final_sdf,
              int64_t* block_var, RmStats* stats, RmTiming* timing)
{
    RmOutputs o;
    memset(&o, 0, sizeof o);
    o.depth = depth; o.iters = iters; o.hit = hit; o.t_raw = t_raw; o.final_sdf = final_sdf; o.block_var = block_var;
    return rm_render_outputs(d, &o, stats, timing);
}

int rm_render_device(const RmFrameDesc* d, void* d_depth, void* d_iters, void* d_hit, void* d_stats, void* stream)
{
    Entry e;                                  // the enqueue touches the shared workspace (queues, tile order, pass events)
    int rc = e.rc();
    if (rc || (rc = check_desc(d))) return rc;
    if (!d_depth || !d_iters || !d_hit) return fail(RM_E_BAD_ARG, "device output pointers are required");
    hipStream_t s;
    if ((rc = e.stream(stream, &s))) return rc;
    const rm::LaunchPlan p = plan_for(d);
    rm::KernelArgs a;
    if ((rc = make_args(d, p, (float*)d_depth, (int32_t*)d_iters, (uint8_t*)d_hit, nullptr, nullptr, nullptr,
                        (unsigned long long*)d_stats, &a)))
        return rc;
    return launch(d, p, a, s);
}

int rm_read_stats(const void* d_stats, void* stream, RmStats* out)
{
    Entry e;
    int rc = e.rc();
    if (rc) return rc;
    if (!out) return fail(RM_E_BAD_ARG, "out is NULL");
    hipStream_t s;
    if ((rc = e.stream(stream, &s))) return rc;
    unsigned long long* own = nullptr;
    if (!d_stats && (rc = g_stats.get(&own))) return rc;
    return read_stats(e, d_stats ? d_stats : own, s, out);
}

int rm_bench_device(const RmFrameDesc* d, void* d_depth, void* d_iters, void* d_hit, RmStats* stats, RmTiming* timing)
{
    Entry e;
    int rc = e.rc();
    if (rc || (rc = check_desc(d))) return rc;
    if (!d_depth || !d_iters || !d_hit || !timing) return fail(RM_E_BAD_ARG, "device outputs and timing are required");
    const rm::LaunchPlan p = plan_for(d);
    rm::KernelArgs a;
    if ((rc = make_args(d, p, (float*)d_depth, (int32_t*)d_iters, (uint8_t*)d_hit, nullptr, nullptr, nullptr,
                        nullptr, &a)))
        return rc;
    if ((rc = timed_launches(e, d, p, a, timing))) return rc;
    return stats ? read_stats(e, g_stats.buf.p, lib_stream(), stats) : RM_OK;
}

int rm_render_batch_outputs(const RmFrameDesc* shape, int32_t nframes, const double* cams, const RmMarchConfig* configs,
                            const RmOutputs* o, RmStats* stats, float* ms_total)
{
    if (!o) return fail(RM_E_BAD_ARG, "outputs record is NULL");
    if (o->t_raw || o->final_sdf || o->block_var) return fail(RM_E_BAD_ARG, "batches return depth, iters, hit and evals only");
    float* const depth = o->depth;
    int32_t* const iters = o->iters;
    uint8_t* const hit = o->hit;
    int32_t* const evals = o->evals;
    Entry e;
    int rc = e.rc();
    if (rc || (rc = check_desc(shape))) return rc;
    if (nframes < 0 || (nframes > 0 && (!cams || !depth || !iters || !hit))) return fail(RM_E_BAD_ARG, "bad batch arguments");
    if (shape->tile_order_mode != 0) return fail(RM_E_BAD_ARG, "tile_order_mode is not supported for batches");
    if (nframes == 0) return RM_OK;
    const int full = configs ? (configs[0].full ? 1 : 0) : (shape->march.full ? 1 : 0);
    for (int f = 0; configs && f < nframes; ++f)
        if ((configs[f].full ? 1 : 0) != full) return fail(RM_E_BAD_ARG, "all frames of a batch must share march.full");
    const size_t n = (size_t)shape->rows * (size_t)shape->width;          // elements per frame
    const size_t total = n * (size_t)nframes;
    if (total > (size_t)1 << 31) return fail(RM_E_BAD_DIMS, "batch too large");
    if ((rc = g.batch_ev.ensure())) return rc;
    // the frame table: one camera + march configuration per frame
    std::vector<rm::FrameParams> fp((size_t)nframes);
    for (int f = 0; f < nframes; ++f) {
        fp[f].cam = camera_of(cams + (size_t)f * 14);
        fp[f].cfg = to_cfg(configs ? configs[f] : shape->march);
    }
    Staged st(e);
    float* d_depth = st.out(g.depth, depth, total * 4, 16);
    int32_t* d_iters = st.out(g.iters, iters, total * 4, 16);
    uint8_t* d_hit = st.out(g.hit, hit, total, 16);
    int32_t* d_evals = st.out(g.evals, evals, total * 4, 16);
    const rm::FrameParams* d_frames = st.in(g.frames, fp.data(), sizeof(rm::FrameParams) * (size_t)nframes);
    if ((rc = st.begin())) return rc;
    const rm::LaunchPlan p = plan_for(shape, nframes, configs);
    RmFrameDesc d = *shape;
    if (p.march_frame >= 0) d.march = configs[p.march_frame];      // (KernelArgs.single: the configuration the plan looked at)
    rm::KernelArgs a;
    if ((rc = make_args(&d, p, d_depth, d_iters, d_hit, nullptr, nullptr, nullptr, nullptr, &a))) return rc;
    a.frames = d_frames;
    a.nframes = nframes;
    a.full = full;
    a.evals = d_evals;
    HIP_TRY(hipEventRecord(g.batch_ev[0], lib_stream()));
    if ((rc = launch(&d, p, a, lib_stream()))) return rc;
    HIP_TRY(hipEventRecord(g.batch_ev[1], lib_stream()));
    if ((rc = st.download())) return rc;
    unsigned long long whead[rm::kStatsHead];
    HIP_TRY(hipMemcpyAsync(whead, g_stats.buf.p, sizeof whead, hipMemcpyDeviceToHost, lib_stream()));
    HIP_TRY(hipStreamSynchronize(lib_stream()));
    if (g_passes.key.last_was_pipeline && (rc = check_pipeline_error(whead))) return rc;      // a wait bound hit: the maps are incomplete
    if (ms_total) HIP_TRY(hipEventElapsedTime(ms_total, g.batch_ev[0], g.batch_ev[1]));
    if (stats) {
        // per-frame integer reduce of the returned maps (the in-kernel block aggregates the whole batch)
        for (int f = 0; f < nframes; ++f) {
            RmStats& st = stats[f];
            memset(&st, 0, sizeof st);
            st.total_rays = n;
            st.iter_min = n ? 0x7fffffff : 0;
            const int32_t* it = iters + (size_t)f * n;
            const uint8_t* h = hit + (size_t)f * n;
            for (size_t i = 0; i < n; ++i) {
                st.hit_count += h[i];
                st.sum_iters += (uint64_t)it[i];
                st.iter_max = std::max(st.iter_max, it[i]);
                st.iter_min = std::min(st.iter_min, it[i]);
                st.iter_hist[std::min<int32_t>(std::max<int32_t>(it[i], 0), RM_HIST_BINS - 1)] += 1;
            }
            if (evals)
                for (size_t i = 0; i < n; ++i) st.sum_evals += (uint64_t)evals[(size_t)f * n + i];
        }
    }
    return RM_OK;
}

int rm_set_queue_capacity(int64_t entries)
{
    if (entries < 0) return fail(RM_E_BAD_ARG, "negative queue capacity");
    Lock lk;
    g_queues.key.cap = entries == 0 ? kQueueCapMax : std::min<long long>(entries, 1ll << 30);
    return RM_OK;
}

int rm_set_pass_timing(int enable)
{
    Entry e;
    if (e.rc()) return e.rc();
    if (enable)
        if (int rc = g_passes.ev.ensure()) return rc;
    g_passes.key.on = enable != 0;
    g_passes.key.count = 0;
    return RM_OK;
}

int rm_get_pass_ms(void* stream, int32_t* npasses, float* ms)
{
    Entry e;
    int rc = e.rc();
    if (rc) return rc;
    if (!npasses || !ms) return fail(RM_E_BAD_ARG, "NULL output");
    if (!g_passes.key.on) return fail(RM_E_BAD_ARG, "pass timing is off (rm_set_pass_timing)");
    hipStream_t s;
    if ((rc = e.stream(stream, &s))) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    *npasses = g_passes.key.count;
    for (int i = 0; i < g_passes.key.count; ++i) HIP_TRY(hipEventElapsedTime(&ms[i], g_passes.ev[i], g_passes.ev[i + 1]));
    if (g_passes.key.last_was_pipeline && g_passes.key.count == 1 && g_passes.key.last_stats) {
        // one kernel: split its time at the marks its waves left in the stats block (100 MHz device clock)
        unsigned long long w[rm::kStatsHead];
        HIP_TRY(hipMemcpyAsync(w, g_passes.key.last_stats, sizeof w, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        const unsigned long long start = ~w[rm::kWMarkStart], tiles = ~w[rm::kWMarkTiles];
        if (w[rm::kWMarkStart] != 0 && w[rm::kWMarkTiles] != 0 && tiles >= start && w[rm::kWMarkFresh] >= tiles &&
            w[rm::kWMarkProd] >= w[rm::kWMarkFresh]) {
            const float total = ms[0];
            const float t_tiles = (float)((double)(tiles - start) * 1e-5);
            const float fresh = (float)((double)(w[rm::kWMarkFresh] - start) * 1e-5);
            const float prod = (float)((double)(w[rm::kWMarkProd] - start) * 1e-5);
            ms[0] = t_tiles; ms[1] = fresh - t_tiles; ms[2] = prod - fresh; ms[3] = std::max(0.f, total - prod);
            *npasses = 4;
            // times of the last push into / pop out of queue 1 since launch, for tools (rm_last_queue_marks)
            g_passes.key.last_push_ms = w[rm::kWMarkPush] >= start ? (float)((double)(w[rm::kWMarkPush] - start) * 1e-5) : 0.f;
            g_passes.key.last_pop_ms = w[rm::kWMarkPop] >= start ? (float)((double)(w[rm::kWMarkPop] - start) * 1e-5) : 0.f;
            g_passes.key.long_marks[0] = w[rm::kWLongPushMin] ? (float)((double)(~w[rm::kWLongPushMin]) * 1e-5) : 0.f;
            g_passes.key.long_marks[1] = (float)((double)w[rm::kWLongPushMax] * 1e-5);
            g_passes.key.long_marks[2] = w[rm::kWLongTeamMin] ? (float)((double)(~w[rm::kWLongTeamMin]) * 1e-5) : 0.f;
            g_passes.key.long_marks[3] = (float)((double)w[rm::kWLongTeamMax] * 1e-5);
        }
    }
    return RM_OK;
}

int rm_last_queue_marks(float* last_push_ms, float* last_pop_ms)
{
    if (!last_push_ms || !last_pop_ms) return fail(RM_E_BAD_ARG, "NULL output");
    Lock lk;
    *last_push_ms = g_passes.key.last_push_ms;
    *last_pop_ms = g_passes.key.last_pop_ms;
    return RM_OK;
}

int rm_long_ray_marks(float ms[4])
{
    if (!ms) return fail(RM_E_BAD_ARG, "NULL output");
    Lock lk;
    for (int i = 0; i < 4; ++i) ms[i] = g_passes.key.long_marks[i];
    return RM_OK;
}

int rm_render_batch(const RmFrameDesc* shape, int32_t nframes, const double* cams, const RmMarchConfig* configs,
                    float* depth, int32_t* iters, uint8_t* hit, RmStats* stats, float* ms_total)
{
    RmOutputs o;
    memset(&o, 0, sizeof o);
    o.depth = depth; o.iters = iters; o.hit = hit;
    return rm_render_batch_outputs(shape, nframes, cams, configs, &o, stats, ms_total);
}

int rm_debug_poison_queues(uint32_t word_offset, uint32_t* next_generation)
{
    Entry e;
    if (e.rc()) return e.rc();
    HIP_TRY(hipStreamSynchronize(lib_stream()));
    uint32_t next = g_single.key.generation + 1u;
    if (next == 0) next = 1;
    if (int rc = g_queues.poison(next + word_offset)) return rc;
    HIP_TRY(hipDeviceSynchronize());
    if (next_generation) *next_generation = next;
    return RM_OK;
}

int rm_debug_set_trace(int enable)
{
    Entry e;
    if (e.rc()) return e.rc();
    g_single.key.tracing = enable != 0;
    return RM_OK;
}

int rm_debug_get_trace(uint32_t* records, int64_t max_records, int64_t* nrecords, uint32_t* start_ticks, uint32_t* detach_ticks,
                       int64_t npix, uint32_t* launch_tick)
{
    Entry e;
    if (e.rc()) return e.rc();
    if (!nrecords) return fail(RM_E_BAD_ARG, "nrecords is NULL");
    HIP_TRY(hipDeviceSynchronize());
    if (!g_single.trace.p || !g_passes.key.last_stats) return fail(RM_E_BAD_ARG, "no traced single-launch frame (rm_debug_set_trace, then render)");
    uint32_t head[8];
    HIP_TRY(hipMemcpy(head, g_single.trace.p, sizeof head, hipMemcpyDeviceToHost));
    const int64_t n = std::min<int64_t>(head[0], 1 << 20);
    *nrecords = n;
    if (records && max_records > 0)
        HIP_TRY(hipMemcpy(records, (const uint32_t*)g_single.trace.p + 8, (size_t)std::min<int64_t>(n, max_records) * 32, hipMemcpyDeviceToHost));
    const size_t np = std::min<size_t>((size_t)std::max<int64_t>(npix, 0), g_single.key.trace_pix);
    if (start_ticks && np) HIP_TRY(hipMemcpy(start_ticks, g_single.trace_start.p, np * 4, hipMemcpyDeviceToHost));
    if (detach_ticks && np) HIP_TRY(hipMemcpy(detach_ticks, g_single.trace_detach.p, np * 4, hipMemcpyDeviceToHost));
    if (launch_tick) {
        unsigned long long w[rm::kStatsHead];
        HIP_TRY(hipMemcpy(w, g_passes.key.last_stats, sizeof w, hipMemcpyDeviceToHost));
        *launch_tick = (uint32_t)(~w[rm::kWMarkStart]);
    }
    return RM_OK;
}

int rm_bench_store_path(int32_t width, int32_t rows, void* d_depth, void* d_iters, void* d_hit, RmTiming* t)
{
    Entry e;
    if (e.rc()) return e.rc();
    if (width <= 0 || rows <= 0 || !d_depth || !d_iters || !d_hit || !t) return fail(RM_E_BAD_ARG, "bad arguments");
    const int tiles_x = (width + 63) / 64, tiles_y = (rows + 3) / 4;
    const int ntiles = tiles_x * tiles_y;
    const int grid = std::min(ntiles, device_prop().multiProcessorCount * 32);
    return timed(e, t, lib_stream(), [&] {
        hipLaunchKernelGGL(store_path_kernel, dim3(grid), dim3(64), 0, lib_stream(), (float*)d_depth, (int32_t*)d_iters,
                           (uint8_t*)d_hit, width, rows, tiles_x, ntiles);
        HIP_TRY(hipGetLastError());
        return (int)RM_OK;
    });
}

// ---- capture on the device: hit normals and shading (rm_capture.h, capture_kernel) ------------------------------------

int rm_capture(const RmFrameDesc* d, const RmCaptureOutputs* o, RmStats* stats, RmTiming* timing)
{
    if (!d || !o) return fail(RM_E_BAD_ARG, "desc or out is NULL");
    if (!o->hit) return fail(RM_E_BAD_ARG, "hit is required");
    if (!d->march.full) return fail(RM_E_BAD_ARG, "rm_capture requires march.full = 1 (final_sdf is part of geom)");
    if (d->band_rows > 0 && d->band_stride > 1) return fail(RM_E_BAD_ARG, "rm_capture takes no band-cyclic slice");
    int rc = check_desc(d);
    if (rc || (timing && (rc = check_timing(timing)))) return rc;
    Entry e;
    if ((rc = e.rc())) return rc;

    const size_t n = (size_t)d->rows * (size_t)d->width;
    // the march's outputs stay in the workspace; only the float maps the caller asked for (and hit) are staged back
    Staged st(e);
    float* d_depth = st.scratch<float>(g.depth, n * 4, 16);
    int32_t* d_iters = st.scratch<int32_t>(g.iters, n * 4, 16);
    double* d_traw = st.scratch<double>(g.traw, n * 8, 16);
    double* d_fs = st.scratch<double>(g.fs, n * 8, 16);
    int32_t* d_evals = st.scratch<int32_t>(g.evals, n * 4, 16);
    uint8_t* d_hit = st.out(g.hit, o->hit, n, 16);
    rm::CaptureArgs c;
    memset(&c, 0, sizeof c);
    c.geom = st.out(g.cap_out[0], o->geom, n * 16);
    c.normal = st.out(g.cap_out[1], o->normal, n * 12);
    c.depth = st.out(g.cap_out[2], o->depth, n * 4);
    c.color = st.out(g.cap_out[3], o->color, n * 12);
    c.evals_f = st.out(g.cap_out[4], o->evals, n * 4);
    if ((rc = st.begin())) return rc;
    const rm::LaunchPlan p = plan_for(d);
    rm::KernelArgs a;
    if ((rc = make_args(d, p, d_depth, d_iters, d_hit, d_traw, d_fs, nullptr, nullptr, &a))) return rc;
    a.evals = d_evals;
    c.cam = a.single.cam;
    c.width = d->width; c.height = d->height; c.row0 = d->row0; c.rows = d->rows;
    c.max_iterations = d->march.max_iterations; c.max_distance = d->march.max_distance;
    c.hit = d_hit; c.t = a.t_raw; c.iters = a.iters; c.final_sdf = a.final_sdf; c.evals = a.evals;
    c.scene_data = a.scene_data;
    const rm::SceneLaunchers* const sc = launchers(d->scene_id);
    rc = once_or_timed(e, timing, lib_stream(), [&] {
        if (int rc1 = launch(d, p, a, lib_stream())) return rc1;
        HIP_TRY(sc->capture(c, 1, lib_stream()));
        return (int)RM_OK;
    });
    if (rc || (rc = st.download())) return rc;
    return read_stats(e, g_stats.buf.p, lib_stream(), stats);
}

int rm_shade_frames(int scene_id, int32_t width, int32_t height, int32_t nframes, const double* cams, const double* t,
                    const float* depth, const uint8_t* hit, float* normal, float* color, RmTiming* timing)
{
    if (!cams || !hit || !normal || !color) return fail(RM_E_BAD_ARG, "cams, hit, normal or color is NULL");
    if (!t == !depth) return fail(RM_E_BAD_ARG, "exactly one of t and depth must be given");
    if (nframes < 1 || nframes > 65535) return fail(RM_E_BAD_ARG, "nframes %d outside [1, 65535]", nframes);
    if (width <= 0 || height <= 0) return fail(RM_E_BAD_DIMS, "bad frame shape %dx%d", width, height);
    if ((long long)width * height * nframes > (1ll << 31) - 1) return fail(RM_E_BAD_DIMS, "frames too large");
    int rc = check_scene(scene_id);
    if (rc || (timing && (rc = check_timing(timing)))) return rc;
    const size_t npix = (size_t)width * (size_t)height, n = npix * (size_t)nframes;
    for (size_t i = 0; i < n; ++i) {      // the libm restatements are unclaimed for NaN arguments
        if (!hit[i]) continue;
        const double v = t ? t[i] : (double)depth[i];
        if (!(v - v == 0.0))
            return fail(RM_E_BAD_ARG, "frame %zu, pixel %zu: the depth of a hit is not finite", i / npix, i % npix);
    }
    for (size_t i = 0; i < (size_t)nframes * 14; ++i)
        if (!(cams[i] - cams[i] == 0.0)) return fail(RM_E_BAD_ARG, "camera %zu: field %zu is not finite", i / 14, i % 14);
    Entry e;
    if ((rc = e.rc())) return rc;

    const void* data = nullptr;
    if ((rc = scene_data(scene_id, &data))) return rc;
    Staged st(e);
    rm::CaptureArgs c;
    memset(&c, 0, sizeof c);
    static_assert(sizeof(rm::CameraParams) == 14 * sizeof(double), "cams is an array of CameraParams");
    c.cams = (const rm::CameraParams*)st.in(g.cap_cams, cams, (size_t)nframes * sizeof(rm::CameraParams));
    if (t) c.t = st.in(stage_in[0], t, n * 8);
    else c.depth_in = st.in(stage_in[0], depth, n * 4);
    c.hit = st.in(stage_in[1], hit, n);
    c.normal = st.out(g.cap_out[1], normal, n * 12);
    c.color = st.out(g.cap_out[3], color, n * 12);
    if ((rc = st.begin())) return rc;
    c.width = width; c.height = height; c.row0 = 0; c.rows = height;
    c.max_iterations = 1; c.max_distance = 1.0;
    c.scene_data = data;
    const rm::SceneLaunchers* const sc = launchers(scene_id);
    rc = once_or_timed(e, timing, lib_stream(), [&] {
        HIP_TRY(sc->capture(c, nframes, lib_stream()));
        return (int)RM_OK;
    });
    if (rc) return rc;
    return st.finish();
}

}  // extern "C"
