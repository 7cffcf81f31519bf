// rm_interval.hip -- the interval first-hit oracle on the device (rm_interval.h; rm_interval_* in include/rm_hip.h).
//
// One ray (or one point box) per lane, 256-thread workgroups.  The prologue copies the scene program into LDS and the
// pow tables (pow_half, rm_pow of the extensions and of the camera's normalisation) into their mirrors; every
// instruction word is then read at a wave-uniform address and moved to a scalar register (SceneProgram, ProgSrc), so
// the opcode dispatch is a chain of scalar branches.  The march loop itself is per lane: the lanes of a wave leave it
// after different numbers of steps.
#include <memory>

#include "rm_kernels.h"
#include "rm_interval.h"
#include "rm_interval_catalogue.h"
#include "rm_capi_internal.h"

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

// ---- the host side: what the five sound tracers share (rm_capi_internal.h), then rm_interval_* of the C ABI ----------------

namespace capi {

static WsBuf ivprog;   // the device image of a catalogue scene's program

// The encoded programs of the restated catalogue scenes (program_encode of rm_interval_catalogue.h, made once).
const ProgramImage* interval_catalogue_image(int id)
{
    static std::once_flag once;
    static std::unique_ptr<rm::ProgramImage> imgs[RM_NUM_SCENES];
    std::call_once(once, [] {
        for (int i = 0; i < RM_NUM_SCENES; ++i) {
            int32_t n = 0;
            const RmSceneOp* ops = rm::interval_catalogue_ops(i, &n);
            if (!ops) continue;
            std::unique_ptr<rm::ProgramImage> img(new rm::ProgramImage);
            char why[160];
            if (rm::program_encode(ops, n, img.get(), why, sizeof why)) imgs[i] = std::move(img);
        }
    });
    return id >= 0 && id < RM_NUM_SCENES ? imgs[id].get() : nullptr;
}

int interval_check_scene(int id)
{
    if (is_program_id(id)) return program_exists(id) ? RM_OK : no_such_program(id);
    if (!interval_catalogue_image(id)) return fail(RM_E_BAD_SCENE, "scene %d has no interval extension", id);
    return RM_OK;
}

int interval_params(int id, const RmIntervalConfig* cfg, rm::IntervalParams* P)
{
    char why[160];
    if (!rm::interval_resolve(cfg, rm::interval_scene_bound(id), P, why, sizeof why))
        return fail(RM_E_BAD_ARG, "RmIntervalConfig: %s", why);
    return RM_OK;
}

// the device image of scene `id` (under the library's lock with the device selected): a program's own copy, or the
// catalogue scene's image copied into the library's buffer on the stream
int interval_program(const Entry&, int id, const void** prog)
{
    if (is_program_id(id)) return scene_data(id, prog);
    const rm::ProgramImage* img = interval_catalogue_image(id);
    int rc = ivprog.ensure(sizeof(rm::ProgramImage));
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(ivprog.p, img, sizeof(rm::ProgramImage), hipMemcpyHostToDevice, lib_stream()));
    *prog = ivprog.p;
    return RM_OK;
}

}  // namespace capi
}  // namespace rm

using namespace rm::capi;

// (every launch below: the arguments are validated, `prog` is the device copy of the scene's ProgramImage, n > 0)
extern "C" {

int rm_interval_supported(int scene_id)
{
    if (is_program_id(scene_id)) return program_exists(scene_id) ? 1 : 0;
    return interval_catalogue_image(scene_id) ? 1 : 0;
}

int rm_interval_sdf_eval(int scene_id, const double* lo, const double* hi, size_t n, double* out_lo, double* out_hi)
{
    SoundCall c;
    int rc = c.open(scene_id, no_config, nullptr, nullptr, n, lo && hi && out_lo && out_hi, "NULL buffer");
    if (rc || !c.prog) return rc;
    Staged st(*c.e);
    const double* d_lo = st.in(stage_in[0], lo, n * 24);
    const double* d_hi = st.in(stage_in[1], hi, n * 24);
    double* d_out_lo = st.out(stage_out[0], out_lo, n * 8);
    double* d_out_hi = st.out(stage_out[1], out_hi, n * 8);
    if ((rc = st.begin())) return rc;
    hipLaunchKernelGGL(rm::interval_sdf_kernel, dim3(rm::grid_of(n)), dim3(rm::kIntervalBlock), 0, lib_stream(), c.prog, d_lo, d_hi, n,
                       d_out_lo, d_out_hi);
    HIP_TRY(hipGetLastError());
    return st.finish();
}

int rm_interval_march_rays(int scene_id, const RmIntervalConfig* cfg, const double* origins, const double* dirs, size_t n,
                           double* t, int32_t* steps, double* normals)
{
    rm::IntervalParams P;
    SoundCall c;
    int rc = c.open(scene_id, [&] { return interval_params(scene_id, cfg, &P); }, nullptr, nullptr, n, origins && dirs && t, "NULL buffer");
    if (rc || !c.prog) return rc;
    Staged st(*c.e);
    const double* d_origins = st.in(stage_in[0], origins, n * 24);
    const double* d_dirs = st.in(stage_in[1], dirs, n * 24);
    double* d_t = st.out(stage_out[0], t, n * 8);
    int32_t* d_steps = st.out(stage_out[1], steps, n * 4);
    double* d_normals = st.out(stage_out[2], normals, n * 24);
    if ((rc = st.begin())) return rc;
    hipLaunchKernelGGL(rm::interval_march_kernel, dim3(rm::grid_of(n)), dim3(rm::kIntervalBlock), 0, lib_stream(), c.prog, P, d_origins,
                       d_dirs, n, d_t, d_steps, d_normals);
    HIP_TRY(hipGetLastError());
    return st.finish();
}

int rm_interval_render(const RmFrameDesc* d, const RmIntervalConfig* cfg, double* depth, uint8_t* hit, double* normal,
                       int32_t* steps, RmTiming* timing)
{
    if (!d) return fail(RM_E_BAD_ARG, "desc is NULL");
    rm::IntervalParams P;
    const size_t n = (size_t)d->width * (size_t)d->rows;
    SoundCall c;
    int rc = c.open(d->scene_id, [&] { return interval_params(d->scene_id, cfg, &P); }, d, timing, n, depth && hit,
                    "depth and hit are required");
    if (rc || !c.prog) return rc;
    Staged st(*c.e);
    double* d_depth = st.out(stage_out[0], depth, n * 8);
    uint8_t* d_hit = st.out(stage_out[1], hit, n);
    double* d_normal = st.out(stage_out[2], normal, n * 24);
    int32_t* d_steps = st.out(stage_out[3], steps, n * 4);
    if ((rc = st.begin())) return rc;
    const rm::CameraParams cam = camera_of(d->cam);
    // (a timed call waits twice: the timing before it reads its events, finish() for the maps)
    rc = once_or_timed(*c.e, timing, lib_stream(), [&] {
        hipLaunchKernelGGL(rm::interval_render_kernel, dim3(rm::grid_of(n)), dim3(rm::kIntervalBlock), 0, lib_stream(), c.prog, P, cam,
                           d->width, d->height, d->row0, n, d_depth, d_hit, d_normal, d_steps);
        HIP_TRY(hipGetLastError());
        return (int)RM_OK;
    });
    return rc ? rc : st.finish();
}

}  // extern "C"
