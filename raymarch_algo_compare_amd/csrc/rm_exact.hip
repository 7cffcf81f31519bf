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
#include "rm_capi_internal.h"

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

}  // namespace rm

// ---- rm_exact_* of the C ABI: the interval oracle's scenes that pass exact_supported --------------------------------------
// (every launch below: the arguments are validated, `prog` is the device copy of the scene's ProgramImage, n > 0)
using namespace rm::capi;

namespace {

// RM_OK when the scene has an exact form; RM_E_BAD_SCENE with the reason otherwise.  Host only.
int exact_check_scene(int id)
{
    char why[160];
    if (is_program_id(id)) {
        bool ok = false;
        if (!with_program_image(id, [&](const rm::ProgramImage& img) { ok = rm::exact_supported(img, why, sizeof why); }))
            return no_such_program(id);
        if (!ok) return fail(RM_E_BAD_SCENE, "scene %d has no exact form: %s", id, why);
        return RM_OK;
    }
    const rm::ProgramImage* img = interval_catalogue_image(id);
    if (!img) return fail(RM_E_BAD_SCENE, "scene %d has no exact form: it is no composition of primitives", id);
    if (!rm::exact_supported(*img, why, sizeof why)) return fail(RM_E_BAD_SCENE, "scene %d has no exact form: %s", id, why);
    return RM_OK;
}

int exact_params(int id, const RmExactConfig* cfg, rm::ExactParams* P)
{
    int rc = exact_check_scene(id);
    if (rc) return rc;
    char why[160];
    if (!rm::exact_resolve(cfg, P, why, sizeof why)) return fail(RM_E_BAD_ARG, "RmExactConfig: %s", why);
    return RM_OK;
}

}  // namespace

extern "C" {

int rm_exact_supported(int scene_id) { return exact_check_scene(scene_id) == RM_OK ? 1 : 0; }

int rm_exact_march_rays(int scene_id, const RmExactConfig* cfg, const double* origins, const double* dirs, size_t n, double* t,
                        double* normals, int32_t* leaf)
{
    rm::ExactParams P;
    SoundCall c;
    int rc = c.open(scene_id, [&] { return exact_params(scene_id, cfg, &P); }, nullptr, nullptr, n, origins && dirs && t, "NULL buffer");
    if (rc || !c.prog) return rc;
    Staged st(*c.e);
    const double* d_origins = st.in(stage_in[0], origins, n * 24);
    const double* d_dirs = st.in(stage_in[1], dirs, n * 24);
    double* d_t = st.out(stage_out[0], t, n * 8);
    double* d_normals = st.out(stage_out[1], normals, n * 24);
    int32_t* d_leaf = st.out(stage_out[2], leaf, n * 4);
    if ((rc = st.begin())) return rc;
    hipLaunchKernelGGL(rm::exact_march_kernel, dim3(rm::grid_of(n)), dim3(rm::kExactBlock), 0, lib_stream(), c.prog, P, d_origins, d_dirs,
                       n, d_t, d_normals, d_leaf);
    HIP_TRY(hipGetLastError());
    return st.finish();
}

int rm_exact_render(const RmFrameDesc* d, const RmExactConfig* cfg, double* depth, uint8_t* hit, double* normal, int32_t* leaf,
                    RmTiming* timing)
{
    if (!d) return fail(RM_E_BAD_ARG, "desc is NULL");
    rm::ExactParams P;
    const size_t n = (size_t)d->width * (size_t)d->rows;
    SoundCall c;
    int rc = c.open(d->scene_id, [&] { return exact_params(d->scene_id, cfg, &P); }, d, timing, n, depth && hit,
                    "depth and hit are required");
    if (rc || !c.prog) return rc;
    Staged st(*c.e);
    double* d_depth = st.out(stage_out[0], depth, n * 8);
    uint8_t* d_hit = st.out(stage_out[1], hit, n);
    double* d_normal = st.out(stage_out[2], normal, n * 24);
    int32_t* d_leaf = st.out(stage_out[3], leaf, n * 4);
    if ((rc = st.begin())) return rc;
    const rm::CameraParams cam = camera_of(d->cam);
    rc = once_or_timed(*c.e, timing, lib_stream(), [&] {
        hipLaunchKernelGGL(rm::exact_render_kernel, dim3(rm::grid_of(n)), dim3(rm::kExactBlock), 0, lib_stream(), c.prog, P, cam, d->width,
                           d->height, d->row0, n, d_depth, d_hit, d_normal, d_leaf);
        HIP_TRY(hipGetLastError());
        return (int)RM_OK;
    });
    return rc ? rc : st.finish();
}

}  // extern "C"
