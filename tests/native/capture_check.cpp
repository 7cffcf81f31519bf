// Host-only check build of csrc/rm_capture.h (one pixel of a capture: hit normal, shading, the float maps) over the
// catalogue scenes and the scene-program interpreter -- compiled by g++ for tests ONLY, so the exact source the gfx950
// capture kernel is built from can be checked against a per-pixel restatement and against the device in a container
// without a GPU.  Never loaded by the product.
#include <stddef.h>
#include <stdint.h>
#include "../../raymarch_algo_compare_amd/csrc/rm_capture.h"
#include "../../raymarch_algo_compare_amd/csrc/rm_scene_program.h"
#include "../../raymarch_algo_compare_amd/csrc/rm_strategies.h"

using namespace rm;

namespace {

thread_local long long g_calls = 0;      // Scene::sdf calls of the running rmc_capture*
thread_local ProgramImage g_img;

// the scene with its evaluations counted
template <class Scene>
struct Counted {
    static inline double sdf(vec3 p)
    {
        ++g_calls;
        return Scene::sdf(p);
    }
};

struct Frame {
    const double* cam14;
    int W, H, row0, rows, max_iterations;
    double max_distance;
    const uint8_t* hit;
    const double* t;
    const int32_t* iters;
    const double* fs;
    const int32_t* evals;
    float *geom, *normal, *depth, *color, *evals_f;
};

// what capture_kernel does with one lane per pixel (rm_kernels.h)
template <class Scene>
int capture_frame(const Frame& f, long long* calls)
{
    CameraParams cam;
    for (int i = 0; i < 14; ++i) cam.v[i] = f.cam14[i];
    g_calls = 0;
    for (int r = 0; r < f.rows; ++r)
        for (int px = 0; px < f.W; ++px) {
            const size_t i = (size_t)r * f.W + px;
            const bool hit = f.hit[i] != 0;
            capture_shade<Counted<Scene>>(cam, f.W, f.H, px, f.row0 + r, hit, f.t[i], f.normal + 3 * i, f.color + 3 * i);
            capture_geom(hit, f.t[i], f.iters[i], f.fs[i], f.evals[i], f.max_iterations, f.max_distance, f.geom + 4 * i,
                         f.depth + i, f.evals_f + i);
        }
    if (calls) *calls = g_calls;
    return 0;
}

template <class Scene, class Strat>
void march_frame(const MarchCfg& cfg, const double* cam14, int W, int H, uint8_t* hit, double* t, int32_t* iters, double* fs)
{
    CameraParams cam;
    for (int i = 0; i < 14; ++i) cam.v[i] = cam14[i];
    for (int py = 0; py < H; ++py)
        for (int px = 0; px < W; ++px) {
            vec3 o, d;
            camera_ray(cam, W, H, px, py, o, d);
            const Result res = march_one<Scene, Strat>(o, d, cfg);
            const size_t k = (size_t)py * W + px;
            hit[k] = (uint8_t)res.hit; t[k] = res.t; iters[k] = res.iters; fs[k] = res.final_sdf;
        }
}

}  // namespace

extern "C" {

double rmc_light(int c) { return c == 0 ? kCaptureLightX : c == 1 ? kCaptureLightY : kCaptureLightZ; }

// the six maps of rows [row0, row0 + rows) of a catalogue scene's frame (hit is the input map); -1: unknown scene
int rmc_capture(int scene, const double* cam14, int W, int H, int row0, int rows, int max_iterations, double max_distance,
                const uint8_t* hit, const double* t, const int32_t* iters, const double* fs, const int32_t* evals, float* geom,
                float* normal, float* depth, float* color, float* evals_f, long long* calls)
{
    const Frame f = { cam14, W, H, row0, rows, max_iterations, max_distance, hit, t, iters, fs, evals, geom, normal, depth, color, evals_f };
    switch (scene) {
#define RM_X(id, S) case id: return capture_frame<S>(f, calls);
        RM_SCENE_LIST(RM_X)
#undef RM_X
    }
    return -1;
}

// ... of a scene program's frame; -1: the program does not encode
int rmc_capture_program(const RmSceneOp* ops, int32_t nops, const double* cam14, int W, int H, int row0, int rows,
                        int max_iterations, double max_distance, const uint8_t* hit, const double* t, const int32_t* iters,
                        const double* fs, const int32_t* evals, float* geom, float* normal, float* depth, float* color,
                        float* evals_f, long long* calls)
{
    char why[256];
    if (!program_encode(ops, nops, &g_img, why, sizeof why)) return -1;
    rm_host_program = &g_img;
    const Frame f = { cam14, W, H, row0, rows, max_iterations, max_distance, hit, t, iters, fs, evals, geom, normal, depth, color, evals_f };
    const int rc = program_has_ext(g_img) ? capture_frame<SceneExtProgram>(f, calls) : capture_frame<SceneProgram>(f, calls);
    rm_host_program = nullptr;
    return rc;
}

// the host-compiled SDFs the restatement takes its four samples from
int rmc_sdf(int scene, const double* xyz, size_t n, double* out)
{
    switch (scene) {
#define RM_X(id, S) case id: for (size_t i = 0; i < n; ++i) out[i] = S::sdf(v3(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2])); return 0;
        RM_SCENE_LIST(RM_X)
#undef RM_X
    }
    return -1;
}

int rmc_sdf_program(const RmSceneOp* ops, int32_t nops, const double* xyz, size_t n, double* out)
{
    char why[256];
    if (!program_encode(ops, nops, &g_img, why, sizeof why)) return -1;
    const ProgSrc src{ &g_img };
    for (size_t i = 0; i < n; ++i) out[i] = program_eval(src, v3(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]));
    return 0;
}

// a whole frame of a program marched by the host build (the CPU oracle has no interpreter); strategy 0 Standard, 10 Segment
int rmc_march_program(const RmSceneOp* ops, int32_t nops, int strategy, int max_iterations, double hit_threshold,
                      double max_distance, double lipschitz, const double* cam14, int W, int H, uint8_t* hit, double* t,
                      int32_t* iters, double* fs)
{
    char why[256];
    if (!program_encode(ops, nops, &g_img, why, sizeof why)) return -1;
    MarchCfg cfg;
    cfg.hit_threshold = hit_threshold; cfg.max_distance = max_distance; cfg.lipschitz = lipschitz;
    cfg.max_iterations = max_iterations; cfg.full = 1;
    cfg.prm = default_strat_params();
    rm_host_program = &g_img;
    int rc = 0;
    if (strategy == 0) march_frame<SceneProgram, StratStandard>(cfg, cam14, W, H, hit, t, iters, fs);
    else if (strategy == 10) march_frame<SceneProgram, StratSegment>(cfg, cam14, W, H, hit, t, iters, fs);
    else rc = -2;
    rm_host_program = nullptr;
    return rc;
}

}
