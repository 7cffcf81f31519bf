// Host-only check build of the strategy-program interpreter (csrc/rm_strategy_program.h) -- compiled by g++ for tests
// ONLY: strategy_encode as the library runs it, and march_one<Scene, StratProgram> over explicit rays, so the source the
// gfx950 kernels are built from can be compared with the compiled strategies (tests/native/host_check.cpp) and with the
// NumPy machine without a GPU.  Never loaded by the product.
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include "../../raymarch_algo_compare_amd/csrc/rm_scenes.h"
#include "../../raymarch_algo_compare_amd/csrc/rm_strategy_program.h"

using namespace rm;

template <class Scene>
static void rays_t(const MarchCfg& cfg, const double* origins, const double* dirs, size_t n, uint8_t* hit, double* t,
                   int32_t* iters, double* fs, int32_t* evals)
{
    for (size_t i = 0; i < n; ++i) {
        const vec3 o = v3(origins[3 * i], origins[3 * i + 1], origins[3 * i + 2]);
        const vec3 d = normalized(v3(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]));
        const Result res = march_one<Scene, StratProgram>(o, d, cfg);
        hit[i] = (uint8_t)res.hit; t[i] = res.t; iters[i] = res.iters; fs[i] = res.final_sdf;
        if (evals) {      // the same loop once more, counting what the kernels count
            StratProgram s;
            int nev = 0;
            bool done = s.start(cfg);
            while (!done) {
                const double v = Scene::sdf(o + d * s.te);
                ++nev;
                done = s.step(v, cfg);
            }
            evals[i] = nev;
        }
    }
}

extern "C" {

// 1 and the image's instruction and constant counts, or 0 with the reason in `why`
int rsp_encode(const RmStrategyOp* ops, int32_t nops, char* why, size_t why_len, int32_t* counts)
{
    StrategyImage img;
    if (why_len) why[0] = 0;
    if (!strategy_encode(ops, nops, &img, why, why_len)) return 0;
    if (counts) { counts[0] = img.nops; counts[1] = img.nconst; }
    return 1;
}

// -1 unknown scene, -6 a program strategy_encode refuses (reason on stderr)
int rsp_march_rays(int scene, const RmStrategyOp* ops, int32_t nops, int max_iterations, double hit_threshold,
                   double max_distance, double lipschitz, int full, const double* origins, const double* dirs, size_t n,
                   uint8_t* hit, double* t, int32_t* iters, double* fs, int32_t* evals)
{
    StrategyImage img;
    char why[256];
    if (!strategy_encode(ops, nops, &img, why, sizeof why)) {
        fprintf(stderr, "strategy_program_check: %s\n", why);
        return -6;
    }
    MarchCfg cfg;
    cfg.hit_threshold = hit_threshold; cfg.max_distance = max_distance; cfg.lipschitz = lipschitz;
    cfg.max_iterations = max_iterations; cfg.full = full;
    cfg.prm = default_strat_params();
    rm_host_strategy = &img;
    int rc = -1;
    switch (scene) {
#define RM_X(id, S) case id: rays_t<S>(cfg, origins, dirs, n, hit, t, iters, fs, evals); rc = 0; break;
        RM_SCENE_LIST(RM_X)
#undef RM_X
    }
    rm_host_strategy = nullptr;
    return rc;
}

int rsp_sizeof_op(void) { return (int)sizeof(RmStrategyOp); }
int rsp_offsetof_op(int field)
{
    switch (field) {
        case 0: return (int)offsetof(RmStrategyOp, op);
        case 1: return (int)offsetof(RmStrategyOp, dst);
        case 2: return (int)offsetof(RmStrategyOp, a);
        case 3: return (int)offsetof(RmStrategyOp, b);
        case 4: return (int)offsetof(RmStrategyOp, c);
        case 5: return (int)offsetof(RmStrategyOp, reserved);
        default: return (int)offsetof(RmStrategyOp, k);
    }
}

}
