// Host-only check build of the scene-program interpreter (csrc/rm_scene_program.h) -- compiled by g++ for tests ONLY,
// so the exact source the gfx950 kernels are built from can be diffed against the reference's fixtures in a container
// without a GPU.  Never loaded by the product.
#include <stddef.h>
#include <stdint.h>
#include "../../raymarch_algo_compare_amd/csrc/rm_scene_program.h"

using namespace rm;

extern "C" {

// program_encode of the library (validation + encoding); 0 or -1 with the reason in why
int rmp_encode(const RmSceneOp* ops, int32_t nops, ProgramImage* img, char* why, int why_len)
{
    return program_encode(ops, nops, img, why, (size_t)why_len) ? 0 : -1;
}

// SceneProgram::sdf over n points (xyz: n x 3)
int rmp_eval(const RmSceneOp* ops, int32_t nops, const double* xyz, size_t n, double* out, char* why, int why_len)
{
    static thread_local ProgramImage img;
    if (!program_encode(ops, nops, &img, why, (size_t)why_len)) return -1;
    rm_host_program = &img;
    for (size_t i = 0; i < n; ++i) out[i] = SceneProgram::sdf(v3(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]));
    rm_host_program = nullptr;
    return 0;
}

size_t rmp_sizeof_op(void) { return sizeof(RmSceneOp); }
size_t rmp_offsetof_f(void) { return offsetof(RmSceneOp, f); }
size_t rmp_sizeof_image(void) { return sizeof(ProgramImage); }

}
