// rm_interval_catalogue.h -- the catalogue scenes that are compositions of primitives.py, as scene programs:
// scene_program.compile_ops(catalogue_expressions()[id]) for the 14 ids (ids 0-8, 12, 13, 14, 17, 19).
// Written by tools/gen_interval_catalogue.py; tests/test_interval_host.py checks it against compile_ops.
// Constants are hex-float literals: Capped Torus's sc = (math.sin(2.0), math.cos(2.0)) are the ones
// SceneCappedTorus (rm_scenes.h) holds; the device never evaluates trigonometry.
#pragma once

#include "../../include/rm_hip.h"

namespace rm {

// scene 0
static const RmSceneOp kIntervalCatalogue0[1] = {
    { 0, 0, { 0x1.0000000000000p+0 } },   // sd_sphere
};
// scene 1
static const RmSceneOp kIntervalCatalogue1[1] = {
    { 2, 0, { 0.0, 0x1.0000000000000p+0, 0.0, -0x1.0000000000000p-1 } },   // sd_plane
};
// scene 2
static const RmSceneOp kIntervalCatalogue2[1] = {
    { 1, 0, { 0x1.0000000000000p+0, 0x1.0000000000000p+0, 0x1.0000000000000p+0 } },   // sd_box
};
// scene 3
static const RmSceneOp kIntervalCatalogue3[1] = {
    { 4, 0, { 0x1.8000000000000p+0, 0x1.999999999999ap-5 } },   // sd_torus
};
// scene 4
static const RmSceneOp kIntervalCatalogue4[1] = {
    { 3, 0, { 0x1.0000000000000p+0, 0x1.8000000000000p+0 } },   // sd_cylinder
};
// scene 5
static const RmSceneOp kIntervalCatalogue5[7] = {
    { 14, 0, { -0x1.028f5c28f5c29p+0, 0.0, 0.0 } },   // op_translate
    { 0, 0, { 0x1.0000000000000p+0 } },   // sd_sphere
    { 16, 0, { 0.0 } },   // pop_point
    { 14, 0, { 0x1.028f5c28f5c29p+0, 0.0, 0.0 } },   // op_translate
    { 0, 0, { 0x1.0000000000000p+0 } },   // sd_sphere
    { 16, 0, { 0.0 } },   // pop_point
    { 8, 0, { 0.0 } },   // op_union
};
// scene 6
static const RmSceneOp kIntervalCatalogue6[3] = {
    { 1, 0, { 0x1.0000000000000p+0, 0x1.0000000000000p+0, 0x1.0000000000000p+0 } },   // sd_box
    { 0, 0, { 0x1.4cccccccccccdp+0 } },   // sd_sphere
    { 9, 0, { 0.0 } },   // op_subtract
};
// scene 7
static const RmSceneOp kIntervalCatalogue7[7] = {
    { 14, 0, { -0x1.0000000000000p-1, 0.0, 0.0 } },   // op_translate
    { 0, 0, { 0x1.999999999999ap-1 } },   // sd_sphere
    { 16, 0, { 0.0 } },   // pop_point
    { 14, 0, { 0x1.0000000000000p-1, 0.0, 0.0 } },   // op_translate
    { 1, 0, { 0x1.3333333333333p-1, 0x1.3333333333333p-1, 0x1.3333333333333p-1 } },   // sd_box
    { 16, 0, { 0.0 } },   // pop_point
    { 11, 0, { 0x1.0000000000000p-1 } },   // op_smooth_union
};
// scene 8
static const RmSceneOp kIntervalCatalogue8[3] = {
    { 0, 0, { 0x1.0000000000000p+1 } },   // sd_sphere
    { 18, 0, { 0x1.999999999999ap-4 } },   // op_onion
    { 18, 0, { 0x1.999999999999ap-5 } },   // op_onion
};
// scene 12
static const RmSceneOp kIntervalCatalogue12[5] = {
    { 15, 0, { 0x1.0000000000000p+1, 0.0, 0x1.0000000000000p+1 } },   // op_repeat
    { 3, 0, { 0x1.3333333333333p-3, 0x1.8000000000000p+1 } },   // sd_cylinder
    { 16, 0, { 0.0 } },   // pop_point
    { 2, 0, { 0.0, 0x1.0000000000000p+0, 0.0, -0x1.8000000000000p+1 } },   // sd_plane
    { 8, 0, { 0.0 } },   // op_union
};
// scene 13
static const RmSceneOp kIntervalCatalogue13[4] = {
    { 15, 0, { 0.0, 0x1.0000000000000p-1, 0.0 } },   // op_repeat
    { 2, 0, { 0.0, 0x1.0000000000000p+0, 0.0, 0.0 } },   // sd_plane
    { 16, 0, { 0.0 } },   // pop_point
    { 18, 0, { 0x1.47ae147ae147bp-7 } },   // op_onion
};
// scene 14
static const RmSceneOp kIntervalCatalogue14[97] = {
    { 2, 0, { 0.0, 0.0, 0.0, -0x1.2a05f20000000p+33 } },   // sd_plane
    { 14, 0, { 0x1.b381d7dbf4880p-2, 0x1.59ba5e353f7cfp+0, 0x1.dfe5c91d14e3cp-1 } },   // op_translate
    { 0, 0, { 0x1.e3a29c779a6b5p-2 } },   // sd_sphere
    { 16, 0, { 0.0 } },   // pop_point
    { 8, 0, { 0.0 } },   // op_union
    { 14, 0, { -0x1.de5c91d14e3bdp-1, -0x1.5bda5119ce076p-1, 0x1.4525460aa64c3p+0 } },   // op_translate
    { 0, 0, { 0x1.b3eab367a0f91p-2 } },   // sd_sphere
    { 16, 0, { 0.0 } },   // pop_point
    { 8, 0, { 0.0 } },   // op_union
    { 14, 0, { -0x1.ae9e1b089a027p+0, 0x1.179a6b50b0f28p+0, 0x1.028f5c28f5c29p+0 } },   // op_translate
    { 0, 0, { 0x1.3c6a7ef9db22dp-2 } },   // sd_sphere
    { 16, 0, { 0.0 } },   // pop_point
    { 8, 0, { 0.0 } },   // op_union
    { 14, 0, { -0x1.be76c8b439581p-4, -0x1.56e2eb1c432cap-1, -0x1.81bda5119ce07p-1 } },   // op_translate
    { 0, 0, { 0x1.dd14e3bcd35a8p-2 } },   // sd_sphere
    { 16, 0, { 0.0 } },   // pop_point
    { 8, 0, { 0.0 } },   // op_union
    { 14, 0, { -0x1.aab367a0f9097p-1, -0x1.7e5c91d14e3bdp-3, 0x1.fbe76c8b43958p-7 } },   // op_translate
    { 0, 0, { 0x1.f39c0ebedfa44p-2 } },   // sd_sphere
    { 16, 0, { 0.0 } },   // pop_point
    { 8, 0, { 0.0 } },   // op_union
    { 14, 0, { 0x1.7487fcb923a2ap-3, 0x1.af487fcb923a3p+0, 0x1.fd7dbf487fcb9p-1 } },   // op_translate
    { 0, 0, { 0x1.ea64c2f837b4ap-2 } },   // sd_sphere
    { 16, 0, { 0.0 } },   // pop_point
    { 8, 0, { 0.0 } },   // op_union
    { 14, 0, { 0x1.a95e9e1b089a0p-2, 0x1.a99999999999ap+0, -0x1.ef9db22d0e560p-1 } },   // op_translate
    { 0, 0, { 0x1.9f06f69446738p-2 } },   // sd_sphere
    { 16, 0, { 0.0 } },   // pop_point
    { 8, 0, { 0.0 } },   // op_union
    { 14, 0, { -0x1.27c1bda5119cep+0, 0x1.87c84b5dcc63fp-2, -0x1.8cf41f212d773p+0 } },   // op_translate
    { 0, 0, { 0x1.3f7ced916872bp-2 } },   // sd_sphere
    { 16, 0, { 0.0 } },   // pop_point
    { 8, 0, { 0.0 } },   // op_union
    { 14, 0, { -0x1.9425aee631f8ap+0, 0x1.9e83e425aee63p-5, -0x1.d6a161e4f7660p-4 } },   // op_translate
    { 0, 0, { 0x1.4a0902de00d1bp-2 } },   // sd_sphere
    { 16, 0, { 0.0 } },   // pop_point
    { 8, 0, { 0.0 } },   // op_union
    { 14, 0, { 0x1.6b1c432ca57a8p+0, 0x1.c1f212d773190p-2, 0x1.89374bc6a7efap-5 } },   // op_translate
    { 0, 0, { 0x1.efb7e90ff9724p-2 } },   // sd_sphere
    { 16, 0, { 0.0 } },   // pop_point
    { 8, 0, { 0.0 } },   // op_union
    { 14, 0, { -0x1.5b573eab367a1p-7, -0x1.b780346dc5d64p-1, -0x1.a8ef34d6a161ep+0 } },   // op_translate
    { 0, 0, { 0x1.9b22d0e560419p-2 } },   // sd_sphere
    { 16, 0, { 0.0 } },   // pop_point
    { 8, 0, { 0.0 } },   // op_union
    { 14, 0, { -0x1.0bb98c7e28241p+0, 0x1.4e48e8a71de6ap-1, -0x1.0495182a9930cp+0 } },   // op_translate
    { 0, 0, { 0x1.475f6fd21ff2ep-2 } },   // sd_sphere
    { 16, 0, { 0.0 } },   // pop_point
    { 8, 0, { 0.0 } },   // op_union
    { 14, 0, { -0x1.c63f141205bc0p-2, -0x1.aff2e48e8a71ep+0, 0x1.1f487fcb923a3p+0 } },   // op_translate
    { 0, 0, { 0x1.e5e353f7ced91p-2 } },   // sd_sphere
    { 16, 0, { 0.0 } },   // pop_point
    { 8, 0, { 0.0 } },   // op_union
    { 14, 0, { -0x1.2cbfb15b573ebp+0, -0x1.9495182a9930cp-1, 0x1.4b089a0275254p+0 } },   // op_translate
    { 0, 0, { 0x1.af34d6a161e4fp-2 } },   // sd_sphere
    { 16, 0, { 0.0 } },   // pop_point
    { 8, 0, { 0.0 } },   // op_union
    { 14, 0, { 0x1.10cb295e9e1b1p-5, 0x1.2e28240b78034p+0, 0x1.e666666666666p-2 } },   // op_translate
    { 0, 0, { 0x1.9f06f69446738p-2 } },   // sd_sphere
    { 16, 0, { 0.0 } },   // pop_point
    { 8, 0, { 0.0 } },   // op_union
    { 14, 0, { 0x1.a4dd2f1a9fbe7p-1, -0x1.638ef34d6a162p+0, 0x1.1e83e425aee63p-3 } },   // op_translate
    { 0, 0, { 0x1.7381d7dbf4880p-2 } },   // sd_sphere
    { 16, 0, { 0.0 } },   // pop_point
    { 8, 0, { 0.0 } },   // op_union
    { 14, 0, { 0x1.b089a02752546p-6, 0x1.4339c0ebedfa4p+0, -0x1.e305532617c1cp-2 } },   // op_translate
    { 0, 0, { 0x1.7b4a2339c0ebfp-2 } },   // sd_sphere
    { 16, 0, { 0.0 } },   // pop_point
    { 8, 0, { 0.0 } },   // op_union
    { 14, 0, { 0x1.55cfaacd9e83ep-2, -0x1.7f9db22d0e560p+0, -0x1.874538ef34d6ap-2 } },   // op_translate
    { 0, 0, { 0x1.54af4f0d844d0p-2 } },   // sd_sphere
    { 16, 0, { 0.0 } },   // pop_point
    { 8, 0, { 0.0 } },   // op_union
    { 14, 0, { -0x1.341205bc01a37p-1, -0x1.3075f6fd21ff3p+0, 0x1.1353f7ced9168p+0 } },   // op_translate
    { 0, 0, { 0x1.27525460aa64cp-2 } },   // sd_sphere
    { 16, 0, { 0.0 } },   // pop_point
    { 8, 0, { 0.0 } },   // op_union
    { 14, 0, { -0x1.a3bcd35a85879p-2, 0x1.a0b0f27bb2fecp+0, 0x1.395810624dd2fp-2 } },   // op_translate
    { 0, 0, { 0x1.e425aee631f8ap-2 } },   // sd_sphere
    { 16, 0, { 0.0 } },   // pop_point
    { 8, 0, { 0.0 } },   // op_union
    { 14, 0, { 0x1.6dc5d63886595p-2, 0x1.e075f6fd21ff3p-2, 0x1.332617c1bda51p-1 } },   // op_translate
    { 0, 0, { 0x1.8816f0068db8cp-2 } },   // sd_sphere
    { 16, 0, { 0.0 } },   // pop_point
    { 8, 0, { 0.0 } },   // op_union
    { 14, 0, { -0x1.2ff2e48e8a71ep+0, -0x1.9f8a0902de00dp-3, -0x1.c5604189374bcp-1 } },   // op_translate
    { 0, 0, { 0x1.9a1cac083126fp-2 } },   // sd_sphere
    { 16, 0, { 0.0 } },   // pop_point
    { 8, 0, { 0.0 } },   // op_union
    { 14, 0, { -0x1.5374bc6a7ef9ep-2, -0x1.5f06f69446738p+0, 0x1.97318fc504817p+0 } },   // op_translate
    { 0, 0, { 0x1.67525460aa64cp-2 } },   // sd_sphere
    { 16, 0, { 0.0 } },   // pop_point
    { 8, 0, { 0.0 } },   // op_union
    { 14, 0, { -0x1.f020c49ba5e35p-1, 0x1.2b020c49ba5e3p-1, -0x1.5b71758e21965p-1 } },   // op_translate
    { 0, 0, { 0x1.c7fcb923a29c7p-2 } },   // sd_sphere
    { 16, 0, { 0.0 } },   // pop_point
    { 8, 0, { 0.0 } },   // op_union
};
// scene 17
static const RmSceneOp kIntervalCatalogue17[1] = {
    { 6, 0, { 0x1.d18f6ead1b446p-1, -0x1.aa22657537205p-2, 0x1.3333333333333p+0, 0x1.999999999999ap-3 } },   // sd_capped_torus
};
// scene 19
static const RmSceneOp kIntervalCatalogue19[23] = {
    { 14, 0, { 0.0, 0.0, 0.0 } },   // op_translate
    { 0, 0, { 0x1.999999999999ap-1 } },   // sd_sphere
    { 16, 0, { 0.0 } },   // pop_point
    { 14, 0, { 0x1.0000000000000p+0, 0.0, 0.0 } },   // op_translate
    { 0, 0, { 0x1.3333333333333p-1 } },   // sd_sphere
    { 16, 0, { 0.0 } },   // pop_point
    { 11, 0, { 0x1.ccccccccccccdp-2 } },   // op_smooth_union
    { 14, 0, { -0x1.0000000000000p+0, 0.0, 0.0 } },   // op_translate
    { 0, 0, { 0x1.3333333333333p-1 } },   // sd_sphere
    { 16, 0, { 0.0 } },   // pop_point
    { 11, 0, { 0x1.ccccccccccccdp-2 } },   // op_smooth_union
    { 14, 0, { 0.0, 0x1.0000000000000p+0, 0.0 } },   // op_translate
    { 0, 0, { 0x1.3333333333333p-1 } },   // sd_sphere
    { 16, 0, { 0.0 } },   // pop_point
    { 11, 0, { 0x1.ccccccccccccdp-2 } },   // op_smooth_union
    { 14, 0, { 0.0, -0x1.0000000000000p+0, 0.0 } },   // op_translate
    { 0, 0, { 0x1.3333333333333p-1 } },   // sd_sphere
    { 16, 0, { 0.0 } },   // pop_point
    { 11, 0, { 0x1.ccccccccccccdp-2 } },   // op_smooth_union
    { 14, 0, { 0.0, 0.0, 0x1.0000000000000p+0 } },   // op_translate
    { 0, 0, { 0x1.3333333333333p-1 } },   // sd_sphere
    { 16, 0, { 0.0 } },   // pop_point
    { 11, 0, { 0x1.ccccccccccccdp-2 } },   // op_smooth_union
};

// the program of catalogue scene `id`, nullptr for a scene without one (Mandelbulb, Menger, Gyroid, ...)
inline const RmSceneOp* interval_catalogue_ops(int id, int32_t* nops)
{
    switch (id) {
        case 0: *nops = (int32_t)(sizeof kIntervalCatalogue0 / sizeof(RmSceneOp)); return kIntervalCatalogue0;
        case 1: *nops = (int32_t)(sizeof kIntervalCatalogue1 / sizeof(RmSceneOp)); return kIntervalCatalogue1;
        case 2: *nops = (int32_t)(sizeof kIntervalCatalogue2 / sizeof(RmSceneOp)); return kIntervalCatalogue2;
        case 3: *nops = (int32_t)(sizeof kIntervalCatalogue3 / sizeof(RmSceneOp)); return kIntervalCatalogue3;
        case 4: *nops = (int32_t)(sizeof kIntervalCatalogue4 / sizeof(RmSceneOp)); return kIntervalCatalogue4;
        case 5: *nops = (int32_t)(sizeof kIntervalCatalogue5 / sizeof(RmSceneOp)); return kIntervalCatalogue5;
        case 6: *nops = (int32_t)(sizeof kIntervalCatalogue6 / sizeof(RmSceneOp)); return kIntervalCatalogue6;
        case 7: *nops = (int32_t)(sizeof kIntervalCatalogue7 / sizeof(RmSceneOp)); return kIntervalCatalogue7;
        case 8: *nops = (int32_t)(sizeof kIntervalCatalogue8 / sizeof(RmSceneOp)); return kIntervalCatalogue8;
        case 12: *nops = (int32_t)(sizeof kIntervalCatalogue12 / sizeof(RmSceneOp)); return kIntervalCatalogue12;
        case 13: *nops = (int32_t)(sizeof kIntervalCatalogue13 / sizeof(RmSceneOp)); return kIntervalCatalogue13;
        case 14: *nops = (int32_t)(sizeof kIntervalCatalogue14 / sizeof(RmSceneOp)); return kIntervalCatalogue14;
        case 17: *nops = (int32_t)(sizeof kIntervalCatalogue17 / sizeof(RmSceneOp)); return kIntervalCatalogue17;
        case 19: *nops = (int32_t)(sizeof kIntervalCatalogue19 / sizeof(RmSceneOp)); return kIntervalCatalogue19;
    }
    *nops = 0;
    return nullptr;
}

}  // namespace rm
