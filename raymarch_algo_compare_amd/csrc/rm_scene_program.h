// rm_scene_program.h -- user-defined CSG scenes: a postfix program of the reference's scenes/primitives.py functions,
// validated and encoded on the host, evaluated by an interpreter on the device (SceneProgram::sdf).
//
// Format (RmSceneOp, include/rm_hip.h): primitives push a distance, combinators pop two and push one, distance
// modifiers replace the top one, point transforms save the current point and replace it, RM_SOP_POP_POINT restores
// it.  The host resolves every stack position once (program_encode): each instruction word carries its opcode, the
// value slot it writes (a binary combinator reads that slot and the next), the point slot it saves to / restores from,
// and the offset of its constants.  The device never tracks a stack pointer and never indexes an array by a runtime
// value: the eight value slots and four saved points are named registers, selected by selects on the slot number,
// which is wave-uniform (no scratch: a runtime-indexed private array would live there).
//
// Where the program lives: the launch passes the device copy of its ProgramImage (KernelArgs.scene_data); the
// kernel's prologue copies the used part into LDS next to the libm tables (rm_load_scene_data, rm_kernels.h), and
// every instruction word is read with a wave-uniform address and moved to a scalar register (readfirstlane), so the
// opcode dispatch is a chain of scalar branches, not a waterfall over lanes.
//
// Arithmetic: the helpers of rm_scenes.h (py_max / py_min, pow_half, rm_pow(x, 2.0) where the reference writes `** 2`),
// the reference's evaluation order, no contraction; op_repeat uses CPython's float.__mod__ (exact fmod + float_rem's
// sign fix), which equals py_mod_pow2 on the power-of-two spacings of the catalogue (and uses it there).
#pragma once

#include "../../include/rm_hip.h"
#include "rm_scenes.h"

#include <stdio.h>
#include <string.h>

namespace rm {

constexpr int kProgMaxOps = RM_SCENE_PROGRAM_MAX_OPS;
constexpr int kProgMaxArgs = 7;                        // RM_SOP_CAPSULE
constexpr int kProgMaxConst = kProgMaxArgs * kProgMaxOps;
constexpr uint32_t kProgTranslated = 1u << 13;

// The device image of a program (what a launch's scene_data points to).  code[i]: bits 0-5 opcode, 6-9 value slot,
// 10-12 point slot, 13-15 axes of RM_SOP_REPEAT / RM_SOP_LIMITED_REPEAT with a positive spacing, of RM_SOP_ROTATE whose
// (cos, sin) is not exactly (1, 0) and of RM_SOP_MIRROR that are flagged, 16-31 offset of the constants in k[].  Two flags reuse bits a word's opcode leaves free:
//  * a primitive with bit 13 set is `translate, primitive, pop point` fused (its first three constants are the offset):
//    the same arithmetic, p - offset then the primitive, without the trip through the point stack;
//  * RM_SOP_REPEAT: bits 6-8 mark the axes whose spacing is a power of two in [2^-64, 2^64]; there py_mod_pow2 (the
//    catalogue's exact division-free remainder) replaces fmod for |x| < 2^900.
struct ProgramImage {
    int32_t nops, nconst;
    uint32_t code[kProgMaxOps];
    double k[kProgMaxConst];
};

// One instruction word of a ProgramImage, decoded (the only place that knows the bit layout besides program_encode).
struct ProgWord {
    uint32_t w;
    RM_HD int op() const { return (int)(w & 63u); }
    RM_HD int slot() const { return (int)((w >> 6) & 15u); }           // value slot written (a combinator also reads slot + 1)
    RM_HD int pslot() const { return (int)((w >> 10) & 7u); }          // point slot saved to / restored from
    RM_HD int ko() const { return (int)(w >> 16); }                    // offset of the constants in k[]
    RM_HD bool translated() const { return (w & kProgTranslated) != 0; }           // a primitive fused with its translate
    RM_HD bool axis(int a) const { return (w & (1u << (13 + a))) != 0; }           // RM_SOP_REPEAT, RM_SOP_LIMITED_REPEAT: axis a is repeated;
                                                                                   // RM_SOP_ROTATE: turned about; RM_SOP_MIRROR: folded
    RM_HD bool pow2(int a) const { return (w & (1u << (6 + a))) != 0; }            // ... with a power-of-two spacing
};

// constants each opcode reads (RmSceneOp.f)
RM_HD int program_op_args(int op)
{
    switch (op) {
        case RM_SOP_SPHERE: return 1;
        case RM_SOP_BOX: return 3;
        case RM_SOP_PLANE: return 4;
        case RM_SOP_CYLINDER: return 2;
        case RM_SOP_TORUS: return 2;
        case RM_SOP_CAPSULE: return 7;
        case RM_SOP_CAPPED_TORUS: return 4;
        case RM_SOP_CONE: return 3;
        case RM_SOP_SMOOTH_UNION: case RM_SOP_SMOOTH_SUBTRACT: case RM_SOP_SMOOTH_INTERSECT: return 1;
        case RM_SOP_TRANSLATE: case RM_SOP_REPEAT: return 3;
        case RM_SOP_ROUND: case RM_SOP_ONION: case RM_SOP_SCALE: return 1;
        case RM_SOP_LIMITED_REPEAT: return 6;
        case RM_SOP_MENGER_CROSS: case RM_SOP_GYROID: return 2;
        case RM_SOP_ROTATE: return 6;
        case RM_SOP_MIRROR: return 3;
        default: return 0;
    }
}

// the three kinds of op the walks tell apart by their opcode (wave-uniform)
RM_HD bool prog_is_transform(int op)
{
    return (op >= RM_SOP_TRANSLATE && op <= RM_SOP_POP_POINT) || op == RM_SOP_LIMITED_REPEAT || op >= RM_SOP_ROTATE;
}
RM_HD bool prog_is_primitive(int op) { return op <= RM_SOP_CONE || op == RM_SOP_MENGER_CROSS || op == RM_SOP_GYROID; }
// ... of an op that is no transform (the walks take those first): the two comparisons the test had before the placement ops
RM_HD bool prog_pushes(int op) { return op <= RM_SOP_CONE || op >= RM_SOP_MENGER_CROSS; }

// ---- scenes/primitives.py functions rm_scenes.h does not already hold ---------------------------------------------

RM_HD double sd_capsule(vec3 p, vec3 a, vec3 b, double radius)                          // :34-39
{
    vec3 ab = b - a;
    vec3 ap = p - a;
    double t = py_max(0.0, py_min(1.0, dot(ap, ab) / py_max(dot(ab, ab), 1e-12)));
    vec3 closest = a + ab * t;
    return length(p - closest) - radius;
}

// c = math.cos(angle_rad), s = math.sin(angle_rad): computed by the host (the reference's libm), not here
RM_HD double sd_cone(vec3 p, double c, double s, double height)                         // :53-65
{
    double q_len = pow_half(p.x * p.x + p.z * p.z);
    // q = (q_len, p.y, 0); tip_dist (:61) is computed by the reference and never used
    double d1 = p.y - (-height);
    double d2 = q_len * c + p.y * s;
    return py_max(-d1, d2);
}

RM_HD double op_smooth_subtract(double d1, double d2, double k) { return -op_smooth_union(-d1, d2, k); }    // :88-89
RM_HD double op_smooth_intersect(double d1, double d2, double k) { return -op_smooth_union(-d1, -d2, k); }  // :91-92

// float.__mod__ (CPython float_rem) for b > 0: fmod is exact; a non-zero remainder takes the divisor's sign, a zero
// one is +0.0
RM_HD double py_mod(double a, double b)
{
    double m = fmod(a, b);
    if (m != 0.0) {
        if ((b < 0.0) != (m < 0.0)) m += b;
    } else {
        m = 0.0;
    }
    return m;
}

// op_repeat (:102-108), one axis with spacing > 0; pow2: the spacing is a power of two in [2^-64, 2^64] (wave-uniform).
// py_mod_pow2's quotient is exact unless it overflows, which |x| < 2^900 excludes; the guard is a per-lane branch that
// no lane of a ray march takes.
RM_HD double repeat_axis_any(double x, double spacing, bool pow2)
{
    const double a = x + spacing * 0.5;
    double m;
    if (pow2 && rm_fabs(a) < 0x1p900)
        m = py_mod_pow2(a, spacing);
    else
        m = py_mod(a, spacing);
    return m - spacing * 0.5;
}

// ---- the four ops beyond primitives.py (scenes/catalog.py) ------------------------------------------------------------

// the cell index of RM_SOP_LIMITED_REPEAT, one axis with spacing c > 0 (Box Lattice, :584-588): non-decreasing in x
RM_HD double limited_repeat_cell(double x, double c, double l) { return py_max(-l, py_min(l, rm_floor(x / c + 0.5))); }
RM_HD double limited_repeat_axis(double x, double c, double l) { return x - c * limited_repeat_cell(x, c, l); }

// one trip of the Menger loop (:221-237); s3 = s * 3.0 as the host multiplied it.  float.__mod__ by 2.0 is py_mod_pow2 for
// every argument: the quotient a / 2 cannot overflow.
RM_HD double menger_fold(double x, double s) { return rm_fabs(1.0 - 3.0 * rm_fabs(py_mod_pow2(x * s, 2.0) - 1.0)); }
RM_HD double sd_menger_cross(vec3 p, double s, double s3)
{
    const double rx = menger_fold(p.x, s), ry = menger_fold(p.y, s), rz = menger_fold(p.z, s);
    const double da = py_max(rx, ry);
    const double db = py_max(ry, rz);
    const double dc = py_max(rz, rx);
    return (py_min(da, py_min(db, dc)) - 1.0) / s3;
}

// the gyroid sheet (:510-514): NaN where rm_sin / rm_cos are (|freq * p| >= 0x1.921fbp+26 or not finite)
RM_HD double sd_gyroid(vec3 p, double freq, double lipschitz)
{
    // One axis per trip of a loop that stays a loop: rm_sincos is branch-free, every one of its conditions is a wave mask in a
    // scalar register pair, and three copies side by side are what pushes the interpreter's kernels over their scalar
    // registers.  (The catalogue's Gyroid, a kernel of its own, unrolls.)  Same operations on the same values.
    // (the axes rotate through q0 and the results shift through s0..s2 / c0..c2: no select on the trip number, whose
    // masks would be scalar register pairs again)
    double q0 = p.x, q1 = p.y, q2 = p.z;
    double sx = 0.0, cx = 0.0, sy = 0.0, cy = 0.0, sz = 0.0, cz = 0.0;
#pragma unroll 1
    for (int a = 0; a < 3; ++a) {
        double s, c;
        rm_sincos(freq * q0, &s, &c);
        sx = sy; sy = sz; sz = s;
        cx = cy; cy = cz; cz = c;
        const double t = q0;
        q0 = q1; q1 = q2; q2 = t;
    }
    return (sx * cy + sy * cz + sz * cx) / lipschitz;
}

// ---- the two placement ops --------------------------------------------------------------------------------------------------

// one plane of RM_SOP_ROTATE: (u, v) <- (c u + s v, c v - s u), four products and then one add and one subtract (no
// contraction), both from the old pair.  c = 0, s = +-1 (a quarter turn) gives (+-v, -+u) without rounding.
RM_HD void rotate_plane(double& u, double& v, double c, double s)
{
    const double cu = c * u, sv = s * v, cv = c * v, su = s * u;
    u = cu + sv;
    v = cv - su;
}

// ---- the interpreter ----------------------------------------------------------------------------------------------

// N register slots of a T (a record of doubles: double, vec3, Ival, IVec3, DIval), kept lane by lane.  Slot i
// (wave-uniform) is reached by selects on i (v_cndmask with a scalar mask): after unrolling every index below is a
// constant, so the array is split into plain locals and nothing can move it to scratch -- selecting whole records
// instead makes the compiler select an address and load from it, and then the slots live in scratch.
template <class T, int N>
struct Slots {
    static constexpr int kLanes = (int)(sizeof(T) / sizeof(double));
    static_assert(sizeof(T) == kLanes * sizeof(double), "a slot holds doubles only");
    double s[N][kLanes];

    RM_HD explicit Slots(const T& x)
    {
#pragma unroll
        for (int j = 0; j < N; ++j) __builtin_memcpy(s[j], &x, sizeof x);
    }
    RM_HD T at(int j) const
    {
        T r;
        __builtin_memcpy(&r, s[j], sizeof r);
        return r;
    }
    // slot i; `r` where i is no slot (cannot occur after program_encode)
    RM_HD T get(int i, T r) const
    {
        double t[kLanes];
        __builtin_memcpy(t, &r, sizeof r);
#pragma unroll
        for (int l = 0; l < kLanes; ++l)
#pragma unroll
            for (int j = N - 1; j >= 0; --j) t[l] = i == j ? s[j][l] : t[l];
        __builtin_memcpy(&r, t, sizeof r);
        return r;
    }
    // writes slot i, nothing where i is no slot
    RM_HD void set(int i, const T& x)
    {
        double t[kLanes];
        __builtin_memcpy(t, &x, sizeof x);
#pragma unroll
        for (int j = 0; j < N; ++j)
#pragma unroll
            for (int l = 0; l < kLanes; ++l) s[j][l] = i == j ? t[l] : s[j][l];
    }
};

// The walk over a program image for the two sound evaluations of a program: over a box (IntervalAlgebra, rm_interval.h)
// and over a box with the derivative along a ray (DualAlgebra, rm_segment.h).  (program_eval below keeps its own loop:
// DESIGN.md section 3, "Interval oracle".)
// An algebra names its Value and its Point (a record with members x, y, z) and provides the ten primitives, translate,
// repeat and limited repeat of one coordinate, lincomb (a * ca + b * cb of two coordinates) and mirror (abs of a coordinate) for
// the placement ops, the three modifiers and the six combinators.  Src: nops(), word(i) (wave-uniform), k(i).
// One plane of RM_SOP_ROTATE in an algebra: (u, v) <- (c u + s v, c v - s u), the products first, both from the old pair.
// `on` (wave-uniform) is clear for a pair that is exactly (1, 0).
template <class A, class C>
RM_HD void prog_rotate(const A& alg, C& u, C& v, bool on, double c, double s)
{
    if (!on) return;
    const C u0 = u;
    u = alg.lincomb(u0, c, v, s);
    v = alg.lincomb(v, c, u0, -s);
}

template <class A, class Src>
RM_HD typename A::Value program_walk(const A& alg, const Src& src, typename A::Point p)
{
    typedef typename A::Value V;
    typedef typename A::Point P;
    Slots<V, RM_SCENE_PROGRAM_MAX_VALUES> vals{ V() };
    Slots<P, RM_SCENE_PROGRAM_MAX_POINTS> saved{ p };
    const int n = src.nops();
    for (int pc = 0; pc < n; ++pc) {
        const ProgWord w{ src.word(pc) };
        const int slot = w.slot(), pslot = w.pslot(), op = w.op();
        int ko = w.ko();
        if (prog_is_transform(op)) {
            if (op == RM_SOP_POP_POINT) {
                p = saved.get(pslot, p);
            } else {
                saved.set(pslot, p);
                const double kx = src.k(ko), ky = src.k(ko + 1), kz = src.k(ko + 2);
                if (op == RM_SOP_TRANSLATE) {
                    p = alg.translate(p, kx, ky, kz);                                // :99-100
                } else if (op == RM_SOP_REPEAT) {                                    // :102-108
                    if (w.axis(0)) p.x = alg.repeat(p.x, kx, w.pow2(0));
                    if (w.axis(1)) p.y = alg.repeat(p.y, ky, w.pow2(1));
                    if (w.axis(2)) p.z = alg.repeat(p.z, kz, w.pow2(2));
                } else if (op == RM_SOP_LIMITED_REPEAT) {
                    if (w.axis(0)) p.x = alg.limited_repeat(p.x, kx, src.k(ko + 3));
                    if (w.axis(1)) p.y = alg.limited_repeat(p.y, ky, src.k(ko + 4));
                    if (w.axis(2)) p.z = alg.limited_repeat(p.z, kz, src.k(ko + 5));
                } else if (op == RM_SOP_ROTATE) {                                    // about z, then y, then x: the solid's order reversed
                    prog_rotate(alg, p.x, p.y, w.axis(2), src.k(ko + 4), src.k(ko + 5));
                    prog_rotate(alg, p.z, p.x, w.axis(1), kz, src.k(ko + 3));
                    prog_rotate(alg, p.y, p.z, w.axis(0), kx, ky);
                } else {                                                             // RM_SOP_MIRROR
                    if (w.axis(0)) p.x = alg.mirror(p.x);
                    if (w.axis(1)) p.y = alg.mirror(p.y);
                    if (w.axis(2)) p.z = alg.mirror(p.z);
                }
            }
            continue;
        }
        V r;
        if (prog_pushes(op)) {                                                       // primitives: push
            P q = p;
            if (w.translated()) {                                                    // fused op_translate (:99-100)
                q = alg.translate(q, src.k(ko), src.k(ko + 1), src.k(ko + 2));
                ko += 3;
            }
            switch (op) {
                case RM_SOP_SPHERE: r = alg.sphere(q, src.k(ko)); break;
                case RM_SOP_BOX: r = alg.box(q, src.k(ko), src.k(ko + 1), src.k(ko + 2)); break;
                case RM_SOP_PLANE: r = alg.plane(q, src.k(ko), src.k(ko + 1), src.k(ko + 2), src.k(ko + 3)); break;
                case RM_SOP_CYLINDER: r = alg.cylinder(q, src.k(ko), src.k(ko + 1)); break;
                case RM_SOP_TORUS: r = alg.torus(q, src.k(ko), src.k(ko + 1)); break;
                case RM_SOP_CAPSULE:
                    r = alg.capsule(q, v3(src.k(ko), src.k(ko + 1), src.k(ko + 2)), v3(src.k(ko + 3), src.k(ko + 4), src.k(ko + 5)),
                                    src.k(ko + 6));
                    break;
                case RM_SOP_CAPPED_TORUS: r = alg.capped_torus(q, src.k(ko), src.k(ko + 1), src.k(ko + 2), src.k(ko + 3)); break;
                case RM_SOP_MENGER_CROSS: r = alg.menger_cross(q, src.k(ko), src.k(ko + 1)); break;
                case RM_SOP_GYROID: r = alg.gyroid(q, src.k(ko), src.k(ko + 1)); break;
                default: r = alg.cone(q, src.k(ko), src.k(ko + 1), src.k(ko + 2)); break;
            }
        } else {
            const V a = vals.get(slot, vals.at(RM_SCENE_PROGRAM_MAX_VALUES - 1));
            if (op >= RM_SOP_ROUND) {                                                // distance modifiers
                if (op == RM_SOP_SCALE) r = alg.scale(a, src.k(ko));
                else r = op == RM_SOP_ROUND ? alg.round(a, src.k(ko)) : alg.round(alg.abs(a), src.k(ko));   // :110-111, :113-114
            } else {                                                                 // combinators: d1 = a, d2 = b
                const V b = vals.get(slot + 1, vals.at(RM_SCENE_PROGRAM_MAX_VALUES - 1));
                switch (op) {
                    case RM_SOP_UNION: r = alg.union_(a, b); break;                                     // :70
                    case RM_SOP_SUBTRACT: r = alg.subtract(a, b); break;                                // :73
                    case RM_SOP_INTERSECT: r = alg.intersect(a, b); break;                              // :77
                    case RM_SOP_SMOOTH_UNION: r = alg.smooth_union(a, b, src.k(ko)); break;             // :80-86
                    case RM_SOP_SMOOTH_SUBTRACT: r = alg.smooth_subtract(a, b, src.k(ko)); break;       // :88-89
                    default: r = alg.smooth_intersect(a, b, src.k(ko)); break;                          // :91-92
                }
            }
        }
        vals.set(slot, r);
    }
    return vals.at(0);
}

// The point walk.  Its register stacks are plain local variables of program_eval -- eight value slots v0..v7, four saved points
// (x0, y0, z0) .. (x3, y3, z3) -- and slot i (wave-uniform) is reached by selects on i (v_cndmask with a scalar mask).
// No access has a computed address, so nothing can move them to scratch: a struct of slots read through a switch or a
// chain of selects is turned back into a load from a selected address by the compiler, and then lives in scratch.
// Out-of-range slots cannot occur after program_encode; they would read the last slot and write nothing.
#define RM_PV_GET(i, r)                                                                                               \
    do {                                                                                                              \
        r = v7; r = (i) == 6 ? v6 : r; r = (i) == 5 ? v5 : r; r = (i) == 4 ? v4 : r;                                  \
        r = (i) == 3 ? v3_ : r; r = (i) == 2 ? v2 : r; r = (i) == 1 ? v1 : r; r = (i) == 0 ? v0 : r;                  \
    } while (0)
#define RM_PV_SET(i, x)                                                                                               \
    do {                                                                                                              \
        v0 = (i) == 0 ? (x) : v0; v1 = (i) == 1 ? (x) : v1; v2 = (i) == 2 ? (x) : v2; v3_ = (i) == 3 ? (x) : v3_;     \
        v4 = (i) == 4 ? (x) : v4; v5 = (i) == 5 ? (x) : v5; v6 = (i) == 6 ? (x) : v6; v7 = (i) == 7 ? (x) : v7;       \
    } while (0)
#define RM_PP_SET1(j, i, q)                                                                                           \
    do {                                                                                                              \
        x##j = (i) == j ? q.x : x##j; y##j = (i) == j ? q.y : y##j; z##j = (i) == j ? q.z : z##j;                     \
    } while (0)

// Src: nops(), word(i) (wave-uniform), k(i).  EXT: the four ops beyond primitives.py (RM_SOP_SCALE .. RM_SOP_GYROID) and the two
// placement ops (RM_SOP_ROTATE, RM_SOP_MIRROR) are built in (SceneExtProgram below).  Without it every test on them is a compile-time constant and the walk is the one the
// interpreter had before those ops existed -- the host never sends a program that holds one to such a kernel.
template <bool EXT = true, class Src>
RM_HD double program_eval(const Src& src, vec3 p)
{
    double v0 = 0.0, v1 = 0.0, v2 = 0.0, v3_ = 0.0, v4 = 0.0, v5 = 0.0, v6 = 0.0, v7 = 0.0;
    double x0 = p.x, y0 = p.y, z0 = p.z, x1 = p.x, y1 = p.y, z1 = p.z;
    double x2 = p.x, y2 = p.y, z2 = p.z, x3 = p.x, y3 = p.y, z3 = p.z;
    const int n = src.nops();
    for (int pc = 0; pc < n; ++pc) {
        const ProgWord w{ src.word(pc) };
        const int slot = w.slot(), pslot = w.pslot(), ko = w.ko(), op = w.op();
        if (EXT ? prog_is_transform(op) : (op >= RM_SOP_TRANSLATE && op <= RM_SOP_POP_POINT)) {
            if (op == RM_SOP_POP_POINT) {
                vec3 r = v3(x3, y3, z3);
                r = pslot == 2 ? v3(x2, y2, z2) : r;
                r = pslot == 1 ? v3(x1, y1, z1) : r;
                r = pslot == 0 ? v3(x0, y0, z0) : r;
                p = r;
            } else {
                RM_PP_SET1(0, pslot, p); RM_PP_SET1(1, pslot, p); RM_PP_SET1(2, pslot, p); RM_PP_SET1(3, pslot, p);
                const double kx = src.k(ko), ky = src.k(ko + 1), kz = src.k(ko + 2);
                if (op == RM_SOP_TRANSLATE) {
                    p = p - v3(kx, ky, kz);                                          // :99-100
                } else if (!EXT || op == RM_SOP_REPEAT) {                            // :102-108
                    if (w.axis(0)) p.x = repeat_axis_any(p.x, kx, w.pow2(0));
                    if (w.axis(1)) p.y = repeat_axis_any(p.y, ky, w.pow2(1));
                    if (w.axis(2)) p.z = repeat_axis_any(p.z, kz, w.pow2(2));
                } else if (op == RM_SOP_LIMITED_REPEAT) {
                    if (w.axis(0)) p.x = limited_repeat_axis(p.x, kx, src.k(ko + 3));
                    if (w.axis(1)) p.y = limited_repeat_axis(p.y, ky, src.k(ko + 4));
                    if (w.axis(2)) p.z = limited_repeat_axis(p.z, kz, src.k(ko + 5));
                } else if (op == RM_SOP_ROTATE) {                                    // about z, then y, then x: the solid's order reversed
                    if (w.axis(2)) rotate_plane(p.x, p.y, src.k(ko + 4), src.k(ko + 5));
                    if (w.axis(1)) rotate_plane(p.z, p.x, kz, src.k(ko + 3));
                    if (w.axis(0)) rotate_plane(p.y, p.z, kx, ky);
                } else {                                                             // RM_SOP_MIRROR
                    if (w.axis(0)) p.x = rm_fabs(p.x);
                    if (w.axis(1)) p.y = rm_fabs(p.y);
                    if (w.axis(2)) p.z = rm_fabs(p.z);
                }
            }
            continue;
        }
        double r;
        if (EXT ? prog_pushes(op) : op <= RM_SOP_CONE) {                             // primitives: push
            vec3 p0 = p;
            int ko = w.ko();
            if (w.translated()) {                                               // fused op_translate (:99-100)
                p = p - v3(src.k(ko), src.k(ko + 1), src.k(ko + 2));
                ko += 3;
            }
            switch (op) {
                case RM_SOP_SPHERE: r = sd_sphere(p, src.k(ko)); break;
                case RM_SOP_BOX: r = sd_box(p, v3(src.k(ko), src.k(ko + 1), src.k(ko + 2))); break;
                case RM_SOP_PLANE: r = sd_plane(p, v3(src.k(ko), src.k(ko + 1), src.k(ko + 2)), src.k(ko + 3)); break;
                case RM_SOP_CYLINDER: r = sd_cylinder(p, src.k(ko), src.k(ko + 1)); break;
                case RM_SOP_TORUS: r = sd_torus(p, src.k(ko), src.k(ko + 1)); break;
                case RM_SOP_CAPSULE:
                    r = sd_capsule(p, v3(src.k(ko), src.k(ko + 1), src.k(ko + 2)), v3(src.k(ko + 3), src.k(ko + 4), src.k(ko + 5)),
                                   src.k(ko + 6));
                    break;
                case RM_SOP_CAPPED_TORUS: r = sd_capped_torus(p, src.k(ko), src.k(ko + 1), src.k(ko + 2), src.k(ko + 3)); break;
                // The two labels below stay in the switch without EXT too, with the default's body: no such op arrives there,
                // the compiler folds them into the default, and one switch serves both instantiations.
                case RM_SOP_MENGER_CROSS:
                    if constexpr (EXT) r = sd_menger_cross(p, src.k(ko), src.k(ko + 1));
                    else r = sd_cone(p, src.k(ko), src.k(ko + 1), src.k(ko + 2));
                    break;
                case RM_SOP_GYROID:
                    if constexpr (EXT) r = sd_gyroid(p, src.k(ko), src.k(ko + 1));
                    else r = sd_cone(p, src.k(ko), src.k(ko + 1), src.k(ko + 2));
                    break;
                default: r = sd_cone(p, src.k(ko), src.k(ko + 1), src.k(ko + 2)); break;
            }
            p = p0;
        } else {
            double a, b;
            RM_PV_GET(slot, a);
            if (op >= RM_SOP_ROUND) {                                                // distance modifiers
                if (EXT && op == RM_SOP_SCALE) r = a * src.k(ko);
                else r = op == RM_SOP_ROUND ? a - src.k(ko) : rm_fabs(a) - src.k(ko);     // :110-111, :113-114
            } else {                                                                 // combinators: d1 = a, d2 = b
                RM_PV_GET(slot + 1, b);
                switch (op) {
                    case RM_SOP_UNION: r = py_min(a, b); break;                                     // :70
                    case RM_SOP_SUBTRACT: r = py_max(a, -b); break;                                 // :73
                    case RM_SOP_INTERSECT: r = py_max(a, b); break;                                 // :77
                    case RM_SOP_SMOOTH_UNION: r = op_smooth_union(a, b, src.k(ko)); break;          // :80-86
                    case RM_SOP_SMOOTH_SUBTRACT: r = op_smooth_subtract(a, b, src.k(ko)); break;    // :88-89
                    default: r = op_smooth_intersect(a, b, src.k(ko)); break;                       // :91-92
                }
            }
        }
        RM_PV_SET(slot, r);
    }
    return v0;
}
#undef RM_PV_GET
#undef RM_PV_SET
#undef RM_PP_SET1

#if defined(__HIP_DEVICE_COMPILE__)
// the program of the launch, copied by SceneProgram::load (used only by the SceneProgram kernels)
__shared__ uint32_t rm_s_prog_code[kProgMaxOps];
__shared__ double rm_s_prog_k[kProgMaxConst];
__shared__ int32_t rm_s_prog_nops;
struct ProgSrc {
    __device__ __forceinline__ int nops() const { return __builtin_amdgcn_readfirstlane(rm_s_prog_nops); }
    __device__ __forceinline__ uint32_t word(int i) const { return (uint32_t)__builtin_amdgcn_readfirstlane((int)rm_s_prog_code[i]); }
    __device__ __forceinline__ double k(int i) const { return rm_s_prog_k[i]; }
};
#else
// host builds (tests/native): the program SceneProgram::sdf evaluates on this thread
inline thread_local const ProgramImage* rm_host_program = nullptr;
struct ProgSrc {
    const ProgramImage* img;
    int nops() const { return img ? img->nops : 0; }
    uint32_t word(int i) const { return img->code[i]; }
    double k(int i) const { return img->k[i]; }
};
#endif

// The interpreter as a scene functor, in two instantiations: SceneProgram without the four ops beyond primitives.py and
// without the sin / cos table in LDS -- the kernels of every program that holds none of those ops -- and SceneExtProgram with
// both, chosen by the host for a program that holds one (program_has_ext).  DESIGN.md section 3, "Program extensions", has
// the measurements that decided for two and for where the line runs.
template <bool EXT>
struct ProgramScene {
    static constexpr bool kLaunchData = true;
#if defined(__HIP_DEVICE_COMPILE__)
    // prologue of a kernel (all threads of the workgroup; the barrier follows in rm_load_tables).  The bounds are
    // program_encode's; the clamps only keep a corrupt image inside the LDS arrays.
    static __device__ __forceinline__ void load(const void* data)
    {
        const ProgramImage* img = static_cast<const ProgramImage*>(data);
        const int n = min(max(img->nops, 0), kProgMaxOps), nk = min(max(img->nconst, 0), kProgMaxConst);
        for (int i = threadIdx.x; i < n; i += blockDim.x) rm_s_prog_code[i] = img->code[i];
        for (int i = threadIdx.x; i < nk; i += blockDim.x) rm_s_prog_k[i] = img->k[i];
        if (threadIdx.x == 0) rm_s_prog_nops = n;
    }
    static __device__ __forceinline__ double sdf(vec3 p) { return program_eval<EXT>(ProgSrc{}, p); }
#else
#if defined(__HIPCC__)
    static __device__ void load(const void*) {}      // (hipcc's host pass; the device pass has the body above)
#endif
    static inline double sdf(vec3 p) { return program_eval(ProgSrc{ rm_host_program }, p); }
#endif
};

struct SceneProgram : ProgramScene<false> {};
struct SceneExtProgram : ProgramScene<true> {};
// RM_SOP_GYROID reads the sin / cos table: the kernels that hold the op stage it next to the pow tables
template <> struct SceneTables<SceneExtProgram> { static constexpr unsigned value = TB_POW | TB_SINCOS; };

// (host code) does the image hold an op that needs SceneExtProgram's kernels?
inline bool program_has_ext(const ProgramImage& img)
{
    for (int i = 0; i < img.nops; ++i)
        if (ProgWord{ img.code[i] }.op() >= RM_SOP_SCALE) return true;
    return false;
}

// (host code) Validates a program and writes its device image.  false with the reason in `why` for a malformed program: opcode out
// of range, reserved field set, non-finite or (for unused entries) non-zero constant, smooth k == 0 (a division by zero
// in the reference), a scale factor, Menger scale or gyroid lipschitz that is not > 0, a Menger f[1] that is not f[0] * 3.0,
// a negative limit of a limited repeat, a rotate pair that is not a cosine and sine (|c c + s s - 1| > 2^-50), a mirror flag that
// is neither 0.0 nor 1.0, value stack deeper than RM_SCENE_PROGRAM_MAX_VALUES or popped when empty, more than
// RM_SCENE_PROGRAM_MAX_POINTS nested transforms or a pop without a transform, not exactly one value left, a transform
// left open, length outside 1..RM_SCENE_PROGRAM_MAX_OPS.
inline bool program_encode(const RmSceneOp* ops, int32_t nops, ProgramImage* img, char* why, size_t why_len)
{
    if (!ops) return snprintf(why, why_len, "ops is NULL"), false;
    if (nops <= 0 || nops > kProgMaxOps) return snprintf(why, why_len, "program length %d outside 1..%d", nops, kProgMaxOps), false;
    memset(img, 0, sizeof *img);
    uint32_t word[kProgMaxOps];       // per op: opcode and slot fields (validation pass)
    int vsp = 0, psp = 0;
    for (int i = 0; i < nops; ++i) {
        const RmSceneOp& o = ops[i];
        if (o.op < 0 || o.op >= RM_SOP_COUNT) return snprintf(why, why_len, "op %d: opcode %d out of range", i, o.op), false;
        if (o.arg != 0) return snprintf(why, why_len, "op %d: reserved field arg is %d, must be 0", i, o.arg), false;
        const int na = program_op_args(o.op);
        for (int j = 0; j < 8; ++j) {
            const double f = o.f[j];
            if (!(f - f == 0.0)) return snprintf(why, why_len, "op %d: constant f[%d] is not finite", i, j), false;
            if (j >= na && f != 0.0) return snprintf(why, why_len, "op %d: unused constant f[%d] must be 0", i, j), false;
        }
        uint32_t slot = 0, pslot = 0, axes = 0;
        switch (o.op) {
            case RM_SOP_UNION: case RM_SOP_SUBTRACT: case RM_SOP_INTERSECT:
            case RM_SOP_SMOOTH_UNION: case RM_SOP_SMOOTH_SUBTRACT: case RM_SOP_SMOOTH_INTERSECT:
                if (vsp < 2) return snprintf(why, why_len, "op %d: combinator needs two values, the stack holds %d", i, vsp), false;
                if (o.op >= RM_SOP_SMOOTH_UNION && o.f[0] == 0.0) return snprintf(why, why_len, "op %d: smooth k must not be 0", i), false;
                slot = (uint32_t)(vsp - 2);
                --vsp;
                break;
            case RM_SOP_ROUND: case RM_SOP_ONION: case RM_SOP_SCALE:
                if (o.op == RM_SOP_SCALE && !(o.f[0] > 0.0)) return snprintf(why, why_len, "op %d: scale factor must be > 0", i), false;
                if (vsp < 1) return snprintf(why, why_len, "op %d: modifier needs a value, the stack is empty", i), false;
                slot = (uint32_t)(vsp - 1);
                break;
            case RM_SOP_TRANSLATE: case RM_SOP_REPEAT: case RM_SOP_LIMITED_REPEAT: case RM_SOP_ROTATE: case RM_SOP_MIRROR:
                if (o.op == RM_SOP_ROTATE)
                    for (int j = 0; j < 3; ++j) {
                        const double c = o.f[2 * j], s = o.f[2 * j + 1];
                        if (!(rm_fabs(c * c + s * s - 1.0) <= 0x1p-50))
                            return snprintf(why, why_len, "op %d: (f[%d], f[%d]) is not the cosine and sine of an angle", i, 2 * j, 2 * j + 1), false;
                        if (!(c == 1.0 && s == 0.0)) axes |= 1u << j;
                    }
                if (o.op == RM_SOP_MIRROR)
                    for (int j = 0; j < 3; ++j) {
                        if (o.f[j] != 0.0 && o.f[j] != 1.0) return snprintf(why, why_len, "op %d: mirror flag f[%d] must be 0 or 1", i, j), false;
                        if (o.f[j] == 1.0) axes |= 1u << j;
                    }
                if (o.op == RM_SOP_LIMITED_REPEAT)
                    for (int j = 3; j < 6; ++j)
                        if (o.f[j] < 0.0) return snprintf(why, why_len, "op %d: limit f[%d] is negative", i, j), false;
                if (psp >= RM_SCENE_PROGRAM_MAX_POINTS)
                    return snprintf(why, why_len, "op %d: more than %d nested transforms", i, RM_SCENE_PROGRAM_MAX_POINTS), false;
                pslot = (uint32_t)psp++;
                if (o.op == RM_SOP_REPEAT || o.op == RM_SOP_LIMITED_REPEAT)
                    for (int j = 0; j < 3; ++j)
                        if (o.f[j] > 0.0) {
                            axes |= 1u << j;
                            int e = 0;
                            const double m = frexp(o.f[j], &e);
                            if (o.op == RM_SOP_REPEAT && m == 0.5 && e >= -63 && e <= 65) slot |= 1u << j;   // a power of two in [2^-64, 2^64]
                        }
                break;
            case RM_SOP_POP_POINT:
                if (psp < 1) return snprintf(why, why_len, "op %d: pop point without a transform", i), false;
                pslot = (uint32_t)--psp;
                break;
            default:   // primitives
                if (o.op == RM_SOP_MENGER_CROSS) {
                    if (!(o.f[0] > 0.0)) return snprintf(why, why_len, "op %d: Menger scale must be > 0", i), false;
                    if (o.f[1] != o.f[0] * 3.0) return snprintf(why, why_len, "op %d: f[1] must be the scale times 3.0", i), false;
                }
                if (o.op == RM_SOP_GYROID && !(o.f[1] > 0.0)) return snprintf(why, why_len, "op %d: gyroid lipschitz must be > 0", i), false;
                if (vsp >= RM_SCENE_PROGRAM_MAX_VALUES)
                    return snprintf(why, why_len, "op %d: value stack deeper than %d", i, RM_SCENE_PROGRAM_MAX_VALUES), false;
                slot = (uint32_t)vsp++;
                break;
        }
        word[i] = (uint32_t)o.op | slot << 6 | pslot << 10 | axes << 13;
    }
    if (vsp != 1) return snprintf(why, why_len, "program leaves %d values, must leave exactly 1", vsp), false;
    if (psp != 0) return snprintf(why, why_len, "program leaves %d transforms without a pop point", psp), false;
    // emit: `translate, primitive, pop point` becomes one word; constants in op order (at most kProgMaxArgs per op)
    int n = 0, nk = 0;
    for (int i = 0; i < nops; ++i) {
        const RmSceneOp& o = ops[i];
        if (o.op == RM_SOP_TRANSLATE && i + 2 < nops && prog_is_primitive(ops[i + 1].op) && ops[i + 2].op == RM_SOP_POP_POINT) {
            img->code[n++] = word[i + 1] | kProgTranslated | (uint32_t)nk << 16;
            for (int j = 0; j < 3; ++j) img->k[nk++] = o.f[j];
            for (int j = 0; j < program_op_args(ops[i + 1].op); ++j) img->k[nk++] = ops[i + 1].f[j];
            i += 2;
            continue;
        }
        img->code[n++] = word[i] | (uint32_t)nk << 16;
        for (int j = 0; j < program_op_args(o.op); ++j) img->k[nk++] = o.f[j];
    }
    img->nops = n;
    img->nconst = nk;
    return true;
}

}  // namespace rm
