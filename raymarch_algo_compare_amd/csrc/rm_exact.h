// rm_exact.h -- the exact first hit of a hard-CSG scene program along a ray: closed-form ray / surface intersection and
// set algebra, the one ground truth of the project that shares no algorithm with marching ("Exact
// first hit").  Compiles for the device and, with g++ -ffp-contract=off, for the host (tests/native/exact_check.cpp).
//
// Semantics.  For the ray o + t d (d as given) S = { t : f(o + t d) <= 0 } is built from closed per-leaf sets: op_union
// is the union, op_intersect the intersection, op_subtract(a, b) is A with closure(R \ B); op_translate moves the origin,
// op_rotate / op_turn turn origin and direction into the child's frame (the hit normal is turned back into the world's);
// op_round(child, r) cuts the child at level + r, op_scale(child, k) at level / k, op_onion(child, th) maps a level range
// [a, b] to [max(a + th, 0), b + th] and its mirror image.  The result is the smallest end point t_min < t <= t_max of a
// maximal interval of S -- an entry, an exit (eye inside the solid) or a contact of measure zero ([t, t]).
//
// Structure.  The program is the same for every lane, so every walk is wave-uniform and nothing is indexed per lane.
// Instead of interval lists, S is examined through its germs: the local shape of a closed set at one t, three bits
// (member just before t, at t, just after t).  Germs combine bit for bit: union |, intersection &, closure of the
// complement: before and after flip, `at` is set unless all three were.  Every end point of a maximal interval of S is a
// root of some leaf, so: for each leaf and each of its roots (exact_first_hit), walk the program once more with the germ
// of every leaf at that t, from that leaf's freshly computed roots (exact_germ_at), and keep the smallest t at which the
// germ of the whole program is a boundary (at, and not both before and after).  The candidate leaf is on its boundary
// in that walk because the same expressions on the same values give the same bits.  O(leaves^2) quadratics per ray.
//
// Modifiers (round, onion, scale) are folded into the leaf they follow: a leaf and its chain of modifiers is the leaf's
// own distance g restricted to a union of level ranges la <= g <= lb, one per choice of side at every onion.  Sphere,
// plane, torus and capsule are cut at any level (the radius or offset moves); box and cylinder at level 0 only.
// exact_supported names what has no exact form here.
#pragma once

#include "rm_camera.h"
#include "rm_scene_program.h"

namespace rm {

constexpr int kExactMaxOnions = 3;      // onions in one leaf's chain: 2^3 level ranges
constexpr int kExactBisect = 64;        // trips of one bisection: the window shrinks to 2^-64 of its width

// ---- germs ---------------------------------------------------------------------------------------------------------
// bit 0: member just before t, bit 1: at t, bit 2: just after t
RM_HD uint32_t ex_germ(double a, double b, double t)            // of the closed interval [a, b]; a > b: empty
{
    return (a < t && t <= b ? 1u : 0u) | (a <= t && t <= b ? 2u : 0u) | (a <= t && t < b ? 4u : 0u);
}
RM_HD uint32_t ex_cc(uint32_t g) { return (~g & 5u) | (g != 7u ? 2u : 0u); }       // closure of the complement
RM_HD bool ex_boundary(uint32_t g) { return (g & 2u) != 0 && (g & 5u) != 5u; }

// ---- leaves: { t : g(o + t d) <= level } as at most two closed intervals ------------------------------------------------
struct ExCut {
    double a0, b0, a1, b1;
};
RM_HD ExCut ex_cut(double a0, double b0)
{
    ExCut c;
    c.a0 = a0; c.b0 = b0; c.a1 = __builtin_inf(); c.b1 = -__builtin_inf();
    return c;
}
RM_HD ExCut ex_empty() { return ex_cut(__builtin_inf(), -__builtin_inf()); }
RM_HD ExCut ex_meet(ExCut x, ExCut y)             // of two single intervals
{
    const double a = x.a0 > y.a0 ? x.a0 : y.a0, b = x.b0 < y.b0 ? x.b0 : y.b0;
    return a <= b ? ex_cut(a, b) : ex_empty();
}
RM_HD ExCut ex_hull(ExCut x, ExCut y)             // of two single intervals whose union is connected
{
    if (!(x.a0 <= x.b0)) return y;
    if (!(y.a0 <= y.b0)) return x;
    return ex_cut(x.a0 < y.a0 ? x.a0 : y.a0, x.b0 > y.b0 ? x.b0 : y.b0);
}
RM_HD uint32_t ex_cut_germ(ExCut c, double t) { return ex_germ(c.a0, c.b0, t) | ex_germ(c.a1, c.b1, t); }

// A t^2 + 2 hb t + C <= 0 with A >= 0: the cancellation-free form q = -(hb + sign(hb) sqrt(disc)), roots q / A and C / q
RM_HD ExCut ex_quadratic(double A, double hb, double C)
{
    if (!(A > 0.0)) return C <= 0.0 ? ex_cut(-__builtin_inf(), __builtin_inf()) : ex_empty();     // no t^2 term: all or nothing
    const double disc = hb * hb - A * C;
    if (!(disc >= 0.0)) return ex_empty();
    const double root = rm_sqrt(disc);
    const double q = -(hb + (hb < 0.0 ? -root : root));
    if (q == 0.0) return ex_cut(0.0, 0.0);                       // hb == 0 and disc == 0: a double root at 0
    const double r0 = q / A, r1 = C / q;
    return r0 <= r1 ? ex_cut(r0, r1) : ex_cut(r1, r0);
}
// lo <= m0 + t m1 <= hi; empty for lo > hi (a negative half extent: the primitive's distance is positive everywhere)
RM_HD ExCut ex_slab(double m0, double m1, double lo, double hi)
{
    if (!(lo <= hi)) return ex_empty();
    if (m1 == 0.0) return (m0 >= lo && m0 <= hi) ? ex_cut(-__builtin_inf(), __builtin_inf()) : ex_empty();
    const double t0 = (lo - m0) / m1, t1 = (hi - m0) / m1;
    return t0 <= t1 ? ex_cut(t0, t1) : ex_cut(t1, t0);
}

RM_HD ExCut ex_sphere(vec3 o, vec3 d, double radius)
{
    if (!(radius >= 0.0)) return ex_empty();
    return ex_quadratic(dot(d, d), dot(o, d), dot(o, o) - radius * radius);
}
// dot(p, n) - offset <= 0
RM_HD ExCut ex_plane(vec3 o, vec3 d, vec3 n, double offset)
{
    const double dn = dot(d, n), on = dot(o, n);
    if (dn == 0.0) return on - offset <= 0.0 ? ex_cut(-__builtin_inf(), __builtin_inf()) : ex_empty();
    const double t = (offset - on) / dn;
    return dn < 0.0 ? ex_cut(t, __builtin_inf()) : ex_cut(-__builtin_inf(), t);
}
RM_HD ExCut ex_box(vec3 o, vec3 d, vec3 h)                        // the slab method
{
    return ex_meet(ex_meet(ex_slab(o.x, d.x, -h.x, h.x), ex_slab(o.y, d.y, -h.y, h.y)), ex_slab(o.z, d.z, -h.z, h.z));
}
RM_HD ExCut ex_cylinder(vec3 o, vec3 d, double radius, double half_height)      // about the y axis
{
    if (!(radius >= 0.0)) return ex_empty();
    const ExCut side = ex_quadratic(d.x * d.x + d.z * d.z, o.x * d.x + o.z * d.z, (o.x * o.x + o.z * o.z) - radius * radius);
    return ex_meet(side, ex_slab(o.y, d.y, -half_height, half_height));
}
// a finite cylinder about the segment a b and a sphere at either end; the union of the three is convex
RM_HD ExCut ex_capsule(vec3 o, vec3 d, vec3 a, vec3 b, double radius)
{
    if (!(radius >= 0.0)) return ex_empty();
    const vec3 ab = b - a, oa = o - a;
    const double l2 = dot(ab, ab);
    ExCut c = ex_hull(ex_sphere(oa, d, radius), ex_sphere(o - b, d, radius));
    if (l2 > 0.0) {
        const double m0 = dot(oa, ab), m1 = dot(d, ab);
        const ExCut side = ex_quadratic(l2 * dot(d, d) - m1 * m1, l2 * dot(oa, d) - m0 * m1, l2 * (dot(oa, oa) - radius * radius) - m0 * m0);
        c = ex_hull(c, ex_meet(side, ex_slab(m0, m1, 0.0, l2)));
    }
    return c;
}

// The torus about the y axis, (rho - R)^2 + y^2 <= r^2 with rho = sqrt(x^2 + z^2): the quartic
//   F(s) = u^2 - 4 R^2 v,  u = |p|^2 + R^2 - r^2,  v = rho^2,  p = c + s d,  c the ray's point nearest the origin,
// has the sign of h = (rho - R)^2 + y^2 - r^2 while r < R.  No eigenvalues: the closed-form roots of F'' (a quadratic)
// bracket the roots of F' (a cubic), those bracket the roots of F; every bracket is finished by bisection, kExactBisect
// trips at the most, the cubic on F', the quartic on the sign of h itself -- the residual the caller sees.  Only the
// window |s| <= (R + r) / |d| (with slack), outside which the ray is outside the torus' bounding sphere, is searched.
struct ExTorusRay {
    vec3 c, d;
    double A, B, K, a2, b2, R, r2, k4;
};
RM_HD double ex_torus_h(const ExTorusRay& T, double s)
{
    const double x = T.c.x + s * T.d.x, y = T.c.y + s * T.d.y, z = T.c.z + s * T.d.z;
    const double q = rm_sqrt(x * x + z * z) - T.R;
    return (q * q + y * y) - T.r2;
}
RM_HD double ex_torus_dF(const ExTorusRay& T, double s)
{
    const double u = (T.A * s + T.B) * s + T.K;
    return 2.0 * u * (2.0 * T.A * s + T.B) - T.k4 * (2.0 * T.a2 * s + T.b2);
}
// the root of F' in [lo, hi] where its signs differ at the ends, else hi
RM_HD double ex_torus_critical(const ExTorusRay& T, double lo, double hi)
{
    const bool neg_lo = ex_torus_dF(T, lo) < 0.0;
    if (neg_lo == (ex_torus_dF(T, hi) < 0.0)) return hi;
    for (int i = 0; i < kExactBisect; ++i) {
        const double mid = lo + (hi - lo) * 0.5;
        if (mid == lo || mid == hi) break;
        if ((ex_torus_dF(T, mid) < 0.0) == neg_lo) lo = mid; else hi = mid;
    }
    return hi;
}
// the last s of [lo, hi] on lo's side of the surface, or the first on hi's: the one inside the solid (h <= 0)
RM_HD double ex_torus_root(const ExTorusRay& T, double lo, double hi, bool in_lo)
{
    for (int i = 0; i < kExactBisect; ++i) {
        const double mid = lo + (hi - lo) * 0.5;
        if (mid == lo || mid == hi) break;
        if ((ex_torus_h(T, mid) <= 0.0) == in_lo) lo = mid; else hi = mid;
    }
    return in_lo ? lo : hi;
}
RM_HD ExCut ex_torus(vec3 o, vec3 d, double R, double r)
{
    ExCut cut = ex_empty();
    const double A = dot(d, d);
    if (!(r >= 0.0) || !(A > 0.0)) return cut;
    ExTorusRay T;
    const double tc = -dot(o, d) / A;
    T.c = v3(o.x + tc * d.x, o.y + tc * d.y, o.z + tc * d.z);
    T.d = d;
    T.A = A;
    T.B = 2.0 * dot(T.c, d);
    T.R = R;
    T.r2 = r * r;
    T.K = dot(T.c, T.c) + R * R - T.r2;
    T.a2 = d.x * d.x + d.z * d.z;
    T.b2 = 2.0 * (T.c.x * d.x + T.c.z * d.z);
    T.k4 = 4.0 * R * R;
    const double W = (R + r) / rm_sqrt(A) * 1.000001 + 1e-9;
    // F'' = 12 A^2 s^2 + 12 A B s + (2 B^2 + 4 A K - 2 k4 a2)
    double i0 = -W, i1 = -W;
    {
        const ExCut f2 = ex_quadratic(12.0 * A * A, 6.0 * A * T.B, 2.0 * T.B * T.B + 4.0 * A * T.K - 2.0 * T.k4 * T.a2);
        if (f2.a0 <= f2.b0) {
            i0 = f2.a0 < -W ? -W : (f2.a0 > W ? W : f2.a0);
            i1 = f2.b0 < -W ? -W : (f2.b0 > W ? W : f2.b0);
        }
    }
    double e[5];
    e[0] = -W;
    e[1] = ex_torus_critical(T, -W, i0);
    e[2] = ex_torus_critical(T, i0, i1);
    e[3] = ex_torus_critical(T, i1, W);
    e[4] = W;
    bool in_prev = false;                 // the window's ends are outside the bounding sphere
    int closed = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const bool in_next = j < 3 ? ex_torus_h(T, e[j + 1]) <= 0.0 : false;
        if (in_next != in_prev) {
            const double t = tc + ex_torus_root(T, e[j], e[j + 1], in_prev);
            if (in_next) {                // the solid begins
                if (closed == 0) cut.a0 = t; else cut.a1 = t;
            } else {                      // ... and ends
                if (closed == 0) cut.b0 = t; else cut.b1 = t;
                ++closed;
            }
        }
        in_prev = in_next;
    }
    return cut;
}

// ---- a leaf, its chain of modifiers and its level ranges ------------------------------------------------------------

RM_HD bool ex_is_modifier(int op) { return op == RM_SOP_ROUND || op == RM_SOP_ONION || op == RM_SOP_SCALE; }
RM_HD bool ex_is_combinator(int op) { return op >= RM_SOP_UNION && op <= RM_SOP_SMOOTH_INTERSECT; }

// The modifiers applied to the value the leaf at word `pc` pushed (slot `slot`) before a combinator consumes it: the
// index of the last one (pc without any) and the number of onions among them.  Wave-uniform.
template <class Src>
RM_HD void exact_chain(const Src& src, int pc, int slot, int* last, int* onions)
{
    const int n = src.nops();
    int qe = pc, no = 0;
    for (int q = pc + 1; q < n; ++q) {
        const ProgWord w{ src.word(q) };
        const int op = w.op();
        if (ex_is_combinator(op) && w.slot() <= slot) break;
        if (ex_is_modifier(op) && w.slot() == slot) {
            qe = q;
            if (op == RM_SOP_ONION) ++no;
        }
    }
    *last = qe;
    *onions = no;
}

// The level range la <= g <= lb of the leaf's own distance that the chain (pc, last] maps to `value <= 0`, for one choice
// of side at every onion (bit i of `combo`: the i-th onion from the outside takes its negative side).  la = -inf: no
// lower bound.  An empty range: la = +inf, lb = -inf.
template <class Src>
RM_HD void exact_range(const Src& src, int pc, int slot, int last, int combo, double* la_out, double* lb_out)
{
    double la = -__builtin_inf(), lb = 0.0;
    for (int q = last; q > pc; --q) {
        const ProgWord w{ src.word(q) };
        const int op = w.op();
        if (!ex_is_modifier(op) || w.slot() != slot) continue;
        const double k = src.k(w.ko());
        if (op == RM_SOP_ROUND) {
            la = la + k; lb = lb + k;
        } else if (op == RM_SOP_SCALE) {
            la = la / k; lb = lb / k;
        } else {
            const double a = py_max(la + k, 0.0), b = lb + k;        // a <= |g| <= b
            const bool neg = (combo & 1) != 0;
            combo >>= 1;
            la = neg ? -b : a;
            lb = neg ? -a : b;
            if (!(a <= b)) { la = __builtin_inf(); lb = -__builtin_inf(); }
        }
    }
    *la_out = la;
    *lb_out = lb;
}

// { t : g <= level } of the primitive `op` with its constants at k[ko], the ray in the leaf's frame
template <class Src>
RM_HD ExCut exact_leaf_cut(const Src& src, int op, int ko, vec3 o, vec3 d, double level)
{
    switch (op) {
        case RM_SOP_SPHERE: return ex_sphere(o, d, src.k(ko) + level);
        case RM_SOP_BOX: return ex_box(o, d, v3(src.k(ko), src.k(ko + 1), src.k(ko + 2)));
        case RM_SOP_PLANE: return ex_plane(o, d, v3(src.k(ko), src.k(ko + 1), src.k(ko + 2)), src.k(ko + 3) + level);
        case RM_SOP_CYLINDER: return ex_cylinder(o, d, src.k(ko), src.k(ko + 1));
        case RM_SOP_TORUS: return ex_torus(o, d, src.k(ko), src.k(ko + 1) + level);
        case RM_SOP_CAPSULE:
            return ex_capsule(o, d, v3(src.k(ko), src.k(ko + 1), src.k(ko + 2)), v3(src.k(ko + 3), src.k(ko + 4), src.k(ko + 5)),
                              src.k(ko + 6) + level);
        default: return ex_empty();       // (exact_supported refuses the program)
    }
}

// the closed-form gradient of the primitive's distance at p (in the leaf's frame), not normalised
template <class Src>
RM_HD vec3 exact_leaf_gradient(const Src& src, int op, int ko, vec3 p)
{
    switch (op) {
        case RM_SOP_BOX: {                // the face with the largest |p| / half, the first one on ties
            const double qx = rm_fabs(p.x) / src.k(ko), qy = rm_fabs(p.y) / src.k(ko + 1), qz = rm_fabs(p.z) / src.k(ko + 2);
            const int ax = (qx >= qy && qx >= qz) ? 0 : (qy >= qz ? 1 : 2);
            const double c = ax == 0 ? p.x : (ax == 1 ? p.y : p.z);
            const double s = c > 0.0 ? 1.0 : (c < 0.0 ? -1.0 : 0.0);
            return v3(ax == 0 ? s : 0.0, ax == 1 ? s : 0.0, ax == 2 ? s : 0.0);
        }
        case RM_SOP_PLANE: return v3(src.k(ko), src.k(ko + 1), src.k(ko + 2));
        case RM_SOP_CYLINDER: {           // the side where the radial distance is the larger one, else a cap
            const double rho = rm_sqrt(p.x * p.x + p.z * p.z);
            if (rho - src.k(ko) > rm_fabs(p.y) - src.k(ko + 1)) return v3(p.x, 0.0, p.z);
            return v3(0.0, p.y < 0.0 ? -1.0 : 1.0, 0.0);
        }
        case RM_SOP_TORUS: {
            const double rho = rm_sqrt(p.x * p.x + p.z * p.z);
            const double w = (rho - src.k(ko)) / (rho > 1e-300 ? rho : 1e-300);
            return v3(p.x * w, p.y, p.z * w);
        }
        case RM_SOP_CAPSULE: {
            const vec3 a = v3(src.k(ko), src.k(ko + 1), src.k(ko + 2)), b = v3(src.k(ko + 3), src.k(ko + 4), src.k(ko + 5));
            const vec3 ab = b - a, ap = p - a;
            const double t = py_max(0.0, py_min(1.0, dot(ap, ab) / py_max(dot(ab, ab), 1e-12)));       // sd_capsule's own
            return v3(ap.x - ab.x * t, ap.y - ab.y * t, ap.z - ab.z * t);
        }
        default: return p;                // RM_SOP_SPHERE
    }
}

// is the value the leaf at `pc` pushed negated on its way to the result: the number of subtractions it reaches as their
// second operand, odd or even
template <class Src>
RM_HD bool exact_leaf_negated(const Src& src, int pc, int slot)
{
    const int n = src.nops();
    bool neg = false;
    int cs = slot;
    for (int q = pc + 1; q < n; ++q) {
        const ProgWord w{ src.word(q) };
        if (!ex_is_combinator(w.op())) continue;
        if (w.slot() == cs - 1) {
            if (w.op() == RM_SOP_SUBTRACT) neg = !neg;
            cs = cs - 1;
        }
    }
    return neg;
}

// ---- the two walks -------------------------------------------------------------------------------------------------

// The walk of a program's transforms (translate and rotate; exact_supported refuses the repeats and the mirror): the ray is
// transformed, not the solid, so every leaf stays closed-form in its own frame.  A translate moves the origin; a rotate turns
// origin and direction by the point walk's own arithmetic (rotate_plane), so t along the ray means the same in every frame.
struct ExFrame {
    vec3 p, d;
    Slots<vec3, RM_SCENE_PROGRAM_MAX_POINTS> saved, saved_d;
    RM_HD ExFrame(vec3 o, vec3 dir) : p(o), d(dir), saved(o), saved_d(dir) {}
    template <class Src>
    RM_HD void transform(const Src& src, ProgWord w)
    {
        const int ko = w.ko();
        if (w.op() == RM_SOP_POP_POINT) {
            p = saved.get(w.pslot(), p);
            d = saved_d.get(w.pslot(), d);
        } else {
            saved.set(w.pslot(), p);
            saved_d.set(w.pslot(), d);
            if (w.op() == RM_SOP_TRANSLATE) p = p - v3(src.k(ko), src.k(ko + 1), src.k(ko + 2));
            if (w.op() == RM_SOP_ROTATE) {
                if (w.axis(2)) { rotate_plane(p.x, p.y, src.k(ko + 4), src.k(ko + 5)); rotate_plane(d.x, d.y, src.k(ko + 4), src.k(ko + 5)); }
                if (w.axis(1)) { rotate_plane(p.z, p.x, src.k(ko + 2), src.k(ko + 3)); rotate_plane(d.z, d.x, src.k(ko + 2), src.k(ko + 3)); }
                if (w.axis(0)) { rotate_plane(p.y, p.z, src.k(ko), src.k(ko + 1)); rotate_plane(d.y, d.z, src.k(ko), src.k(ko + 1)); }
            }
        }
    }
    // the frame and the constants of the primitive word w
    template <class Src>
    RM_HD vec3 leaf(const Src& src, ProgWord w, int* ko) const
    {
        *ko = w.ko();
        if (!w.translated()) return p;
        *ko += 3;
        return p - v3(src.k(w.ko()), src.k(w.ko() + 1), src.k(w.ko() + 2));
    }
};

// The germ of S at t: every leaf's germ from its own roots, combined by the program.  The eight value slots are three
// bits each of one word.
template <class Src>
RM_HD uint32_t exact_germ_at(const Src& src, vec3 o, vec3 d, double t)
{
    ExFrame fr(o, d);
    uint32_t st = 0;
    const int n = src.nops();
    for (int pc = 0; pc < n; ++pc) {
        const ProgWord w{ src.word(pc) };
        const int op = w.op(), slot = w.slot();
        if (prog_is_transform(op)) {
            fr.transform(src, w);
            continue;
        }
        uint32_t g = 0;
        if (prog_is_primitive(op)) {
            int ko, last, onions;
            const vec3 q = fr.leaf(src, w, &ko);
            exact_chain(src, pc, slot, &last, &onions);
            const int combos = 1 << (onions < kExactMaxOnions ? onions : kExactMaxOnions);
            for (int combo = 0; combo < combos; ++combo) {
                double la, lb;
                exact_range(src, pc, slot, last, combo, &la, &lb);
                if (!(la <= lb)) continue;
                uint32_t gr = ex_cut_germ(exact_leaf_cut(src, op, ko, q, fr.d, lb), t);
                if (la > -__builtin_inf()) gr &= ex_cc(ex_cut_germ(exact_leaf_cut(src, op, ko, q, fr.d, la), t));
                g |= gr;
            }
        } else if (ex_is_modifier(op)) {
            continue;                     // folded into its leaf
        } else {
            const uint32_t a = (st >> (3 * slot)) & 7u, b = (st >> (3 * slot + 3)) & 7u;
            g = op == RM_SOP_UNION ? (a | b) : (op == RM_SOP_INTERSECT ? (a & b) : (a & ex_cc(b)));
        }
        st = (st & ~(7u << (3 * slot))) | (g << (3 * slot));
    }
    return st & 7u;
}

// A gradient in the frame of the leaf at word `pc`, turned into the world frame: the transposes of the rotations open at
// the leaf, innermost first.  A walk back over the words before the leaf (wave-uniform) finds them: a pop point hides the
// transform it closes.  Each plane is rotate_plane with the sine negated, the planes in the reverse of the point walk's order.
template <class Src>
RM_HD vec3 exact_frame_to_world(const Src& src, int pc, vec3 g)
{
    int closed = 0;
    for (int q = pc - 1; q >= 0; --q) {
        const ProgWord w{ src.word(q) };
        const int op = w.op();
        if (!prog_is_transform(op)) continue;
        if (op == RM_SOP_POP_POINT) {
            ++closed;
        } else if (closed > 0) {
            --closed;
        } else if (op == RM_SOP_ROTATE) {
            const int ko = w.ko();
            if (w.axis(0)) rotate_plane(g.y, g.z, src.k(ko), -src.k(ko + 1));
            if (w.axis(1)) rotate_plane(g.z, g.x, src.k(ko + 2), -src.k(ko + 3));
            if (w.axis(2)) rotate_plane(g.x, g.y, src.k(ko + 4), -src.k(ko + 5));
        }
    }
    return g;
}

struct ExactHit {
    double t;             // +inf: a miss
    vec3 normal;          // the outward unit normal of the solid; 0 on a miss
    int32_t leaf;         // index, in the program as it was given, of the op whose boundary was hit; -1 on a miss
};

template <class Src>
RM_HD ExactHit exact_first_hit(const Src& src, vec3 o, vec3 d, double t_min, double t_max)
{
    ExactHit best;
    best.t = __builtin_inf();
    best.normal = v3(0.0, 0.0, 0.0);
    best.leaf = -1;
    if (!(dot(d, d) > 0.0)) return best;
    ExFrame fr(o, d);
    const int n = src.nops();
    int fused = 0;                        // words before pc that stand for `translate, primitive, pop point`
    for (int pc = 0; pc < n; ++pc) {
        const ProgWord w{ src.word(pc) };
        const int op = w.op(), slot = w.slot();
        if (prog_is_transform(op)) {
            fr.transform(src, w);
            continue;
        }
        if (!prog_is_primitive(op)) continue;
        int ko, last, onions;
        const vec3 q = fr.leaf(src, w, &ko);
        const int index = pc + 2 * fused + (w.translated() ? 1 : 0);
        if (w.translated()) ++fused;
        exact_chain(src, pc, slot, &last, &onions);
        const int combos = 1 << (onions < kExactMaxOnions ? onions : kExactMaxOnions);
        for (int combo = 0; combo < combos; ++combo) {
            double la, lb;
            exact_range(src, pc, slot, last, combo, &la, &lb);
            if (!(la <= lb)) continue;
            for (int side = 0; side < 2; ++side) {                     // 0: the cut at lb, 1: the cut at la (the inner side)
                if (side == 1 && !(la > -__builtin_inf())) continue;
                const ExCut c = exact_leaf_cut(src, op, ko, q, fr.d, side == 0 ? lb : la);
#pragma unroll 1
                for (int j = 0; j < 4; ++j) {
                    const double t = j == 0 ? c.a0 : (j == 1 ? c.b0 : (j == 2 ? c.a1 : c.b1));
                    if (!(t > t_min && t <= t_max && t < best.t)) continue;        // (an infinite or missing end too)
                    if (!ex_boundary(exact_germ_at(src, o, d, t))) continue;
                    best.t = t;
                    best.leaf = index;
                    const vec3 g = exact_frame_to_world(
                        src, pc, exact_leaf_gradient(src, op, ko, v3(q.x + t * fr.d.x, q.y + t * fr.d.y, q.z + t * fr.d.z)));
                    const double len = rm_sqrt((g.x * g.x + g.y * g.y) + g.z * g.z);
                    const double inv = ((side == 1) != exact_leaf_negated(src, pc, slot) ? -1.0 : 1.0) / (len > 1e-300 ? len : 1e-300);
                    best.normal = v3(g.x * inv, g.y * inv, g.z * inv);
                }
            }
        }
    }
    return best;
}

// The march's constants after defaults.
struct ExactParams {
    double t_min, t_max;
};

// One pixel of exact_capture: the library's camera ray (rm_camera.h).  A miss has depth 0, hit 0, normal 0, leaf -1.
template <class Src>
RM_HD void exact_pixel(const Src& src, const CameraParams& cam, int width, int height, int px, int py, const ExactParams& P,
                       double* depth, uint8_t* hit, vec3* normal, int32_t* leaf)
{
    vec3 o, d;
    camera_ray(cam, width, height, px, py, o, d);
    const ExactHit h = exact_first_hit(src, o, d, P.t_min, P.t_max);
    const bool ok = h.t < __builtin_inf();
    *depth = ok ? h.t : 0.0;
    *hit = ok ? 1 : 0;
    *normal = h.normal;
    *leaf = h.leaf;
}

// (host code) RmExactConfig -> ExactParams: t_min 0 is 1e-6, t_max 0 is no limit.  false with the reason in `why` for a
// negative or NaN field or reserved != 0.
inline bool exact_resolve(const RmExactConfig* c, ExactParams* P, char* why, size_t why_len)
{
    RmExactConfig z;
    memset(&z, 0, sizeof z);
    if (!c) c = &z;
    if (!(c->t_min >= 0.0)) return snprintf(why, why_len, "t_min is negative or NaN"), false;
    if (!(c->t_max >= 0.0)) return snprintf(why, why_len, "t_max is negative or NaN"), false;
    if (c->reserved[0] != 0 || c->reserved[1] != 0) return snprintf(why, why_len, "reserved must be 0"), false;
    P->t_min = c->t_min != 0.0 ? c->t_min : 1e-6;
    P->t_max = c->t_max != 0.0 ? c->t_max : __builtin_inf();
    return true;
}

// (host code) Does the encoded program have an exact form here?  false with the reason in `why`: a smooth combinator, a
// repeat (needs a cell traversal), a mirror (it folds the ray), a primitive without a closed form (cone, capped torus, Menger cross, gyroid), a
// modifier over a box or a cylinder (cut at level 0 only) or over a combinator's result, more than kExactMaxOnions onions
// over one leaf, a torus cut at a level where its tube closes the hole (minor radius + level >= major radius: the quartic
// then has roots that are not on the surface).  Op numbers are those of the encoded image.
inline bool exact_supported(const ProgramImage& img, char* why, size_t why_len)
{
    struct HostSrc {
        const ProgramImage* img;
        int nops() const { return img->nops; }
        uint32_t word(int i) const { return img->code[i]; }
        double k(int i) const { return img->k[i]; }
    } src{ &img };
    int kind[RM_SCENE_PROGRAM_MAX_VALUES];          // per value slot: the primitive that pushed it, -1 after a combinator
    for (int i = 0; i < RM_SCENE_PROGRAM_MAX_VALUES; ++i) kind[i] = -1;
    for (int pc = 0; pc < img.nops; ++pc) {
        const ProgWord w{ img.code[pc] };
        const int op = w.op(), slot = w.slot();
        switch (op) {
            case RM_SOP_SMOOTH_UNION: case RM_SOP_SMOOTH_SUBTRACT: case RM_SOP_SMOOTH_INTERSECT:
                return snprintf(why, why_len, "op %d: a smooth combinator has no exact form", pc), false;
            case RM_SOP_REPEAT: case RM_SOP_LIMITED_REPEAT:
                return snprintf(why, why_len, "op %d: a repeat needs a cell traversal", pc), false;
            case RM_SOP_CONE: return snprintf(why, why_len, "op %d: sd_cone has no exact form", pc), false;
            case RM_SOP_CAPPED_TORUS: return snprintf(why, why_len, "op %d: sd_capped_torus has no exact form", pc), false;
            case RM_SOP_MENGER_CROSS: return snprintf(why, why_len, "op %d: sd_menger_cross has no exact form", pc), false;
            case RM_SOP_GYROID: return snprintf(why, why_len, "op %d: sd_gyroid has no exact form", pc), false;
            case RM_SOP_UNION: case RM_SOP_SUBTRACT: case RM_SOP_INTERSECT:
                if (slot >= 0 && slot < RM_SCENE_PROGRAM_MAX_VALUES) kind[slot] = -1;
                break;
            case RM_SOP_ROUND: case RM_SOP_ONION: case RM_SOP_SCALE: {
                const int kd = slot >= 0 && slot < RM_SCENE_PROGRAM_MAX_VALUES ? kind[slot] : -1;
                const char* name = op == RM_SOP_ROUND ? "op_round" : (op == RM_SOP_ONION ? "op_onion" : "op_scale");
                if (kd == RM_SOP_BOX || kd == RM_SOP_CYLINDER)
                    return snprintf(why, why_len, "op %d: %s over a %s, which is cut at level 0 only", pc, name,
                                    kd == RM_SOP_BOX ? "box" : "cylinder"), false;
                if (kd < 0) return snprintf(why, why_len, "op %d: %s over a combinator's result", pc, name), false;
                break;
            }
            case RM_SOP_MIRROR:
                return snprintf(why, why_len, "op %d: a mirror folds the ray (its image is no single ray)", pc), false;
            case RM_SOP_TRANSLATE: case RM_SOP_ROTATE: case RM_SOP_POP_POINT: break;
            default:                      // sphere, box, plane, cylinder, torus, capsule
                if (slot >= 0 && slot < RM_SCENE_PROGRAM_MAX_VALUES) kind[slot] = op;
                int last, onions;
                exact_chain(src, pc, slot, &last, &onions);
                if (onions > kExactMaxOnions)
                    return snprintf(why, why_len, "op %d: more than %d onions over one leaf", pc, kExactMaxOnions), false;
                if (op == RM_SOP_TORUS) {
                    const int ko = w.ko() + (w.translated() ? 3 : 0);
                    for (int combo = 0; combo < (1 << onions); ++combo) {
                        double la, lb;
                        exact_range(src, pc, slot, last, combo, &la, &lb);
                        if (la <= lb && !(img.k[ko + 1] + lb < img.k[ko]))
                            return snprintf(why, why_len, "op %d: the torus is cut where its tube closes the hole", pc), false;
                    }
                }
                break;
        }
    }
    return true;
}

}  // namespace rm
