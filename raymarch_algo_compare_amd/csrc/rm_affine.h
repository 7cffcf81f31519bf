// rm_affine.h -- revised affine arithmetic over scene programs: the third sound range of a scene over a ray segment, and
// the forward march of the reference's gpu/affine.py (AAForm, _aff_positions, _affine_range, march_count, _capture).
//
// A quantity over the segment tau in [t0, t1] is tracked as x0 + x1 * eps + e * [-1, 1]: eps in [-1, 1] is the one noise
// symbol, shared by every quantity, of the march parameter (tau = c + r * eps), and e >= 0 collects everything that is not
// linear in eps.  Sums and the linear part of products keep the dependence on tau that an interval throws away; that is
// where the range is tighter than rm_interval.h's.  Aff restates gpu/affine.py's AAForm op for op in binary64 without
// contraction and without re-association (Python's `a * b * c` is `(a * b) * c`).  AffineAlgebra extends every RM_SOP_*
// of the scene-program interpreter:
//  * sphere, plane, box, torus: the reference's _sd_sphere / _sd_plane / _sd_box / _sd_torus over Aff, expression for
//    expression -- its COMPONENT_SCENES, bit for bit in x0, x1 and e;
//  * translate and round: x0 - k, exact and linear, x1 and e untouched; scale: every part times the factor; a limited
//    repeat whose range lies in one cell: the shift by that cell;
//  * every other primitive and op: the hull fallback -- the operands' range(), the interval function of rm_interval.h on
//    those intervals, aff_from_range of the result.  This is what the reference does for its own non-smooth ops (abs,
//    max0, min0, maximum, minimum); it is sound because the interval function is, and it drops the correlation.
// DESIGN.md section 3, "Affine range", has the per-op notes and the argument for the meet of the two ranges.
// Rounding is to nearest, as in the reference: the enclosure is exact in real arithmetic only.
#pragma once

#include "rm_interval.h"

namespace rm {

constexpr double kAffEps = 1e-12;      // _EPS, and the threshold of sqrt's `wide`

struct Aff {
    double x0, x1, e;      // centre, coefficient of the march symbol, remainder radius (>= 0)
};
RM_HD Aff aff(double x0, double x1, double e)
{
    Aff r;
    r.x0 = x0; r.x1 = x1; r.e = e;
    return r;
}

// ---- gpu/affine.py: AAForm ---------------------------------------------------------------------------------------------
RM_HD Ival arange(Aff a)
{
    const double rad = rm_fabs(a.x1) + a.e;
    return iv(a.x0 - rad, a.x0 + rad);
}
// the linear ops: exact, the correlation is kept
RM_HD Aff operator+(Aff a, Aff b) { return aff(a.x0 + b.x0, a.x1 + b.x1, a.e + b.e); }
RM_HD Aff operator+(Aff a, double s) { return aff(a.x0 + s, a.x1, a.e); }
RM_HD Aff operator+(double s, Aff a) { return a + s; }                                     // __radd__
RM_HD Aff operator-(Aff a, Aff b) { return aff(a.x0 - b.x0, a.x1 - b.x1, a.e + b.e); }
RM_HD Aff operator-(Aff a, double s) { return aff(a.x0 - s, a.x1, a.e); }
RM_HD Aff operator-(double s, Aff a) { return aff(s - a.x0, -a.x1, a.e); }                 // __rsub__
RM_HD Aff operator-(Aff a) { return aff(-a.x0, -a.x1, a.e); }
// the product: the linear part exact, every cross term and the eps^2 term bounded into e
RM_HD Aff operator*(Aff a, Aff b)
{
    const double e = rm_fabs(a.x1) * b.e + rm_fabs(b.x1) * a.e + a.e * b.e + rm_fabs(a.x1 * b.x1);
    return aff(a.x0 * b.x0, a.x0 * b.x1 + a.x1 * b.x0, e);
}
RM_HD Aff operator*(Aff a, double s) { return aff(a.x0 * s, a.x1 * s, a.e * rm_fabs(s)); }
RM_HD Aff operator*(double s, Aff a) { return a * s; }                                     // __rmul__
// x^2 = x0^2 + 2 x0 x1 eps + x1^2 eps^2 + (terms in e); eps^2 in [0, 1] is x1^2 / 2 +- x1^2 / 2
RM_HD Aff asquare(Aff a)
{
    const double half = 0.5 * a.x1 * a.x1;
    return aff(a.x0 * a.x0 + half, 2.0 * a.x0 * a.x1, half + 2.0 * (rm_fabs(a.x0) + rm_fabs(a.x1)) * a.e + a.e * a.e);
}
// the minimax (Chebyshev) affine approximation alpha * x + zeta +- delta of the square root over the form's range
// clamped to [a, b] >= 0: alpha is the chord's slope (the tangent's at a where the range is no wider than 1e-12), the
// tangent point u = 1 / (4 alpha^2) is clipped into [a, b], r is the gap between curve and chord there
RM_HD Aff asqrt(Aff x)
{
    const Ival g = arange(x);
    const double a = np_max(g.lo, 0.0), b = np_max(g.hi, 0.0);
    const double sa = rm_sqrt(a), sb = rm_sqrt(b);
    const bool wide = (b - a) > 1e-12;
    const double alpha = wide ? (sb - sa) / (b - a) : 0.5 / rm_sqrt(np_max(a, kAffEps));
    double u = 1.0 / (4.0 * np_max(alpha * alpha, kAffEps));
    u = np_min(np_max(u, a), b);                                                           // np.clip
    const double zeta_chord = sa - alpha * a;
    const double r = np_max(rm_sqrt(u) - (alpha * u + zeta_chord), 0.0);
    const double zeta = zeta_chord + 0.5 * r;
    const double delta = 0.5 * r;
    return aff(alpha * x.x0 + zeta, alpha * x.x1, rm_fabs(alpha) * x.e + delta);
}
// _from_range: the form of an interval -- a fresh remainder, no dependence on the march symbol
RM_HD Aff aff_from_range(Ival r) { return aff(0.5 * (r.lo + r.hi), 0.0, 0.5 * (r.hi - r.lo)); }
// the non-smooth ops: the interval op (rm_interval.h's Ival functions are gpu/affine.py's expressions) on the range(s)
RM_HD Aff aabs(Aff a) { return aff_from_range(iabs(arange(a))); }
RM_HD Aff amax0(Aff a) { return aff_from_range(imax0(arange(a))); }
RM_HD Aff amin0(Aff a) { return aff_from_range(imin0(arange(a))); }
RM_HD Aff amaximum(Aff a, Aff b) { return aff_from_range(imaximum(arange(a), arange(b))); }
RM_HD Aff aminimum(Aff a, Aff b) { return aff_from_range(iminimum(arange(a), arange(b))); }

struct AVec3 {
    Aff x, y, z;
};
RM_HD AVec3 avec3(Aff x, Aff y, Aff z)
{
    AVec3 r;
    r.x = x; r.y = y; r.z = z;
    return r;
}
RM_HD IVec3 aranges(AVec3 p) { return ivec3(arange(p.x), arange(p.y), arange(p.z)); }
RM_HD Aff alength3(Aff x, Aff y, Aff z) { return asqrt(asquare(x) + asquare(y) + asquare(z)); }      // _length3

// _aff_positions: the point o + d * tau over tau = c + r * eps, c and r the midpoint and half-width of [t0, t1]
RM_HD AVec3 aff_seed_segment(vec3 o, vec3 d, double t0, double t1)
{
    const double c = 0.5 * (t0 + t1), r = 0.5 * (t1 - t0);
    return avec3(aff(o.x + d.x * c, d.x * r, 0.0), aff(o.y + d.y * c, d.y * r, 0.0), aff(o.z + d.z * c, d.z * r, 0.0));
}

// ---- gpu/interval.py: the metric primitives over component objects -----------------------------------------------------
RM_HD Aff a_sphere(AVec3 p, double radius) { return alength3(p.x, p.y, p.z) - radius; }
RM_HD Aff a_plane(AVec3 p, double n0, double n1, double n2, double offset) { return p.x * n0 + p.y * n1 + p.z * n2 - offset; }
RM_HD Aff a_box(AVec3 p, double h0, double h1, double h2)
{
    const Aff qx = aabs(p.x) - h0, qy = aabs(p.y) - h1, qz = aabs(p.z) - h2;
    const Aff outside = alength3(amax0(qx), amax0(qy), amax0(qz));
    const Aff inside = amin0(amaximum(amaximum(qx, qy), qz));
    return outside + inside;
}
RM_HD Aff a_torus(AVec3 p, double major_radius, double minor_radius)
{
    const Aff q_xz = asqrt(asquare(p.x) + asquare(p.z)) - major_radius;
    return asqrt(asquare(q_xz) + asquare(p.y)) - minor_radius;
}

// ---- the interpreter ----------------------------------------------------------------------------------------------

// evaluation over the affine point of a ray segment (program_walk, rm_scene_program.h).  Everything below the four
// component formulas and the two exact shifts is the hull fallback through rm_interval.h.
struct AffineAlgebra {
    typedef Aff Value;
    typedef AVec3 Point;
    RM_HD Aff sphere(AVec3 p, double r) const { return a_sphere(p, r); }
    RM_HD Aff box(AVec3 p, double h0, double h1, double h2) const { return a_box(p, h0, h1, h2); }
    RM_HD Aff plane(AVec3 p, double n0, double n1, double n2, double offset) const { return a_plane(p, n0, n1, n2, offset); }
    RM_HD Aff torus(AVec3 p, double major_radius, double minor_radius) const { return a_torus(p, major_radius, minor_radius); }
    RM_HD Aff cylinder(AVec3 p, double radius, double half_height) const { return aff_from_range(i_cylinder(aranges(p), radius, half_height)); }
    RM_HD Aff capsule(AVec3 p, vec3 a, vec3 b, double radius) const { return aff_from_range(i_capsule(aranges(p), a, b, radius)); }
    RM_HD Aff capped_torus(AVec3 p, double sc0, double sc1, double ra, double rb) const
    {
        return aff_from_range(i_capped_torus(aranges(p), sc0, sc1, ra, rb));
    }
    RM_HD Aff cone(AVec3 p, double c, double s, double height) const { return aff_from_range(i_cone(aranges(p), c, s, height)); }
    RM_HD AVec3 translate(AVec3 p, double kx, double ky, double kz) const { return avec3(p.x - kx, p.y - ky, p.z - kz); }
    RM_HD Aff repeat(Aff x, double spacing, bool pow2) const { return aff_from_range(irepeat_axis(arange(x), spacing, pow2)); }
    // same cell at both ends of the range: the exact shift x - c * n, the linear part kept; else the interval fallback
    RM_HD Aff limited_repeat(Aff x, double c, double l) const
    {
        const Ival r = arange(x);
        const double n = limited_repeat_cell(r.lo, c, l);
        if (n == limited_repeat_cell(r.hi, c, l)) return x - c * n;
        return aff_from_range(ilimited_repeat_axis(r, c, l));
    }
    // RM_SOP_ROTATE is linear: both coordinates keep their dependence on the march symbol and no remainder appears (along a
    // ray e stays 0 -- the rotated segment is still a segment, where the interval walk boxes it anew).  RM_SOP_MIRROR: the
    // identity or the negation where the range keeps one sign, else the interval fallback.
    RM_HD Aff lincomb(Aff a, double ca, Aff b, double cb) const { return a * ca + b * cb; }
    RM_HD Aff mirror(Aff x) const
    {
        const Ival r = arange(x);
        if (r.lo >= 0.0) return x;
        if (r.hi <= 0.0) return -x;
        return aff_from_range(iabs_pw(r));
    }
    RM_HD Aff menger_cross(AVec3 p, double s, double s3) const { return aff_from_range(i_menger_cross(aranges(p), s, s3)); }
    RM_HD Aff gyroid(AVec3 p, double freq, double lipschitz) const { return aff_from_range(i_gyroid(aranges(p), freq, lipschitz)); }
    RM_HD Aff round(Aff a, double k) const { return a - k; }
    RM_HD Aff scale(Aff a, double k) const { return a * k; }
    RM_HD Aff abs(Aff a) const { return aff_from_range(iabs_pw(arange(a))); }
    RM_HD Aff union_(Aff a, Aff b) const { return aff_from_range(i_union(arange(a), arange(b))); }
    RM_HD Aff subtract(Aff a, Aff b) const { return aff_from_range(i_subtract(arange(a), arange(b))); }
    RM_HD Aff intersect(Aff a, Aff b) const { return aff_from_range(i_intersect(arange(a), arange(b))); }
    RM_HD Aff smooth_union(Aff a, Aff b, double k) const { return aff_from_range(i_smooth_union(arange(a), arange(b), k)); }
    RM_HD Aff smooth_subtract(Aff a, Aff b, double k) const { return aff_from_range(i_smooth_subtract(arange(a), arange(b), k)); }
    RM_HD Aff smooth_intersect(Aff a, Aff b, double k) const { return aff_from_range(i_smooth_intersect(arange(a), arange(b), k)); }
};

// The affine form of the program's value over the affine point p (same image, words and constants as program_eval).
template <class Src>
RM_HD Aff program_eval_affine(const Src& src, AVec3 p)
{
    return program_walk(AffineAlgebra{}, src, p);
}

// The range of the program over the segment o + d * [t0, t1] in `mode`:
//  * RM_RANGE_AFFINE: _affine_range, the range() of the affine form (which `form` receives when it is not NULL);
//  * RM_RANGE_MEET: the intersection of that range with program_eval_interval over seed_segment of the same segment.
//    Both enclose the program's values on the segment, so their intersection does; per probe it is at least as tight
//    as either.  Only the two final results meet: one more walk per probe.
template <class Src>
RM_HD Ival affine_range(const Src& src, int mode, vec3 o, vec3 d, double t0, double t1, Aff* form = nullptr)
{
    const Aff f = program_eval_affine(src, aff_seed_segment(o, d, t0, t1));
    if (form) *form = f;
    Ival r = arange(f);
    if (mode == RM_RANGE_MEET) {
        const Ival i = program_eval_interval(src, seed_segment(o, d, t0, t1));
        r = iv(np_max(r.lo, i.lo), np_min(r.hi, i.hi));
    }
    return r;
}

// ---- gpu/affine.py: march_count and _capture ---------------------------------------------------------------------------

// march_count for one ray: the interval oracle's loop (sound_first_hit, rm_interval.h) with the range of `mode`.
// `steps` is the ray's share of the reference's eval count.
template <class Src>
RM_HD double affine_first_hit(const Src& src, int mode, vec3 o, vec3 d, const IntervalParams& P, int32_t* steps)
{
    return sound_first_hit([&](double t, double t1) { return affine_range(src, mode, o, d, t, t1); }, P, steps);
}

// One pixel of _capture: the library's camera ray (rm_camera.h), _prune_candidates, the march.  A pruned ray or a miss has
// depth 0 and hit 0; a pruned ray has 0 steps.
template <class Src>
RM_HD void affine_pixel(const Src& src, int mode, const CameraParams& cam, int width, int height, int px, int py,
                        const IntervalParams& P, double* depth, uint8_t* hit, int32_t* steps)
{
    vec3 o, d;
    camera_ray(cam, width, height, px, py, o, d);
    double t = __builtin_inf();
    int32_t s = 0;
    if (interval_candidate(o, d, P.bound)) t = affine_first_hit(src, mode, o, d, P, &s);
    const bool h = t < __builtin_inf();
    *depth = h ? t : 0.0;
    *hit = h ? 1 : 0;
    *steps = s;
}

// (host code) the mode argument of the rm_affine_* calls
inline bool affine_mode_ok(int mode) { return mode == RM_RANGE_AFFINE || mode == RM_RANGE_MEET; }

}  // namespace rm
