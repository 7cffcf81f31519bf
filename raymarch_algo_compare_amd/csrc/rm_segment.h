// rm_segment.h -- the sound segment tracer: dual intervals (value enclosure + enclosure of the derivative along the ray)
// over scene programs, and the Galin-style march of the reference's gpu/interval_autodiff.py and gpu/faithful_offline.py
// (seed_segment, DInterval, segment_trace, faithful_capture).
//
// DIval restates gpu/interval_autodiff.py's DInterval op for op in binary64 without contraction, on top of Ival
// (rm_interval.h): the `val` half of every operation IS the Ival operation, so a dual evaluation carries the interval
// oracle's enclosure bit for bit.  program_eval_dual extends every RM_SOP_* of the interpreter to a dual interval:
//  * sphere, plane, box, torus: the reference's _sd_sphere / _sd_plane / _sd_box / _sd_torus pushed through DIval,
//    expression for expression -- its COMPONENT_SCENES, bit for bit in val and der;
//  * every other op: `val` is the interval extension of rm_interval.h itself (i_cylinder, i_capsule, ... are called, not
//    restated), `der` is the chain rule through the pointwise formula.  DESIGN.md section 3, "Segment ceiling", gives the
//    soundness argument of each rule.
// The walk's point is a dual point (DVec3): every coordinate carries the enclosure of its own d/dtau, seeded once with the ray's
// direction rd_c as a degenerate interval.  A translated, repeated or limited-repeated coordinate keeps its derivative
// (wherever it is differentiable); RM_SOP_ROTATE combines the derivatives as it combines the values, RM_SOP_MIRROR is the
// dual abs.  In a program without those two every der stays the degenerate [rd_c, rd_c], and the arithmetic on it is the
// arithmetic the constant direction had.  Rounding is to nearest, as in the reference.
#pragma once

#include "rm_interval.h"

namespace rm {

constexpr double kSegBig = 1.0e12;     // _BIG
constexpr double kSegEps = 1e-15;      // _EPS

struct DIval {
    Ival val, der;
};
RM_HD DIval dv(Ival val, Ival der)
{
    DIval r;
    r.val = val; r.der = der;
    return r;
}

// ---- gpu/interval_autodiff.py: DInterval ------------------------------------------------------------------------------
RM_HD DIval operator+(DIval a, DIval b) { return dv(a.val + b.val, a.der + b.der); }
RM_HD DIval operator+(DIval a, double s) { return dv(a.val + s, a.der); }
RM_HD DIval operator-(DIval a, DIval b) { return dv(a.val - b.val, a.der - b.der); }
RM_HD DIval operator-(DIval a, double s) { return dv(a.val - s, a.der); }
RM_HD DIval operator-(DIval a) { return dv(-a.val, -a.der); }
RM_HD DIval operator*(DIval a, DIval b) { return dv(a.val * b.val, a.der * b.val + a.val * b.der); }     // product rule
RM_HD DIval operator*(DIval a, double s) { return dv(a.val * s, a.der * s); }
RM_HD Ival seg_hull(Ival a, Ival b) { return iv(np_min(a.lo, b.lo), np_max(a.hi, b.hi)); }                // _hull
// _recip_pos: the reciprocal of a non-negative interval (a square root), capped at _BIG near 0
RM_HD Ival recip_pos(Ival s)
{
    const double a = np_max(s.lo, 0.0), b = np_max(s.hi, 0.0);
    return iv(b > kSegEps ? 1.0 / b : kSegBig, a > kSegEps ? 1.0 / a : kSegBig);
}
RM_HD DIval dsquare(DIval a) { return dv(isquare(a.val), (a.val * a.der) * 2.0); }
// the derivative of a square root whose value enclosure is s: v' / (2 sqrt(v))
RM_HD Ival root_der(Ival der, Ival s) { return der * recip_pos(s) * 0.5; }
RM_HD DIval dsqrt(DIval a)
{
    const Ival s = isqrt(a.val);
    return dv(s, root_der(a.der, s));
}
// DInterval.abs's der: der where val >= 0, -der where val <= 0, [-m, m] across 0
RM_HD Ival abs_der(Ival val, Ival der)
{
    const double m = np_max(rm_fabs(der.lo), rm_fabs(der.hi));
    return iv(val.lo >= 0.0 ? der.lo : (val.hi <= 0.0 ? -der.hi : -m), val.lo >= 0.0 ? der.hi : (val.hi <= 0.0 ? -der.lo : m));
}
RM_HD DIval dabs(DIval a) { return dv(iabs(a.val), abs_der(a.val, a.der)); }
// _clamp_der: der where the clamp is inactive, 0 where it holds, the hull with 0 where the segment leaves it open
RM_HD Ival clamp_der(Ival der, bool active, bool zero)
{
    return iv(active ? der.lo : (zero ? 0.0 : np_min(der.lo, 0.0)), active ? der.hi : (zero ? 0.0 : np_max(der.hi, 0.0)));
}
RM_HD DIval dmax0(DIval a) { return dv(imax0(a.val), clamp_der(a.der, a.val.lo > 0.0, a.val.hi < 0.0)); }
RM_HD DIval dmin0(DIval a) { return dv(imin0(a.val), clamp_der(a.der, a.val.hi < 0.0, a.val.lo > 0.0)); }
// the der of a maximum / minimum: the decided side's, else the hull of both
RM_HD Ival pick_der(bool a_wins, bool b_wins, Ival a, Ival b)
{
    const Ival h = seg_hull(a, b);
    return iv(a_wins ? a.lo : (b_wins ? b.lo : h.lo), a_wins ? a.hi : (b_wins ? b.hi : h.hi));
}
RM_HD Ival max_der(DIval a, DIval b) { return pick_der(a.val.lo > b.val.hi, b.val.lo > a.val.hi, a.der, b.der); }
RM_HD Ival min_der(DIval a, DIval b) { return pick_der(a.val.hi < b.val.lo, b.val.hi < a.val.lo, a.der, b.der); }
RM_HD DIval dmaximum(DIval a, DIval b) { return dv(imaximum(a.val, b.val), max_der(a, b)); }
RM_HD DIval dminimum(DIval a, DIval b) { return dv(iminimum(a.val, b.val), min_der(a, b)); }

struct DVec3 {
    DIval x, y, z;
};
// the dual point of a box on the ray: d(ro_c + rd_c tau)/dtau = rd_c
RM_HD DVec3 dvec3(IVec3 p, vec3 rd)
{
    DVec3 r;
    r.x = dv(p.x, iv(rd.x, rd.x)); r.y = dv(p.y, iv(rd.y, rd.y)); r.z = dv(p.z, iv(rd.z, rd.z));
    return r;
}
RM_HD IVec3 dvals(DVec3 p) { return ivec3(p.x.val, p.y.val, p.z.val); }
RM_HD DIval dlength3(DIval x, DIval y, DIval z) { return dsqrt(dsquare(x) + dsquare(y) + dsquare(z)); }     // _length3

// ---- gpu/interval.py: the metric primitives over component objects -----------------------------------------------------
RM_HD DIval d_sphere(DVec3 p, double radius) { return dlength3(p.x, p.y, p.z) - radius; }
RM_HD DIval d_plane(DVec3 p, double n0, double n1, double n2, double offset) { return p.x * n0 + p.y * n1 + p.z * n2 - offset; }
RM_HD DIval d_box(DVec3 p, double h0, double h1, double h2)
{
    const DIval qx = dabs(p.x) - h0, qy = dabs(p.y) - h1, qz = dabs(p.z) - h2;
    const DIval outside = dlength3(dmax0(qx), dmax0(qy), dmax0(qz));
    const DIval inside = dmin0(dmaximum(dmaximum(qx, qy), qz));
    return outside + inside;
}
RM_HD DIval d_torus(DVec3 p, double major_radius, double minor_radius)
{
    const DIval q_xz = dsqrt(dsquare(p.x) + dsquare(p.z)) - major_radius;
    return dsqrt(dsquare(q_xz) + dsquare(p.y)) - minor_radius;
}

// ---- the other ops: val from rm_interval.h, der by the chain rule ("Segment ceiling") -------------
// pow_half differentiates like sqrt; iabs_pw like abs
RM_HD DIval dpow_half(DIval a)
{
    const Ival s = ipow_half(a.val);
    return dv(s, root_der(a.der, s));
}
RM_HD DIval dabs_pw(DIval a) { return dv(iabs_pw(a.val), abs_der(a.val, a.der)); }

RM_HD DIval d_cylinder(DVec3 p, double radius, double half_height)
{
    const DIval d_radial = dpow_half(dsquare(p.x) + dsquare(p.z)) - radius;
    const DIval d_height = dabs_pw(p.y) - half_height;
    const DIval outside = dpow_half(dsquare(dmax0(d_radial)) + dsquare(dmax0(d_height)));
    const DIval inside = dmin0(dmaximum(d_radial, d_height));
    return dv(i_cylinder(dvals(p), radius, half_height), outside.der + inside.der);
}

RM_HD DIval d_capsule(DVec3 p, vec3 a, vec3 b, double radius)
{
    const vec3 ab = b - a;
    const DIval apx = p.x - a.x, apy = p.y - a.y, apz = p.z - a.z;
    const double den = py_max(dot(ab, ab), 1e-12);
    const DIval num = apx * ab.x + apy * ab.y + apz * ab.z;
    // t = clamp(num / den, 0, 1): den > 0, so the quotient's der is num.der / den end for end; clamped like max0 / min0
    const double ql = num.val.lo / den, qh = num.val.hi / den;
    const Ival tder = clamp_der(iv(num.der.lo / den, num.der.hi / den), ql > 0.0 && qh < 1.0, qh < 0.0 || ql > 1.0);
    const DIval t = dv(iv(py_max(0.0, py_min(1.0, ql)), py_max(0.0, py_min(1.0, qh))), tder);
    const DIval dx = p.x - (t * ab.x + a.x), dy = p.y - (t * ab.y + a.y), dz = p.z - (t * ab.z + a.z);
    const DIval r = dpow_half(dsquare(dx) + dsquare(dy) + dsquare(dz));
    return dv(i_capsule(dvals(p), a, b, radius), r.der);
}

RM_HD DIval d_capped_torus(DVec3 p, double sc0, double sc1, double ra, double rb)
{
    const DIval px = dabs_pw(p.x);
    const Ival ca = px.val * sc1, cb = p.y.val * sc0;
    const DIval k1 = px * sc0 + p.y * sc1;
    const DIval k2 = dpow_half(dsquare(px) + dsquare(p.y));
    // the branch of i_capped_torus: the decided side's der, the hull of both where the box leaves it open
    DIval k;
    if (ca.lo > cb.hi) k = k1;
    else if (!(ca.hi > cb.lo)) k = k2;
    else k = dv(ihull(k1.val, k2.val), seg_hull(k1.der, k2.der));
    const DIval inner = dsquare(p.x) + dsquare(p.y) + dsquare(p.z) + ra * ra - k * (2.0 * ra);
    return dv(i_capped_torus(dvals(p), sc0, sc1, ra, rb), dpow_half(inner).der);
}

RM_HD DIval d_cone(DVec3 p, double c, double s, double height)
{
    const DIval q_len = dpow_half(dsquare(p.x) + dsquare(p.z));
    const DIval d1 = p.y - (-height);
    const DIval d2 = q_len * c + p.y * s;
    return dv(i_cone(dvals(p), c, s, height), max_der(-d1, d2));
}

// RM_SOP_MENGER_CROSS: a is x * s up to jumps that |a| does not see, so d|a|/dtau follows from a's enclosure and the
// exact slope s * rd_c; where the box may span a jump a's enclosure is [-1, 1], which spans 0, and abs_der gives the whole
// of +-s |rd_c|.  The rest is abs, max and min: the decided branch's slope, else the hull.
RM_HD DIval dmenger_fold(DIval x, double s)
{
    const DIval b = dabs_pw(dv(imenger_a(x.val, s), x.der * s));       // (x.der is rd_c unless a rotate or mirror came before)
    return dabs_pw(dv(iv(1.0 - 3.0 * b.val.hi, 1.0 - 3.0 * b.val.lo), -(b.der * 3.0)));
}
RM_HD DIval d_menger_cross(DVec3 p, double s, double s3)
{
    const DIval rx = dmenger_fold(p.x, s), ry = dmenger_fold(p.y, s), rz = dmenger_fold(p.z, s);
    const DIval da = dv(i_intersect(rx.val, ry.val), max_der(rx, ry));
    const DIval db = dv(i_intersect(ry.val, rz.val), max_der(ry, rz));
    const DIval dc = dv(i_intersect(rz.val, rx.val), max_der(rz, rx));
    const DIval dbc = dv(i_union(db.val, dc.val), min_der(db, dc));
    const Ival der = min_der(da, dbc);
    return dv(i_menger_cross(dvals(p), s, s3), iv(der.lo / s3, der.hi / s3));
}

// RM_SOP_GYROID: (sin q)' = cos q * q', (cos q)' = -sin q * q' with q' = freq * rd_c, by the same interval sin / cos; the
// products and sums are DIval's, whose val half is the Ival operation i_gyroid performs.
RM_HD DIval d_gyroid(DVec3 p, double freq, double lipschitz)
{
    const ISinCos3 sc = isincos3(dvals(p), freq);
    const ISinCos x = sc.x, y = sc.y, z = sc.z;
    const Ival qx = p.x.der * freq, qy = p.y.der * freq, qz = p.z.der * freq;
    const DIval sx = dv(x.s, x.c * qx), cx = dv(x.c, -(x.s * qx));
    const DIval sy = dv(y.s, y.c * qy), cy = dv(y.c, -(y.s * qy));
    const DIval sz = dv(z.s, z.c * qz), cz = dv(z.c, -(z.s * qz));
    const DIval g = sx * cy + sy * cz + sz * cx;
    return dv(iv(g.val.lo / lipschitz, g.val.hi / lipschitz), iv(g.der.lo / lipschitz, g.der.hi / lipschitz));
}

// ---- the interpreter ----------------------------------------------------------------------------------------------

// evaluation over the dual point of a ray segment (program_walk, rm_scene_program.h): val is the interval walk's, operation for
// operation.  A smooth combinator's partial derivatives are h and 1 - h (h in [0, 1]) up to the signs of its arguments: the
// hull of the two ders.
struct DualAlgebra {
    typedef DIval Value;
    typedef DVec3 Point;
    RM_HD DIval sphere(DVec3 p, double r) const { return d_sphere(p, r); }
    RM_HD DIval box(DVec3 p, double h0, double h1, double h2) const { return d_box(p, h0, h1, h2); }
    RM_HD DIval plane(DVec3 p, double n0, double n1, double n2, double offset) const { return d_plane(p, n0, n1, n2, offset); }
    RM_HD DIval cylinder(DVec3 p, double radius, double half_height) const { return d_cylinder(p, radius, half_height); }
    RM_HD DIval torus(DVec3 p, double major_radius, double minor_radius) const { return d_torus(p, major_radius, minor_radius); }
    RM_HD DIval capsule(DVec3 p, vec3 a, vec3 b, double radius) const { return d_capsule(p, a, b, radius); }
    RM_HD DIval capped_torus(DVec3 p, double sc0, double sc1, double ra, double rb) const { return d_capped_torus(p, sc0, sc1, ra, rb); }
    RM_HD DIval cone(DVec3 p, double c, double s, double height) const { return d_cone(p, c, s, height); }
    RM_HD DIval menger_cross(DVec3 p, double s, double s3) const { return d_menger_cross(p, s, s3); }
    RM_HD DIval gyroid(DVec3 p, double freq, double lipschitz) const { return d_gyroid(p, freq, lipschitz); }
    RM_HD DVec3 translate(DVec3 p, double kx, double ky, double kz) const
    {
        p.x = p.x - kx; p.y = p.y - ky; p.z = p.z - kz;
        return p;
    }
    // piecewise a shift: the derivative is the coordinate's own wherever the map is differentiable
    RM_HD DIval repeat(DIval x, double spacing, bool pow2) const { return dv(irepeat_axis(x.val, spacing, pow2), x.der); }
    RM_HD DIval limited_repeat(DIval x, double spacing, double limit) const { return dv(ilimited_repeat_axis(x.val, spacing, limit), x.der); }
    RM_HD DIval lincomb(DIval a, double ca, DIval b, double cb) const { return a * ca + b * cb; }       // linear: val and der alike
    RM_HD DIval mirror(DIval x) const { return dabs_pw(x); }
    RM_HD DIval round(DIval a, double k) const { return a - k; }
    RM_HD DIval scale(DIval a, double k) const { return dv(i_scale(a.val, k), i_scale(a.der, k)); }
    RM_HD DIval abs(DIval a) const { return dabs_pw(a); }
    RM_HD DIval union_(DIval a, DIval b) const { return dv(i_union(a.val, b.val), min_der(a, b)); }
    RM_HD DIval subtract(DIval a, DIval b) const { return dv(i_subtract(a.val, b.val), max_der(a, -b)); }
    RM_HD DIval intersect(DIval a, DIval b) const { return dv(i_intersect(a.val, b.val), max_der(a, b)); }
    RM_HD DIval smooth_union(DIval a, DIval b, double k) const { return dv(i_smooth_union(a.val, b.val, k), seg_hull(a.der, b.der)); }
    RM_HD DIval smooth_subtract(DIval a, DIval b, double k) const { return dv(i_smooth_subtract(a.val, b.val, k), seg_hull(a.der, -b.der)); }
    RM_HD DIval smooth_intersect(DIval a, DIval b, double k) const { return dv(i_smooth_intersect(a.val, b.val, k), seg_hull(a.der, b.der)); }
};

// The dual interval of the program over the box p of a ray segment with direction rd: val == program_eval_interval(src,
// p) bit for bit, der encloses d/dtau of the program's value along the ray wherever that derivative exists.
template <class Src>
RM_HD DIval program_eval_dual(const Src& src, IVec3 p, vec3 rd)
{
    return program_walk(DualAlgebra{}, src, dvec3(p, rd));
}

// ---- gpu/faithful_offline.py -----------------------------------------------------------------------------------------

// The tracer's constants after defaults (RmSegmentConfig with every 0 replaced by the reference's value).
struct SegmentParams {
    double t_max, tol, h0, kappa, h_min, h_max, k_min, l_global;
    double bound;          // bounding-sphere radius of the prune; < 0: no prune
    int32_t budget;
};

// segment_trace for one ray: t of the first cursor with |f| < tol, +inf on a miss (t > t_max, or the budget used up).
// `iters`: the trips the ray was active for; `cursor`: the final t.  The step |f| / K is short of the surface because K
// bounds |g'| over [t, t + h] and step <= h.
template <class Src>
RM_HD double segment_trace(const Src& src, vec3 o, vec3 d, const SegmentParams& P, int32_t* iters, double* cursor)
{
    double t = 0.0, h = P.h0, res = __builtin_inf();
    int32_t s = 0;
    while (s < P.budget) {
        ++s;
        const double f = interval_point(src, o.x + t * d.x, o.y + t * d.y, o.z + t * d.z);   // _scalar_sdf at the cursor
        if (rm_fabs(f) < P.tol) {
            res = t;
            break;
        }
        const Ival der = program_eval_dual(src, seed_segment(o, d, t, t + h), d).der;
        const double K = np_min(np_max(np_max(rm_fabs(der.lo), rm_fabs(der.hi)), P.k_min), P.l_global);   // np.clip
        const double safe = rm_fabs(f) / K;
        const double step = np_min(safe, h);
        t = t + step;
        h = np_min(np_max(np_max(step, safe) * P.kappa, P.h_min), P.h_max);
        if (t > P.t_max) break;
    }
    *iters = s;
    *cursor = t;
    return res;
}

// One pixel of faithful_capture: the library's camera ray, _prune_candidates, the trace.  A pruned ray or a miss has
// depth 0 and hit 0; a pruned ray has 0 iters and cursor 0.
template <class Src>
RM_HD void segment_pixel(const Src& src, const CameraParams& cam, int width, int height, int px, int py, const SegmentParams& P,
                         double* depth, uint8_t* hit, int32_t* iters, double* cursor)
{
    vec3 o, d;
    camera_ray(cam, width, height, px, py, o, d);
    double t = __builtin_inf(), c = 0.0;
    int32_t s = 0;
    if (interval_candidate(o, d, P.bound)) t = segment_trace(src, o, d, P, &s, &c);
    const bool h = t < __builtin_inf();
    *depth = h ? t : 0.0;
    *hit = h ? 1 : 0;
    *iters = s;
    *cursor = c;
}

// (host code) RmSegmentConfig -> SegmentParams: 0 fields take the reference's constants; `scene_bound` is the library's
// prune radius of the scene (< 0: none).  false with the reason in `why` for a negative or non-finite field, budget < 0
// or above RM_SEGMENT_MAX_STEPS, reserved != 0.  (A field of 0 is its default, so kappa <= 0 is refused as negative.)
inline bool segment_resolve(const RmSegmentConfig* c, double scene_bound, SegmentParams* P, char* why, size_t why_len)
{
    RmSegmentConfig z;
    memset(&z, 0, sizeof z);
    if (!c) c = &z;
    const double f[9] = { c->t_max, c->tol, c->h0, c->kappa, c->h_min, c->h_max, c->k_min, c->l_global, c->bound_radius };
    static const char* const names[9] = { "t_max", "tol", "h0", "kappa", "h_min", "h_max", "k_min", "l_global", "bound_radius" };
    for (int i = 0; i < 9; ++i) {
        if (!(f[i] - f[i] == 0.0)) return snprintf(why, why_len, "%s is not finite", names[i]), false;
        if (i < 8 && f[i] < 0.0) return snprintf(why, why_len, "%s is negative", names[i]), false;
    }
    if (c->budget < 0) return snprintf(why, why_len, "budget is negative"), false;
    if (c->budget > RM_SEGMENT_MAX_STEPS)
        return snprintf(why, why_len, "budget %d above the ceiling %d", (int)c->budget, RM_SEGMENT_MAX_STEPS), false;
    if (c->reserved != 0) return snprintf(why, why_len, "reserved must be 0"), false;
    P->t_max = c->t_max != 0.0 ? c->t_max : 100.0;
    P->tol = c->tol != 0.0 ? c->tol : 1e-4;
    P->h0 = c->h0 != 0.0 ? c->h0 : 0.1;
    P->kappa = c->kappa != 0.0 ? c->kappa : 1.5;
    P->h_min = c->h_min != 0.0 ? c->h_min : 1e-5;
    P->h_max = c->h_max != 0.0 ? c->h_max : 10.0;
    P->k_min = c->k_min != 0.0 ? c->k_min : 1e-6;
    P->l_global = c->l_global != 0.0 ? c->l_global : 1.0;
    P->budget = c->budget != 0 ? c->budget : 4096;
    P->bound = c->bound_radius != 0.0 ? c->bound_radius : scene_bound;
    return true;
}

}  // namespace rm
