// rm_interval.h -- the interval first-hit oracle: interval arithmetic over scene programs and the sound forward march of
// the reference's gpu/interval.py and gpu/interval_oracle.py (first_hit, _prune_candidates, _normals_fd).
//
// Ival restates gpu/interval.py's Interval op for op in binary64 without contraction: np.minimum / np.maximum are
// `a < b ? a : b` / `a > b ? a : b` (numpy returns the SECOND argument on equal ones, so the signs of zeros match).
// program_eval_interval extends every RM_SOP_* of the scene-program interpreter (rm_scene_program.h) to a box:
//  * sphere, plane, box, torus: the reference's _sd_sphere / _sd_plane / _sd_box / _sd_torus, expression for
//    expression -- sd_sphere(1.0), sd_plane((0,1,0), -0.5), sd_box((1,1,1)), sd_torus(1.5, 0.05) ARE its
//    INTERVAL_SCENES, bit for bit;
//  * every other op: the natural extension of the pointwise formula of rm_scene_program.h / rm_scenes.h, written so
//    that a degenerate box (lo == hi) evaluates the pointwise expression itself.  DESIGN.md section 3, "Interval
//    oracle", gives the soundness argument of each op and lists where a degenerate value differs from program_eval.
// Rounding is to nearest, as in the reference: the enclosure is exact in real arithmetic only.
//
// The walk over the program is program_eval's (program_walk, rm_scene_program.h) with IntervalAlgebra: the eight value
// intervals and the four saved boxes are its register slots.
#pragma once

#include "rm_camera.h"
#include "rm_scene_program.h"

namespace rm {

// np.minimum / np.maximum on scalars (gpu/interval.py): the second argument on ties
RM_HD double np_min(double a, double b) { return a < b ? a : b; }
RM_HD double np_max(double a, double b) { return a > b ? a : b; }

struct Ival {
    double lo, hi;
};
RM_HD Ival iv(double lo, double hi)
{
    Ival r;
    r.lo = lo; r.hi = hi;
    return r;
}

// ---- gpu/interval.py: Interval ---------------------------------------------------------------------------------------
RM_HD Ival operator+(Ival a, Ival b) { return iv(a.lo + b.lo, a.hi + b.hi); }
RM_HD Ival operator+(Ival a, double s) { return iv(a.lo + s, a.hi + s); }
RM_HD Ival operator-(Ival a, Ival b) { return iv(a.lo - b.hi, a.hi - b.lo); }
RM_HD Ival operator-(Ival a, double s) { return iv(a.lo - s, a.hi - s); }
RM_HD Ival operator-(Ival a) { return iv(-a.hi, -a.lo); }
RM_HD Ival operator*(Ival a, Ival b)
{
    const double p0 = a.lo * b.lo, p1 = a.lo * b.hi, p2 = a.hi * b.lo, p3 = a.hi * b.hi;
    return iv(np_min(np_min(p0, p1), np_min(p2, p3)), np_max(np_max(p0, p1), np_max(p2, p3)));
}
RM_HD Ival operator*(Ival a, double s)
{
    const double x = a.lo * s, y = a.hi * s;
    return iv(np_min(x, y), np_max(x, y));
}
RM_HD Ival iabs(Ival a)
{
    return iv(a.lo >= 0.0 ? a.lo : (a.hi <= 0.0 ? -a.hi : 0.0), np_max(rm_fabs(a.lo), rm_fabs(a.hi)));
}
RM_HD Ival isquare(Ival a)
{
    const double x = a.lo * a.lo, y = a.hi * a.hi;
    return iv(a.lo >= 0.0 ? x : (a.hi <= 0.0 ? y : 0.0), np_max(x, y));
}
RM_HD Ival isqrt(Ival a) { return iv(rm_sqrt(np_max(a.lo, 0.0)), rm_sqrt(np_max(a.hi, 0.0))); }
RM_HD Ival iminimum(Ival a, Ival b) { return iv(np_min(a.lo, b.lo), np_min(a.hi, b.hi)); }
RM_HD Ival imaximum(Ival a, Ival b) { return iv(np_max(a.lo, b.lo), np_max(a.hi, b.hi)); }
RM_HD Ival imax0(Ival a) { return iv(np_max(a.lo, 0.0), np_max(a.hi, 0.0)); }
RM_HD Ival imin0(Ival a) { return iv(np_min(a.lo, 0.0), np_min(a.hi, 0.0)); }

struct IVec3 {
    Ival x, y, z;
};
RM_HD IVec3 ivec3(Ival x, Ival y, Ival z)
{
    IVec3 r;
    r.x = x; r.y = y; r.z = z;
    return r;
}
RM_HD IVec3 ipoint(vec3 p) { return ivec3(iv(p.x, p.x), iv(p.y, p.y), iv(p.z, p.z)); }
// IVec3.dot against a constant, left to right
RM_HD Ival idot(IVec3 p, vec3 n) { return p.x * n.x + p.y * n.y + p.z * n.z; }
// _length3 / IVec3.length
RM_HD Ival ilength3(Ival x, Ival y, Ival z) { return isqrt(isquare(x) + isquare(y) + isquare(z)); }

// seed_segment (gpu/interval_autodiff.py; first_hit builds the same box): the box of ro + rd * [t0, t1]
RM_HD IVec3 seed_segment(vec3 o, vec3 d, double t0, double t1)
{
    const double ax = d.x * t0, bx = d.x * t1, ay = d.y * t0, by = d.y * t1, az = d.z * t0, bz = d.z * t1;
    return ivec3(iv(np_min(ax, bx), np_max(ax, bx)) + o.x, iv(np_min(ay, by), np_max(ay, by)) + o.y,
                 iv(np_min(az, bz), np_max(az, bz)) + o.z);
}

// ---- gpu/interval.py: the metric primitives ---------------------------------------------------------------------------
RM_HD Ival i_sphere(IVec3 p, double radius) { return ilength3(p.x, p.y, p.z) - radius; }
RM_HD Ival i_plane(IVec3 p, double n0, double n1, double n2, double offset) { return p.x * n0 + p.y * n1 + p.z * n2 - offset; }
RM_HD Ival i_box(IVec3 p, double h0, double h1, double h2)
{
    const Ival qx = iabs(p.x) - h0, qy = iabs(p.y) - h1, qz = iabs(p.z) - h2;
    const Ival outside = ilength3(imax0(qx), imax0(qy), imax0(qz));
    const Ival inside = imin0(imaximum(imaximum(qx, qy), qz));
    return outside + inside;
}
RM_HD Ival i_torus(IVec3 p, double major_radius, double minor_radius)
{
    const Ival q_xz = isqrt(isquare(p.x) + isquare(p.z)) - major_radius;
    return isqrt(isquare(q_xz) + isquare(p.y)) - minor_radius;
}

// ---- extensions of the other pointwise formulas (a degenerate box evaluates the pointwise expression) ----------------
// a monotone function of one argument applied to both ends
RM_HD Ival ipow_half(Ival a) { return iv(pow_half(py_max(a.lo, 0.0)), pow_half(py_max(a.hi, 0.0))); }
// rm_fabs over an interval: the exact range, and rm_fabs(x) itself on a degenerate box
RM_HD Ival iabs_pw(Ival a)
{
    if (a.lo >= 0.0) return iv(rm_fabs(a.lo), rm_fabs(a.hi));
    if (a.hi <= 0.0) return iv(rm_fabs(a.hi), rm_fabs(a.lo));
    return iv(0.0, py_max(rm_fabs(a.lo), rm_fabs(a.hi)));
}
RM_HD Ival ihull(Ival a, Ival b) { return iv(py_min(a.lo, b.lo), py_max(a.hi, b.hi)); }

RM_HD Ival i_cylinder(IVec3 p, double radius, double half_height)                       // sd_cylinder
{
    const Ival d_radial = ipow_half(isquare(p.x) + isquare(p.z)) - radius;
    const Ival d_height = iabs_pw(p.y) - half_height;
    // max(., 0) and `** 2` of a non-negative value are monotone: both ends
    const double rl = py_max(d_radial.lo, 0.0), rh = py_max(d_radial.hi, 0.0);
    const double hl = py_max(d_height.lo, 0.0), hh = py_max(d_height.hi, 0.0);
    const Ival outside = ipow_half(iv(rm_pow(rl, 2.0) + rm_pow(hl, 2.0), rm_pow(rh, 2.0) + rm_pow(hh, 2.0)));
    const Ival inside = iv(py_min(py_max(d_radial.lo, d_height.lo), 0.0), py_min(py_max(d_radial.hi, d_height.hi), 0.0));
    return outside + inside;
}

RM_HD Ival i_capsule(IVec3 p, vec3 a, vec3 b, double radius)                            // sd_capsule
{
    const vec3 ab = b - a;
    const IVec3 ap = ivec3(p.x - a.x, p.y - a.y, p.z - a.z);
    const double den = py_max(dot(ab, ab), 1e-12);
    const Ival num = idot(ap, ab);
    // num / den (den > 0) and the clamp are monotone: both ends
    const double tl = py_max(0.0, py_min(1.0, num.lo / den)), th = py_max(0.0, py_min(1.0, num.hi / den));
    const Ival t = iv(tl, th);
    const Ival cx = t * ab.x + a.x, cy = t * ab.y + a.y, cz = t * ab.z + a.z;
    const Ival dx = p.x - cx, dy = p.y - cy, dz = p.z - cz;
    return ipow_half(isquare(dx) + isquare(dy) + isquare(dz)) - radius;
}

RM_HD Ival i_capped_torus(IVec3 p, double sc0, double sc1, double ra, double rb)         // sd_capped_torus
{
    const Ival px = iabs_pw(p.x);
    // the branch `sc1 * px > sc0 * p.y`: the decided one, the hull of both where the box leaves it open
    const Ival ca = px * sc1, cb = p.y * sc0;
    const Ival k1 = px * sc0 + p.y * sc1;
    const Ival k2 = ipow_half(isquare(px) + isquare(p.y));
    Ival k;
    if (ca.lo > cb.hi) k = k1;
    else if (!(ca.hi > cb.lo)) k = k2;
    else k = ihull(k1, k2);
    const Ival inner = isquare(p.x) + isquare(p.y) + isquare(p.z) + ra * ra - k * (2.0 * ra);
    return ipow_half(inner) - rb;
}

RM_HD Ival i_cone(IVec3 p, double c, double s, double height)                           // sd_cone
{
    const Ival q_len = ipow_half(isquare(p.x) + isquare(p.z));
    const Ival d1 = p.y - (-height);
    const Ival d2 = q_len * c + p.y * s;
    return iv(py_max(-d1.hi, d2.lo), py_max(-d1.lo, d2.hi));
}

// op_repeat, one axis with spacing s > 0.  The pointwise map is x -> a - n*s - s/2 with a = x + s/2, n = floor(a / s):
// within one cell it is x shifted, so when both ends lie in the same cell the ends map to the ends of the image;
// otherwise the image is the whole cell, [-s/2, s/2].  `Same cell` is decided on the computed a (a monotone rounding of
// x + s/2) and the computed remainders m = a mod s.  The quotient step of fmod / py_mod_pow2 is exact, but the sign fix
// m + s of a negative remainder rounds (by at most half an ulp of s), so the remainders are not exact and the test must
// not need them to be:
//  * a computed a_hi - a_lo < s/2 implies w = a_hi - a_lo < s/2 exactly, so at most one cell boundary lies between them;
//  * if one does, the exact remainders satisfy m_hi = m_lo + w - s, i.e. m_lo - m_hi = s - w > s/2: a gap the rounding of
//    the two remainders cannot close, so the computed m_lo <= m_hi holds only when both ends lie in the same cell;
//  * in the same cell m_lo <= m_hi exactly; rounding can only make the computed order fail, which gives the whole cell.
// A box wider than half a cell also gets the whole cell (sound; the march halves the segment anyway).  A degenerate box
// has a_lo == a_hi and identical remainders: it always takes the pointwise path.
RM_HD Ival irepeat_axis(Ival x, double s, bool pow2)
{
    const double alo = x.lo + s * 0.5, ahi = x.hi + s * 0.5;
    const double rlo = repeat_axis_any(x.lo, s, pow2), rhi = repeat_axis_any(x.hi, s, pow2);
    if (ahi - alo < s * 0.5 && rlo <= rhi) return iv(rlo, rhi);
    return iv(-(s * 0.5), s * 0.5);
}

// op_smooth_union(d1, d2, k) is non-decreasing in d1 and in d2 for either sign of k (inside the blend band the partial
// derivatives are h and 1 - h, outside it the function is d1 or d2): the lower corner gives lo, the upper corner hi.
// op_smooth_subtract = -su(-d1, d2): non-decreasing in d1, non-increasing in d2; op_smooth_intersect = -su(-d1, -d2):
// non-decreasing in both.
RM_HD Ival i_smooth_union(Ival a, Ival b, double k) { return iv(op_smooth_union(a.lo, b.lo, k), op_smooth_union(a.hi, b.hi, k)); }
RM_HD Ival i_smooth_subtract(Ival a, Ival b, double k)
{
    return iv(op_smooth_subtract(a.lo, b.hi, k), op_smooth_subtract(a.hi, b.lo, k));
}
RM_HD Ival i_smooth_intersect(Ival a, Ival b, double k)
{
    return iv(op_smooth_intersect(a.lo, b.lo, k), op_smooth_intersect(a.hi, b.hi, k));
}

// op_union / op_subtract / op_intersect: min and max are monotone, end for end
RM_HD Ival i_union(Ival a, Ival b) { return iv(py_min(a.lo, b.lo), py_min(a.hi, b.hi)); }
RM_HD Ival i_subtract(Ival a, Ival b) { return iv(py_max(a.lo, -b.hi), py_max(a.hi, -b.lo)); }
RM_HD Ival i_intersect(Ival a, Ival b) { return iv(py_max(a.lo, b.lo), py_max(a.hi, b.hi)); }

// ---- the four ops beyond primitives.py ("Program extensions") ------------------------------------

// RM_SOP_SCALE: factor > 0, end for end
RM_HD Ival i_scale(Ival a, double k) { return iv(a.lo * k, a.hi * k); }

// RM_SOP_LIMITED_REPEAT, one axis with spacing c > 0: x -> x - c * n(x), n the clamped cell index.  The computed n is a
// chain of monotone roundings of x, so it is non-decreasing in x: when both ends have the same n every point between them
// has it too, the map is the same shift for the whole box and the ends map to the ends of the image.  Otherwise the map
// is made of pieces of slope 1 separated by downward jumps at cell edges, where the value falls from c/2 (or, with a
// fractional limit, from less) to -c/2 (or more); its supremum is taken at the upper end or just below a jump, its infimum
// at the lower end or just above one: the hull of the two end values and [-c/2, c/2].  The end values are the pointwise
// ones, so the clamped outer cells, where the value leaves [-c/2, c/2], are covered.  A degenerate box has one n.
RM_HD Ival ilimited_repeat_axis(Ival x, double c, double l)
{
    const double flo = limited_repeat_axis(x.lo, c, l), fhi = limited_repeat_axis(x.hi, c, l);
    if (limited_repeat_cell(x.lo, c, l) == limited_repeat_cell(x.hi, c, l)) return iv(flo, fhi);
    return iv(py_min(py_min(flo, fhi), -(c * 0.5)), py_max(py_max(flo, fhi), c * 0.5));
}

// RM_SOP_MENGER_CROSS.  a = py_mod(x * s, 2) - 1 is irepeat_axis's situation with period 2 and no half-cell shift: the
// same argument on the computed remainders (exact but for the sign fix m + 2) decides `same cell`; a box that may span a
// jump, or is wider than half a period, gets the whole period [-1, 1].  |a| is continuous across the jump, so
// r = |1 - 3 |a|| is a continuous function of x and everything after it is monotone min / max.
RM_HD Ival imenger_a(Ival x, double s)
{
    const double ulo = x.lo * s, uhi = x.hi * s;
    const double mlo = py_mod_pow2(ulo, 2.0), mhi = py_mod_pow2(uhi, 2.0);
    if (uhi - ulo < 1.0 && mlo <= mhi) return iv(mlo - 1.0, mhi - 1.0);
    return iv(-1.0, 1.0);
}
RM_HD Ival imenger_fold(Ival x, double s)
{
    const Ival b = iabs_pw(imenger_a(x, s));
    return iabs_pw(iv(1.0 - 3.0 * b.hi, 1.0 - 3.0 * b.lo));
}
RM_HD Ival i_menger_cross(IVec3 p, double s, double s3)
{
    const Ival rx = imenger_fold(p.x, s), ry = imenger_fold(p.y, s), rz = imenger_fold(p.z, s);
    const Ival da = i_intersect(rx, ry), db = i_intersect(ry, rz), dc = i_intersect(rz, rx);
    const Ival m = i_union(da, i_union(db, dc));
    return iv((m.lo - 1.0) / s3, (m.hi - 1.0) / s3);
}

// sin and cos over an interval.  A degenerate box is the pointwise value (NaN outside rm_sincos' exact range).  Otherwise:
// the end values from rm_sincos, and +1 / -1 wherever the box may contain an extremum.  The extrema lie at q = j * pi/2
// (sin: +1 at j = 1, -1 at j = 3 mod 4; cos: +1 at j = 0, -1 at j = 2 mod 4); v = q * (2 / pi) is computed with an error
// below |v| * 2^-51, so every integer within |v| * 2^-50 of [v_lo, v_hi] counts as inside -- an extremum too many costs
// less than 1e-14, one missed would be unsound.  A box of 2 pi or more contains all four residues and gets [-1, 1] by the
// same test.  An end outside the exact range, or not finite, gives [-1, 1].
struct ISinCos {
    Ival s, c;
};
RM_HD bool icontains_residue(int32_t jlo, int32_t jhi, int32_t r) { return jlo + ((r - jlo) & 3) <= jhi; }
RM_HD ISinCos isincos(Ival q)
{
    ISinCos o;
    double slo, clo, shi, chi;
    rm_sincos(q.lo, &slo, &clo);
    rm_sincos(q.hi, &shi, &chi);
    if (q.lo == q.hi) {
        o.s = iv(slo, shi); o.c = iv(clo, chi);
        return o;
    }
    const double lim = 0x1.921fbp+26;
    if (!(rm_fabs(q.lo) < lim && rm_fabs(q.hi) < lim)) {
        o.s = iv(-1.0, 1.0); o.c = iv(-1.0, 1.0);
        return o;
    }
    const double two_over_pi = 0x1.45f306dc9c883p-1;
    const double vlo = q.lo * two_over_pi, vhi = q.hi * two_over_pi;
    const int32_t jlo = (int32_t)-rm_floor((rm_fabs(vlo) * 0x1p-50 + 0x1p-60) - vlo);
    const int32_t jhi = (int32_t)rm_floor(vhi + (rm_fabs(vhi) * 0x1p-50 + 0x1p-60));
    o.s = iv(icontains_residue(jlo, jhi, 3) ? -1.0 : py_min(slo, shi), icontains_residue(jlo, jhi, 1) ? 1.0 : py_max(slo, shi));
    o.c = iv(icontains_residue(jlo, jhi, 2) ? -1.0 : py_min(clo, chi), icontains_residue(jlo, jhi, 0) ? 1.0 : py_max(clo, chi));
    return o;
}
// sin and cos of the three coordinates of freq * p, one axis per trip of a loop that stays a loop (the axes rotate through
// q0, the results shift through x, y, z): six inlined copies of rm_sincos side by side cost the segment kernels their
// vector registers
struct ISinCos3 {
    ISinCos x, y, z;
};
RM_HD ISinCos3 isincos3(IVec3 p, double freq)
{
    Ival q0 = p.x * freq, q1 = p.y * freq, q2 = p.z * freq;
    ISinCos3 o;
    o.x.s = o.x.c = o.y.s = o.y.c = o.z.s = o.z.c = iv(0.0, 0.0);
#pragma unroll 1
    for (int a = 0; a < 3; ++a) {
        const ISinCos r = isincos(q0);
        o.x = o.y; o.y = o.z; o.z = r;
        const Ival t = q0;
        q0 = q1; q1 = q2; q2 = t;
    }
    return o;
}
// RM_SOP_GYROID: the pointwise expression over intervals, summed left to right
RM_HD Ival i_gyroid(IVec3 p, double freq, double lipschitz)
{
    const ISinCos3 sc = isincos3(p, freq);
    const ISinCos x = sc.x, y = sc.y, z = sc.z;
    const Ival g = x.s * y.c + y.s * z.c + z.s * x.c;
    return iv(g.lo / lipschitz, g.hi / lipschitz);
}

// ---- the interpreter ----------------------------------------------------------------------------------------------

// evaluation over a box (program_walk, rm_scene_program.h)
struct IntervalAlgebra {
    typedef Ival Value;
    typedef IVec3 Point;
    RM_HD Ival sphere(IVec3 p, double r) const { return i_sphere(p, r); }
    RM_HD Ival box(IVec3 p, double h0, double h1, double h2) const { return i_box(p, h0, h1, h2); }
    RM_HD Ival plane(IVec3 p, double n0, double n1, double n2, double offset) const { return i_plane(p, n0, n1, n2, offset); }
    RM_HD Ival cylinder(IVec3 p, double radius, double half_height) const { return i_cylinder(p, radius, half_height); }
    RM_HD Ival torus(IVec3 p, double major_radius, double minor_radius) const { return i_torus(p, major_radius, minor_radius); }
    RM_HD Ival capsule(IVec3 p, vec3 a, vec3 b, double radius) const { return i_capsule(p, a, b, radius); }
    RM_HD Ival capped_torus(IVec3 p, double sc0, double sc1, double ra, double rb) const { return i_capped_torus(p, sc0, sc1, ra, rb); }
    RM_HD Ival cone(IVec3 p, double c, double s, double height) const { return i_cone(p, c, s, height); }
    RM_HD Ival menger_cross(IVec3 p, double s, double s3) const { return i_menger_cross(p, s, s3); }
    RM_HD Ival gyroid(IVec3 p, double freq, double lipschitz) const { return i_gyroid(p, freq, lipschitz); }
    RM_HD IVec3 translate(IVec3 p, double kx, double ky, double kz) const { return ivec3(p.x - kx, p.y - ky, p.z - kz); }
    RM_HD Ival repeat(Ival x, double spacing, bool pow2) const { return irepeat_axis(x, spacing, pow2); }
    RM_HD Ival limited_repeat(Ival x, double spacing, double limit) const { return ilimited_repeat_axis(x, spacing, limit); }
    // RM_SOP_ROTATE: the two coordinates are taken as independent, so a tilted box is enclosed by an axis-aligned one (the
    // wrapping effect); a degenerate box evaluates the pointwise expression.  RM_SOP_MIRROR: the exact range of |x|.
    RM_HD Ival lincomb(Ival a, double ca, Ival b, double cb) const { return a * ca + b * cb; }
    RM_HD Ival mirror(Ival x) const { return iabs_pw(x); }
    RM_HD Ival round(Ival a, double k) const { return a - k; }
    RM_HD Ival scale(Ival a, double k) const { return i_scale(a, k); }
    RM_HD Ival abs(Ival a) const { return iabs_pw(a); }
    RM_HD Ival union_(Ival a, Ival b) const { return i_union(a, b); }
    RM_HD Ival subtract(Ival a, Ival b) const { return i_subtract(a, b); }
    RM_HD Ival intersect(Ival a, Ival b) const { return i_intersect(a, b); }
    RM_HD Ival smooth_union(Ival a, Ival b, double k) const { return i_smooth_union(a, b, k); }
    RM_HD Ival smooth_subtract(Ival a, Ival b, double k) const { return i_smooth_subtract(a, b, k); }
    RM_HD Ival smooth_intersect(Ival a, Ival b, double k) const { return i_smooth_intersect(a, b, k); }
};

// The interval of the program's value over the box p (same image, words and constants as program_eval).
template <class Src>
RM_HD Ival program_eval_interval(const Src& src, IVec3 p)
{
    return program_walk(IntervalAlgebra{}, src, p);
}

// ---- gpu/interval_oracle.py ---------------------------------------------------------------------------------------

// The march's constants after defaults (RmIntervalConfig with every 0 replaced by the reference's value).
struct IntervalParams {
    double t_max, tol, h0, growth, h_max, normal_eps;
    double bound;          // bounding-sphere radius of the prune; < 0: no prune
    int32_t max_steps;
};

// first_hit for one ray: t of the first segment [t, t + h] whose enclosure reaches 0 with h <= tol, +inf on a miss.
// `steps`: the loop trips the ray was active for (the reference's active iterations).  `range(t, t1)` is the sound
// enclosure (an Ival) of the scene over the segment: the interval program here, the affine one in rm_affine.h
// (gpu/affine.py's march_count is this loop with its range function plugged in).
template <class Range>
RM_HD double sound_first_hit(const Range& range, const IntervalParams& P, int32_t* steps)
{
    double t = 0.0, h = P.h0, res = __builtin_inf();
    int32_t s = 0;
    while (s < P.max_steps) {
        const double t1 = t + h;
        const Ival f = range(t, t1);
        ++s;
        if (f.lo > 0.0) {                      // proven empty: jump and grow the probe
            t = t1;
            h = np_min(h * P.growth, P.h_max);
            if (t > P.t_max) break;
        } else if (h <= P.tol) {               // first contact bracketed
            res = t;
            break;
        } else {
            h = h * 0.5;                       // shrink and re-probe the same cursor
        }
    }
    *steps = s;
    return res;
}

template <class Src>
RM_HD double interval_first_hit(const Src& src, vec3 o, vec3 d, const IntervalParams& P, int32_t* steps)
{
    return sound_first_hit([&](double t, double t1) { return program_eval_interval(src, seed_segment(o, d, t, t1)); }, P, steps);
}

// _scalar_sdf: the interval program at a degenerate box, lo
template <class Src>
RM_HD double interval_point(const Src& src, double x, double y, double z)
{
    return program_eval_interval(src, ivec3(iv(x, x), iv(y, y), iv(z, z))).lo;
}

// _normals_fd at P = o + t * d: central differences of _scalar_sdf, then _normalize (np.linalg.norm over the last axis
// sums left to right)
template <class Src>
RM_HD vec3 interval_normal(const Src& src, vec3 o, vec3 d, double t, double eps)
{
    const double px = o.x + t * d.x, py = o.y + t * d.y, pz = o.z + t * d.z;
    const double gx = interval_point(src, px + eps, py + 0.0, pz + 0.0) - interval_point(src, px - eps, py - 0.0, pz - 0.0);
    const double gy = interval_point(src, px + 0.0, py + eps, pz + 0.0) - interval_point(src, px - 0.0, py - eps, pz - 0.0);
    const double gz = interval_point(src, px + 0.0, py + 0.0, pz + eps) - interval_point(src, px - 0.0, py - 0.0, pz - eps);
    const double nrm = np_max(rm_sqrt((gx * gx + gy * gy) + gz * gz), 1e-12);
    return v3(gx / nrm, gy / nrm, gz / nrm);
}

// _prune_candidates for an origin-centred bounding sphere of radius `bound` (< 0: every ray is a candidate)
RM_HD bool interval_candidate(vec3 o, vec3 d, double bound)
{
    if (bound < 0.0) return true;
    const double proj = d.x * o.x + d.y * o.y + d.z * o.z;
    const double dist2 = (o.x * o.x + o.y * o.y + o.z * o.z) - proj * proj;
    return (dist2 <= bound * bound) && (-proj + bound > 1e-6);
}

// One pixel of interval_capture: the library's camera ray (rm_camera.h), prune, march, normal (only with want_normal).  A
// pruned ray or a miss has depth 0, hit 0, normal 0 and (pruned) 0 steps.
template <class Src>
RM_HD void interval_pixel(const Src& src, const CameraParams& cam, int width, int height, int px, int py,
                          const IntervalParams& P, bool want_normal, double* depth, uint8_t* hit, vec3* normal, int32_t* steps)
{
    vec3 o, d;
    camera_ray(cam, width, height, px, py, o, d);
    double t = __builtin_inf();
    int32_t s = 0;
    if (interval_candidate(o, d, P.bound)) t = interval_first_hit(src, o, d, P, &s);
    const bool h = t < __builtin_inf();
    *depth = h ? t : 0.0;
    *hit = h ? 1 : 0;
    *steps = s;
    *normal = h && want_normal ? interval_normal(src, o, d, t, P.normal_eps) : v3(0.0, 0.0, 0.0);   // 6 evaluations
}

// (host code) RmIntervalConfig -> IntervalParams: 0 fields take the reference's constants; `scene_bound` is the
// library's prune radius of the scene (< 0: none).  false with the reason in `why` for a negative or non-finite field,
// growth <= 1 after defaults, max_steps < 0 or above RM_INTERVAL_MAX_STEPS, reserved != 0.
inline bool interval_resolve(const RmIntervalConfig* c, double scene_bound, IntervalParams* P, char* why, size_t why_len)
{
    RmIntervalConfig z;
    memset(&z, 0, sizeof z);
    if (!c) c = &z;
    const double f[7] = { c->t_max, c->tol, c->h0, c->growth, c->h_max, c->normal_eps, c->bound_radius };
    static const char* const names[7] = { "t_max", "tol", "h0", "growth", "h_max", "normal_eps", "bound_radius" };
    for (int i = 0; i < 7; ++i) {
        if (!(f[i] - f[i] == 0.0)) return snprintf(why, why_len, "%s is not finite", names[i]), false;
        if (i < 6 && f[i] < 0.0) return snprintf(why, why_len, "%s is negative", names[i]), false;
    }
    if (c->max_steps < 0) return snprintf(why, why_len, "max_steps is negative"), false;
    if (c->max_steps > RM_INTERVAL_MAX_STEPS)
        return snprintf(why, why_len, "max_steps %d above the ceiling %d", (int)c->max_steps, RM_INTERVAL_MAX_STEPS), false;
    if (c->reserved != 0) return snprintf(why, why_len, "reserved must be 0"), false;
    P->t_max = c->t_max != 0.0 ? c->t_max : 100.0;
    P->tol = c->tol != 0.0 ? c->tol : 1e-5;
    P->h0 = c->h0 != 0.0 ? c->h0 : 0.25;
    P->growth = c->growth != 0.0 ? c->growth : 1.5;
    P->h_max = c->h_max != 0.0 ? c->h_max : 10.0;
    P->normal_eps = c->normal_eps != 0.0 ? c->normal_eps : 1e-4;
    P->max_steps = c->max_steps != 0 ? c->max_steps : 20000;
    P->bound = c->bound_radius != 0.0 ? c->bound_radius : scene_bound;
    if (!(P->growth > 1.0)) return snprintf(why, why_len, "growth must be > 1"), false;
    return true;
}

// SCENE_BOUND of gpu/interval_oracle.py by catalogue id (Sphere, Cube, Thin Torus); -1: no prune
inline double interval_scene_bound(int scene_id)
{
    switch (scene_id) {
        case 0: return 1.05;
        case 2: return 1.7421;
        case 3: return 1.65;
    }
    return -1.0;
}

}  // namespace rm
