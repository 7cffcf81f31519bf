// rm_certify.h -- the certified first hit: a proven bracket [t_lo, t_hi] on each ray (rm_certify_* in include/rm_hip.h).
//
// The interval oracle (rm_interval.h) reports a hit where a probe of length <= tol cannot be proven empty: its depth is
// early by up to that tolerance, and an enclosure that never clears (a probe across a repeat cell's boundary, a tangent CSG
// cut) is a hit though the pointwise SDF has none.  This march puts the tree's three sound pieces together instead, for
// g(tau) = f(o + tau d):
//  * proof 1: the interval enclosure of [a, a + h] has lo > 0 (sound_first_hit's rule);
//  * proof 2: g(a) > K h, K = clip(max |der|, k_min, l_global) the dual bound of |g'| over that probe (segment_trace's
//    rule, rm_segment.h): a continuous g cannot fall by more than K h over the probe, so it stays above 0 on all of it;
//  * a witness: the computed pointwise value g(b) < 0 (interval_point) shows that b lies in the solid.  (Strictly below: a
//    computed 0 is what rounding makes of a tangent contact, sqrt(1 + e^2) - 1 for |e| < 2^-27, and witnesses nothing.)
// [0, a) only ever grows by a proven probe, never by "h <= tol"; b only ever moves to a point with a computed g < 0.  So
// in real arithmetic and for a continuous g the first hit lies in [a, b] at every trip, whatever ends the march.  Rounding
// is to nearest, as everywhere in these headers ("Certified first hit").
//
// One trip is one dual-interval walk over the probe (val is the interval oracle's enclosure bit for bit, der comes with
// it) and one point walk at the probe's end: the segment tracer's two walks, so the kernels have its shape.
#pragma once

#include "rm_segment.h"

namespace rm {

// RM_CERTIFY_* of include/rm_hip.h
constexpr uint8_t kCertifyMiss = 0, kCertifyHit = 1, kCertifyOpen = 2;

// The march's constants after defaults (RmCertifyConfig with every 0 replaced).  A HIT's bracket is at most
// width + width_rel * (1 + t_lo) wide: one of the two is 0.
struct CertifyParams {
    double t_max, tol, h0, growth, h_max, width, width_rel, k_min, l_global;
    double bound;          // bounding-sphere radius of the prune; < 0: no prune
    int32_t max_steps;
};

// The bracket of one ray.  a: [0, a) is proven free; b: g(b) < 0 was computed (+inf: no witness yet); h: the next probe.
//  * a probe is [a, t1], t1 = min(a + h, b): once a witness exists the search is confined to [a, b];
//  * proven (either proof): a = t1, the probe grows as the oracle's does; unproven: the probe halves;
//  * g(t1) < 0: b = t1 (t1 <= b always), whether or not the probe was proven;
//  * with a witness the probe is at most half the bracket, so every trip that proves its probe or finds g(t1) < 0 halves
//    the bracket.
// The march ends, in this order, when a > t_max (MISS: all of [0, t_max] is proven free), when b - a is within the width
// (HIT), after max_steps probes, or when an unproven probe has shrunk to 2^-50 a, four units in the last place of the
// cursor (OPEN both: the bracket reached so far is returned, and is as sound as any).  A HIT has t_lo <= t_max; its t_hi may
// lie past t_max by no more than the width.  The eye's own g(0) < 0 is a witness before the first probe: HIT, [0, 0], 0 steps.
// `steps`: the probes made.  (g(0) is read by a trip of the same loop over the probe [0, 0], which counts as no step: the
// kernels hold each of the two walks over the program once.)
template <class Src>
RM_HD void certify_first_hit(const Src& src, vec3 o, vec3 d, const CertifyParams& P, double* t_lo, double* t_hi, uint8_t* status,
                             int32_t* steps)
{
    const double inf = __builtin_inf();
    double a = 0.0, b = inf, h = P.h0, ga = 0.0;
    int32_t s = -1;                            // the trip before the first probe reads g(0): the probe [0, 0]
    uint8_t st = kCertifyOpen;
    for (;;) {
        const bool eye = s < 0;
        if (!eye) {
            if (a > P.t_max) {
                st = kCertifyMiss;
                break;
            }
            if (b - a <= P.width + P.width_rel * (1.0 + a)) {
                st = kCertifyHit;
                break;
            }
            if (s >= P.max_steps || !(h > a * 0x1p-50)) break;
        }
        ++s;
        const double t1 = eye ? a : np_min(a + h, b);
        const DIval f = program_eval_dual(src, seed_segment(o, d, a, t1), d);
        const double g1 = interval_point(src, o.x + t1 * d.x, o.y + t1 * d.y, o.z + t1 * d.z);
        const double K = np_min(np_max(np_max(rm_fabs(f.der.lo), rm_fabs(f.der.hi)), P.k_min), P.l_global);   // as segment_trace
        const double len = t1 - a;
        if (g1 < 0.0) b = t1;
        if (eye) {
            ga = g1;
        } else if (f.val.lo > 0.0 || ga > K * len) {
            a = t1;
            ga = g1;
            h = np_min(h * P.growth, P.h_max);
        } else {
            h = len * 0.5;
        }
        if (b < inf) h = np_min(h, (b - a) * 0.5);
    }
    *t_lo = st == kCertifyMiss ? inf : a;
    *t_hi = st == kCertifyMiss ? inf : b;
    *status = st;
    *steps = s;
}

// One pixel of a certified frame: the library's camera ray, _prune_candidates, the march.  A pruned ray is a MISS with 0
// steps: the prune's sphere bounds the scene, so the ray is free of it by geometry.  It takes the march with t_max < 0, which
// ends after the eye's trip, so that the kernel has no branch round the march (one costs the render kernel registers it
// does not have: copies to the accumulation registers, which count as spills).
template <class Src>
RM_HD void certify_pixel(const Src& src, const CameraParams& cam, int width, int height, int px, int py, const CertifyParams& P,
                         double* t_lo, double* t_hi, uint8_t* status, int32_t* steps)
{
    vec3 o, d;
    camera_ray(cam, width, height, px, py, o, d);
    CertifyParams Q = P;
    if (!interval_candidate(o, d, P.bound)) Q.t_max = -1.0;
    certify_first_hit(src, o, d, Q, t_lo, t_hi, status, steps);
}

// (host code) RmCertifyConfig -> CertifyParams: 0 fields take their defaults (the interval fields as interval_resolve, k_min
// and l_global as segment_resolve, width 0 = 1e-10 (1 + t_lo)); `scene_bound` is the library's prune radius of the scene
// (< 0: none).  false with the reason in `why` for a negative or non-finite field, growth <= 1 after defaults, max_steps < 0
// or above RM_INTERVAL_MAX_STEPS, reserved != 0.
inline bool certify_resolve(const RmCertifyConfig* c, double scene_bound, CertifyParams* P, char* why, size_t why_len)
{
    RmCertifyConfig z;
    memset(&z, 0, sizeof z);
    if (!c) c = &z;
    const double f[9] = { c->t_max, c->tol, c->h0, c->growth, c->h_max, c->width, c->l_global, c->k_min, c->bound_radius };
    static const char* const names[9] = { "t_max", "tol", "h0", "growth", "h_max", "width", "l_global", "k_min", "bound_radius" };
    for (int i = 0; i < 9; ++i) {
        if (!(f[i] - f[i] == 0.0)) return snprintf(why, why_len, "%s is not finite", names[i]), false;
        if (i < 8 && f[i] < 0.0) return snprintf(why, why_len, "%s is negative", names[i]), false;
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
    P->width = c->width;
    P->width_rel = c->width != 0.0 ? 0.0 : 1e-10;
    P->l_global = c->l_global != 0.0 ? c->l_global : 1.0;
    P->k_min = c->k_min != 0.0 ? c->k_min : 1e-6;
    P->max_steps = c->max_steps != 0 ? c->max_steps : 20000;
    P->bound = c->bound_radius != 0.0 ? c->bound_radius : scene_bound;
    if (!(P->growth > 1.0)) return snprintf(why, why_len, "growth must be > 1"), false;
    return true;
}

}  // namespace rm
