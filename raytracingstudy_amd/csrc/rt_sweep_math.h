// rt_sweep_math.h — the swept-sphere query's arithmetic (rt_sweep_spheres,
// rt_sweep_at, rt_pick_thick; include/rt.h), free of HIP and
// of the renderer's state: the cast's validity, the inflated ray-sphere test
// and the grown-cell slab test that guides the descent.  f32 operations in a
// fixed order (built with -ffp-contract=off like the rest, IEEE sqrtf and
// division).  rt_sweep.hip runs it per cast on the device, and
// tests/native/sweep_math_dump.cpp prints it for tests/test_sweep_cpu.py.
#pragma once
#include "rt_guide_math.h"

namespace rtamd {

// A cast takes part iff its origin and direction are finite, its radius is
// finite and >= 0 (R = -0 included; a NaN R fails the comparison) and its
// direction is of unit length to 2^-18: |((dx*dx + dy*dy) + dz*dz) - 1| <=
// 2^-18 in f32, in that order (a direction normalised in f32 is within
// 4 * 2^-24).  R is in world units, so t has to be: the test below is a sphere
// test for a unit direction only.  Any other cast misses.
constexpr float kGuideUnitTol = 1.0f / 262144.0f;  // 2^-18
RT_GUIDE_HD inline bool sweep_cast_ok(float ox, float oy, float oz, float dx, float dy, float dz, float R) {
    const bool finite = finite_f32(ox) && finite_f32(oy) && finite_f32(oz) && finite_f32(dx) &&
                        finite_f32(dy) && finite_f32(dz);
    const float n2 = (dx * dx + dy * dy) + dz * dz;
    return finite && R >= 0.0f && R <= kF32Max && fabsf(n2 - 1.0f) <= kGuideUnitTol;
}

// The frames' ray-sphere test (rt_walk.h isect, oracle.c:isect: the same fmaf
// chain, the same window and the same fall-through to the far root) against
// the sphere (c, s), s = r + R one f32 add.  entry_only: the near root alone
// counts (RT_SWEEP_ENTRY_ONLY).
RT_GUIDE_HD inline bool sweep_isect(float ox, float oy, float oz, float dx, float dy, float dz, float cx,
                                  float cy, float cz, float r, float R, float tmin, float tmax,
                                  bool entry_only, float& tout) {
    const float s = r + R;
    const float ocx = ox - cx;
    const float ocy = oy - cy;
    const float ocz = oz - cz;
    const float b = fmaf(ocz, dz, fmaf(ocy, dy, ocx * dx));
    const float qx = fmaf(-b, dx, ocx);
    const float qy = fmaf(-b, dy, ocy);
    const float qz = fmaf(-b, dz, ocz);
    const float qq = fmaf(qz, qz, fmaf(qy, qy, qx * qx));
    const float h = fmaf(s, s, -qq);
    if (h < 0.0f) return false;
    const float sq = sqrtf(h);
    float t = -b - sq;
    if (!(t > tmin)) {
        if (entry_only) return false;
        t = -b + sq;
    }
    if (!(t > tmin) || !(t < tmax)) return false;
    tout = t;
    return true;
}

// Slack of a grown cell, in units of u = 2^-24.  The descent may skip a cell
// only if no sphere listed in that cell alone can be accepted in f32 with a t
// at or below the current bound (closed: an equal t with a smaller index must
// still get in).  Take an accepted sphere (c, r) with its f32 t, the real
// point p = o + t d, L = |o - c| <= |o| + M, M the root box's farthest corner
// from the origin (every sphere lies in the root box: |c| <= M, r <= M), and
// every f32 operation within 1 + u of the real one.
//  * The test.  With oc as computed (a centre moved by at most u L), b its
//    computed projection (3 roundings: |b - oc.d| <= 3u L) and q' = oc - b d,
//    p - c = q' + (t + b) d.  h >= 0 bounds |q'| <= s (1 + 3u) and (t + b)^2 <=
//    s^2 - |q'|^2 + 8u s^2, and t's own rounding adds u (|b| + s) to |t + b|.
//    |d|^2 = 1 + e with |e| <= 2^-18 + 3u < 68u makes q'.d = (oc.d - b) - b e,
//    at most 72u L.  So |p - c|^2 <= s^2 + 147u L s + 79u s^2, |p - c| <= s +
//    74.5u L + 39.5u s, and with s <= (r + R)(1 + u) the ball (c, r) has a
//    point q within R + 75u |o| + 116u M + 41u R of p, on every axis;
//  * q lies in a leaf cell that lists the sphere (the builders' exact double
//    sphere-box test, scene_build.cpp); a root box rounded to f32 may leave q
//    outside by at most u M, and the clamped point's cell lists the sphere
//    too: + 1u M.  So that cell, grown by the sum on every axis, holds p, and
//    t lies between the cell's slab roots on every axis;
//  * a slab root ((k -+ g) - og) * inv, og = (o - rmin) * scale, inv = 1 /
//    (d * scale), g = grow * scale, scale = G / (rmax - rmin): the plane's
//    position carries rt_overlap_math.h's grid conversion with |o| + M for its
//    M (8u (|o| + M) + 4u grow), and the root's five roundings move it as a
//    plane moved by 5u of |plane - o| <= |o| + 2M + grow would.  Planes moved
//    outward by that much give roots on the far side of the real ones:
//    24u (|o| + M) + 12u grow covers it.
// Sum: 53u R + 99u |o| + 142u M.  grow = R (1 + kSweepSlackR u) + kSweepSlackO
// u (|ox| + |oy| + |oz|) + kSweepSlackM u M is itself five f32 operations and M
// one rounding of a double: + 6 on each.  A NaN comparison visits.
constexpr double kSweepNeedR = 53.0;
constexpr double kSweepNeedO = 99.0;
constexpr double kSweepNeedM = 142.0;
constexpr double kSweepSlackR = 128.0;
constexpr double kSweepSlackO = 256.0;
constexpr double kSweepSlackM = 256.0;
static_assert(kSweepSlackR >= kSweepNeedR + 6.0 && kSweepSlackO >= kSweepNeedO + 6.0 &&
                  kSweepSlackM >= kSweepNeedM + 6.0,
              "the grown cell covers the test's rounding, the slab roots' and its own");

// The scene's part of the slack: kSweepSlackM u M for the effective root box.
inline float sweep_slack_m(const float rmin[3], const float rmax[3]) {
    return static_cast<float>(kSweepSlackM * kGuideU * root_corner_far(rmin, rmax));
}
// The cast's part: kSweepSlackO u (|ox| + |oy| + |oz|), a bound of |o|.
RT_GUIDE_HD inline float sweep_slack_o(float ox, float oy, float oz) {
    return static_cast<float>(kSweepSlackO * kGuideU) * ((fabsf(ox) + fabsf(oy)) + fabsf(oz));
}

// A cast in the walk's grid coordinates (SceneArgs::rmin, scale), made once:
// per axis the origin, the reciprocal of the direction (+-inf for a zero
// component) and the cells' growth.  slack = sweep_slack_o + the scene's
// sweep_slack_m (tests pass 0 to show that the slack is used).
struct SweepGuide {
    float og[3], inv[3], g[3];
};
RT_GUIDE_HD inline SweepGuide sweep_guide(float ox, float oy, float oz, float dx, float dy, float dz, float R,
                                        const float rmin[3], const float scale[3], float slack) {
    const float rel = static_cast<float>(1.0 + kSweepSlackR * kGuideU);
    const float grow = R * rel + slack;
    const float o[3] = {ox, oy, oz}, d[3] = {dx, dy, dz};
    SweepGuide s;
    for (int i = 0; i < 3; ++i) {
        s.og[i] = (o[i] - rmin[i]) * scale[i];
        s.inv[i] = 1.0f / (d[i] * scale[i]);
        s.g[i] = grow * scale[i];
    }
    return s;
}

// The slab of the grown cell [k0 - g, k1 + g] on axis i (k0 < k1: integer grid
// planes, exact in f32): the cast's centre is inside it for t in [enter,
// exit].  A zero direction component gives [-inf, +inf] when the origin is
// strictly inside the slab, an empty interval when it is outside, and a NaN
// on a grown plane itself.
struct SweepSlab {
    float enter, exit;
};
RT_GUIDE_HD inline SweepSlab sweep_slab(const SweepGuide& s, int i, float k0, float k1) {
    const float a = ((k0 - s.g[i]) - s.og[i]) * s.inv[i];
    const float b = ((k1 + s.g[i]) - s.og[i]) * s.inv[i];
    const bool neg = s.inv[i] < 0.0f;  // (the reciprocal's sign: -0 counts as negative)
    SweepSlab r;
    r.enter = neg ? b : a;
    r.exit = neg ? a : b;
    return r;
}

// Whether the segment tmin < t <= bound may have its centre in the grown cell
// whose three slabs these are: every prune written so that a NaN comparison
// visits (fmaxf / fminf drop a NaN operand: that axis does not prune).
RT_GUIDE_HD inline bool sweep_meets(const SweepSlab& x, const SweepSlab& y, const SweepSlab& z, float tmin,
                                  float bound) {
    const float enter = fmaxf(fmaxf(x.enter, y.enter), z.enter);
    const float exit = fminf(fminf(x.exit, y.exit), z.exit);
    return !(enter > exit) && !(enter > bound) && !(exit < tmin);
}

}  // namespace rtamd
