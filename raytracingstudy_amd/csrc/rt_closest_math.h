// rt_closest_math.h — the closest-sphere query's arithmetic (rt_query_closest,
// include/rt.h), free of HIP and of the renderer's state: the
// probe's validity, the key (the signed distance to a sphere's surface) and the
// slack and the reach of the grown box of a bound that guides the descent
// (rt_guide_math.h: the box itself).  f32 operations in a fixed order (built
// with -ffp-contract=off like the rest, IEEE sqrtf).
// rt_closest.hip runs it per probe on the device, and
// tests/native/closest_math_dump.cpp prints it for tests/test_closest_cpu.py.
#pragma once
#include "rt_guide_math.h"

namespace rtamd {

// A probe takes part iff its centre is finite and R >= 0 (R = -0 and R = +inf
// included; a NaN R fails the comparison); any other probe has an empty set.
RT_GUIDE_HD inline bool closest_probe_ok(float px, float py, float pz, float R) {
    return finite_f32(px) && finite_f32(py) && finite_f32(pz) && R >= 0.0f;
}

// The key of sphere (c, r) for probe point p: sqrtf(d2) - r, the signed
// distance from p to the sphere's surface (negative inside), every operation
// one IEEE f32 operation in this order.  A d2 that overflows gives +inf.
RT_GUIDE_HD inline float closest_key(float px, float py, float pz, float cx, float cy, float cz, float r) {
    const float dx = px - cx;
    const float dy = py - cy;
    const float dz = pz - cz;
    const float d2 = (dx * dx + dy * dy) + dz * dz;
    return sqrtf(d2) - r;
}

// Slack of the grown box of a bound B >= 0, in units of u = 2^-24.  The
// descent may skip a cell only if no sphere listed there alone can have
// key <= B in f32.  With D the real distance from p to the centre, M the root
// box's farthest corner from the origin (every sphere lies in the root box:
// |c| <= M, r <= M) and every f32 operation within 1 + u of the real one:
//  * d2 >= D^2 (1 - u)^5 (the difference, the square, two sums), so the
//    rounded root s >= D (1 - u)^3.5 and D <= s (1 + 4u).  key = fl(s - r) <= B:
//    either s <= r, and D - r <= 4u r <= 4u M; or s - r <= B (1 + 2u), and
//    D - r <= (r + B (1 + 2u))(1 + 4u) - r <= B (1 + 7u) + 4u M.  So the
//    sphere's point q nearest p (p itself, when p is inside) is within
//    B + 7u B + 4u M of p, on every axis;
//  * q lies in a leaf cell that lists the sphere (the builders' exact double
//    sphere-box test, scene_build.cpp); a root box rounded to f32 may leave q
//    outside by at most u M, and the clamped point's cell lists the sphere
//    too: + 1u M;
//  * the grid conversion is rt_overlap_math.h's, with B for its R: the corner
//    ((p -+ grow) - rmin) * scale is three f32 operations on values within
//    2M + 2B and 3M + 2B, and scale = G / (rmax - rmin) two more:
//    2u (M + B) + 4u (3M + 2B) = 14u M + 10u B against the builders' cell edge.
// Sum: 17u B + 19u M.  grow = B (1 + kClosestSlackR u) + kClosestSlackM u M is
// itself two f32 operations (2u of it) and M one rounding of a double: + 4 on
// each.  B = +inf grows to the whole space, whatever the constants.
constexpr double kClosestNeedR = 17.0;
constexpr double kClosestNeedM = 19.0;
constexpr double kClosestSlackR = 32.0;
constexpr double kClosestSlackM = 64.0;
static_assert(kClosestSlackR >= kClosestNeedR + 4.0 && kClosestSlackM >= kClosestNeedM + 4.0,
              "the grown box covers the key's rounding, the grid conversion and its own");

// The scene's part of the slack: kClosestSlackM u M for the effective root box.
inline float closest_slack_m(const float rmin[3], const float rmax[3]) {
    return static_cast<float>(kClosestSlackM * kGuideU * root_corner_far(rmin, rmax));
}

// The grown box of a bound: the reach is max(bound, 0).  Every sphere that
// contains p is listed in p's own cell, so a negative bound (the K-th nearest
// surface is behind p) still has to reach that cell.  A cell is met on an axis
// unless lo >= l + size or hi < l (a NaN comparison visits).
using ClosestBox = GridBox;
RT_GUIDE_HD inline ClosestBox closest_box(float px, float py, float pz, float bound, const float rmin[3],
                                        const float scale[3], float slack_m) {
    const float rel = static_cast<float>(1.0 + kClosestSlackR * kGuideU);
    return grown_box(px, py, pz, bound > 0.0f ? bound : 0.0f, rel, rmin, scale, slack_m);
}

}  // namespace rtamd
