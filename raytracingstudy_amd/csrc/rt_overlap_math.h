// rt_overlap_math.h — the sphere-overlap query's arithmetic (rt_query_overlaps,
// include/rt.h), free of HIP and of the renderer's state: the
// acceptance predicate and the slack of the grown box that guides the descent
// (rt_guide_math.h: the box itself).  f32 operations in a fixed order (built
// with -ffp-contract=off like the rest).
// rt_overlap.hip runs it per probe on the device, and
// tests/native/overlap_math_dump.cpp prints it for tests/test_overlap_cpu.py.
#pragma once
#include "rt_guide_math.h"

namespace rtamd {

// A probe takes part iff its four components are finite and R >= 0 (R = -0
// included); any other probe has an empty set.
RT_GUIDE_HD inline bool overlap_probe_ok(float px, float py, float pz, float R) {
    return finite_f32(px) && finite_f32(py) && finite_f32(pz) && R >= 0.0f && R <= kF32Max;
}

// The acceptance predicate: probe (p, R) touches sphere (c, r) iff
// d2 <= s * s, closed, every operation one IEEE f32 operation in this order.
RT_GUIDE_HD inline bool overlap_accepts(float px, float py, float pz, float R, float cx, float cy,
                                      float cz, float r) {
    const float dx = px - cx;
    const float dy = py - cy;
    const float dz = pz - cz;
    const float d2 = (dx * dx + dy * dy) + dz * dz;
    const float s = R + r;
    return d2 <= s * s;
}

// Slack of the grown box, in units of u = 2^-24.  With D the
// real distance of the centres, M the root box's farthest corner from the
// origin (every sphere lies in the root box, so |c| <= M and r <= M) and
// every f32 operation within 1 + u of the real one:
//  * the predicate accepts only D <= (R + r) sqrt((1 + u)^3 / (1 - u)^5)
//    <= (R + r)(1 + 5u): the sphere's point q nearest the probe's centre is
//    within R + 5u R + 5u M of it, on every axis;
//  * q lies in a leaf cell that lists the sphere (the builders' exact double
//    sphere-box test, scene_build.cpp); a root box rounded to f32 may leave q
//    outside by at most u M, and the clamped point's cell lists the sphere too:
//    + 1u M;
//  * the box corner's grid coordinate ((p -+ grow) - rmin) * scale is three
//    f32 operations on values within 2M + 2R and 3M + 2R, and scale =
//    G / (rmax - rmin) is two more: 2u (M + R) + 4u (3M + 2R) = 14u M + 10u R
//    against the builders' cell edge lo + ext * (c / cells), exact to 2^-52.
// Sum: 15u R + 20u M.  grow = R (1 + kOverlapSlackR u) + kOverlapSlackM u M
// is itself two f32 operations (2u of it) and M one rounding of a double:
// the constants keep more than half of themselves in hand.
constexpr double kOverlapNeedR = 15.0;
constexpr double kOverlapNeedM = 20.0;
constexpr double kOverlapSlackR = 32.0;
constexpr double kOverlapSlackM = 64.0;
static_assert(kOverlapSlackR >= kOverlapNeedR + 4.0 && kOverlapSlackM >= kOverlapNeedM + 4.0,
              "the grown box covers the predicate's rounding, the grid conversion and its own");

// The scene's part of the slack: kOverlapSlackM u M for the effective root box.
inline float overlap_slack_m(const float rmin[3], const float rmax[3]) {
    return static_cast<float>(kOverlapSlackM * kGuideU * root_corner_far(rmin, rmax));
}

// The grown box of probe (p, R): the reach is R itself.
using OverlapBox = GridBox;
RT_GUIDE_HD inline OverlapBox overlap_box(float px, float py, float pz, float R, const float rmin[3],
                                        const float scale[3], float slack_m) {
    const float rel = static_cast<float>(1.0 + kOverlapSlackR * kGuideU);
    return grown_box(px, py, pz, R, rel, rmin, scale, slack_m);
}

}  // namespace rtamd
