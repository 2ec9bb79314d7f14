// rt_guide_math.h — the arithmetic that the guided octree descents
// (rt_descent.h) share, free of HIP and of the renderer's state: the grown
// box of a point and a reach in the walk's grid coordinates, the root box's
// farthest corner, and the finiteness test of a query's inputs.  f32 operations
// in a fixed order (built with -ffp-contract=off like the rest).  Each query's
// own header (rt_overlap_math.h, rt_closest_math.h, rt_sweep_math.h) derives
// its constants and calls these with them; tests/native/guide_math_dump.cpp
// prints them for tests/test_guide_math_cpu.py.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RT_GUIDE_HD __host__ __device__
#else
#define RT_GUIDE_HD
#endif

namespace rtamd {

constexpr double kGuideU = 1.0 / 16777216.0;  // u = 2^-24, the unit of every slack constant

// x is neither NaN nor infinite: !(|x| <= FLT_MAX) <=> x is one of them
constexpr float kF32Max = 3.402823466e+38f;
RT_GUIDE_HD inline bool finite_f32(float x) { return fabsf(x) <= kF32Max; }

// M: the distance from the origin of the root box's farthest corner.  Every
// sphere lies in the root box, so |c| <= M and r <= M.  A query's slack_m is
// its own constant times u M, rounded to f32 once.
inline double root_corner_far(const float rmin[3], const float rmax[3]) {
    double m2 = 0.0;
    for (int i = 0; i < 3; ++i) {
        const double a = fabs(static_cast<double>(rmin[i])), b = fabs(static_cast<double>(rmax[i]));
        const double c = a > b ? a : b;
        m2 += c * c;
    }
    return sqrt(m2);
}

// A box in the walk's grid coordinates (SceneArgs::rmin, scale): a cell
// [l, l + size) of the finest grid is met on an axis iff lo < l + size and
// hi >= l (the descent's mid-plane rule, level by level).
struct GridBox {
    float lo[3], hi[3];
};

// The box of the points within grow = reach * rel + slack_m of p on every
// axis: rel = 1 + (the query's relative slack) u in f32, slack_m its scene
// part.  Monotone in the reach: a smaller reach's box lies inside a larger
// one's.  reach = +inf grows to the whole space.
RT_GUIDE_HD inline GridBox grown_box(float px, float py, float pz, float reach, float rel, const float rmin[3],
                                     const float scale[3], float slack_m) {
    const float grow = reach * rel + slack_m;
    const float p[3] = {px, py, pz};
    GridBox b;
    for (int i = 0; i < 3; ++i) {
        b.lo[i] = ((p[i] - grow) - rmin[i]) * scale[i];
        b.hi[i] = ((p[i] + grow) - rmin[i]) * scale[i];
    }
    return b;
}

}  // namespace rtamd
