// rt_reproject_math.h — the arithmetic of carrying a per-pixel layer across
// camera motion (rt_reproject_layer; include/rt.h), free of HIP
// and of the renderer's state: the call's validity, a hit point's position in
// the previous camera's image, a tap's inside test, acceptance and weight, the
// count and the blend.  rt_reproject.hip calls these per lane around its own
// loads (issued ahead of the decisions, from clamped addresses); rt_queries.cpp
// calls the field checks.  reproject_pixel is the specification's loop for one
// pixel over host arrays, built of the same functions: only
// tests/native/reproject_math_dump.cpp runs it, over an image, for
// tests/test_reproject_cpu.py, which holds it and the functions to
// tests/reproject_ref.py's numpy restatement bit for bit; the kernel's own loop is
// held to the same reference in tests/test_gpu_reproject.py.  f32 operations in a
// fixed order (built with -ffp-contract=off like the rest, IEEE division and
// square root), no transcendental.
#pragma once
#include "rt_guide_math.h"

namespace rtamd {

constexpr uint32_t kReprojectNoHit = 0xFFFFFFFFu;  // RT_NO_HIT: an rt_hit's sphere word of a miss

// rt_reproject_params (include/rt.h) field by field; a NaN fails every comparison
RT_GUIDE_HD inline bool reproject_channels_ok(uint32_t channels) { return channels == 1u || channels == 4u; }
RT_GUIDE_HD inline bool reproject_max_count_ok(float max_count) { return finite_f32(max_count) && max_count >= 1.0f; }
RT_GUIDE_HD inline bool reproject_depth_tol_ok(float depth_tol) { return depth_tol > 0.0f; }
RT_GUIDE_HD inline bool reproject_params_ok(uint32_t channels, float max_count, float depth_tol, uint32_t flags) {
    return reproject_channels_ok(channels) && reproject_max_count_ok(max_count) && reproject_depth_tol_ok(depth_tol) &&
           flags == 0u;
}

// The previous camera as the pass reads it: its origin, the three rows of its
// pose's rotation block used as given (rows of the transposed block: no inverse
// is taken, so a pose that is no rotation projects as the arithmetic says), and
// the four intrinsic entries Camera::getRay reads.
struct PrevCamera {
    float o[3];
    float r[9];  // r[3*k + m] = pose[4*k + m]
    float fx, fy, cx, cy;
};
RT_GUIDE_HD inline PrevCamera prev_camera(const float pose[16], const float K[9]) {
    PrevCamera c;
    for (int k = 0; k < 3; ++k) {
        c.o[k] = pose[12 + k];
        for (int m = 0; m < 3; ++m) c.r[3 * k + m] = pose[4 * k + m];
    }
    c.fx = K[0], c.fy = K[4], c.cx = K[2], c.cy = K[5];
    return c;
}

// Where the current pixel's hit point lies in the previous image: the corner
// tap (u0, v0) as floats (they may be huge, infinite or NaN: tap_inside decides in
// float), the bilinear fractions, the point's distance from the previous origin,
// and whether the point is in front of the previous camera (false for a NaN).
struct Reprojection {
    float u0, v0, a, b, dist;
    bool front;
};
RT_GUIDE_HD inline Reprojection reproject_point(const PrevCamera& c, const float o[3], const float d[3], float t) {
    float q[3];
    for (int k = 0; k < 3; ++k) {
        const float td = t * d[k];
        const float p = o[k] + td;
        q[k] = p - c.o[k];
    }
    const float cx = (c.r[0] * q[0] + c.r[1] * q[1]) + c.r[2] * q[2];
    const float cy = (c.r[3] * q[0] + c.r[4] * q[1]) + c.r[5] * q[2];
    const float cz = (c.r[6] * q[0] + c.r[7] * q[1]) + c.r[8] * q[2];
    Reprojection rp;
    rp.dist = sqrtf((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]);
    rp.front = cz > 0.0f;
    const float u = (cx / cz) * c.fx + c.cx;
    const float v = (cy / cz) * c.fy + c.cy;
    rp.u0 = floorf(u);
    rp.v0 = floorf(v);
    rp.a = u - rp.u0;
    rp.b = v - rp.v0;
    return rp;
}

// A tap coordinate (u0 + i as a float) lies on an axis of `size` pixels: compared
// in float before any integer conversion, so a NaN or a huge coordinate is outside.
RT_GUIDE_HD inline bool tap_inside(float coord, uint32_t size) {
    return coord >= 0.0f && coord <= static_cast<float>(size - 1u);
}
// the history's pixel at an inside tap shows the same surface: the same sphere, and
// its recorded distance agrees with the point's within depth_tol, relative
RT_GUIDE_HD inline bool tap_same_sphere(uint32_t s, uint32_t s_hist) { return s_hist == s; }
RT_GUIDE_HD inline bool tap_depth_ok(float dist, float t_hist, float depth_tol) {
    return fabsf(dist - t_hist) <= depth_tol * t_hist;
}
RT_GUIDE_HD inline bool tap_accepted(uint32_t s, uint32_t s_hist, float dist, float t_hist, float depth_tol) {
    return tap_same_sphere(s, s_hist) && tap_depth_ok(dist, t_hist, depth_tol);
}
// the bilinear weight of tap (i, j), i and j in {0, 1}
RT_GUIDE_HD inline float tap_weight(int i, int j, float a, float b) {
    const float wx = i ? a : 1.0f - a;
    const float wy = j ? b : 1.0f - b;
    return wx * wy;
}

// the new count of a pixel whose history's count is hc, and the blend of its
// history value hv with this frame's
RT_GUIDE_HD inline float reproject_count(float hc, float max_count) { return fminf(hc + 1.0f, max_count); }
RT_GUIDE_HD inline float reproject_blend(float hv, float cur, float alpha) { return hv + (cur - hv) * alpha; }

// One pixel of the pass on the host (the test dump's; the kernel has its own loop
// over the functions above).  (x, y)'s current hit is {t, s} along d from o; `cur`
// its kC values of this frame.  hist_* are the previous frame's W*H records, or
// hist_hits null for no history.  Writes out[0..kC) and returns the count.
template <uint32_t kC>
RT_GUIDE_HD inline float reproject_pixel(const PrevCamera& c, const float o[3], const float d[3], float t, uint32_t s,
                                         const float cur[kC], uint32_t W, uint32_t H, const uint32_t* hist_hits,
                                         const float* hist_layer, const float* hist_count, float max_count,
                                         float depth_tol, float out[kC]) {
    for (uint32_t ch = 0; ch < kC; ++ch) out[ch] = cur[ch];
    if (s == kReprojectNoHit || !hist_hits) return 1.0f;
    const Reprojection rp = reproject_point(c, o, d, t);
    if (!rp.front) return 1.0f;
    float sw = 0.0f, sc = 0.0f, sv[kC];
    for (uint32_t ch = 0; ch < kC; ++ch) sv[ch] = 0.0f;
    for (int j = 0; j < 2; ++j) {
        const float fv = rp.v0 + static_cast<float>(j);
        if (!tap_inside(fv, H)) continue;
        for (int i = 0; i < 2; ++i) {
            const float fu = rp.u0 + static_cast<float>(i);
            if (!tap_inside(fu, W)) continue;
            const size_t q = static_cast<size_t>(fv) * W + static_cast<size_t>(fu);
            float t_hist;
            const uint32_t t_bits = hist_hits[2 * q];
            __builtin_memcpy(&t_hist, &t_bits, sizeof(t_hist));
            if (!tap_accepted(s, hist_hits[2 * q + 1], rp.dist, t_hist, depth_tol)) continue;
            const float w = tap_weight(i, j, rp.a, rp.b);
            sw += w;
            for (uint32_t ch = 0; ch < kC; ++ch) sv[ch] += w * hist_layer[q * kC + ch];
            sc += w * hist_count[q];
        }
    }
    if (!(sw > 0.0f)) return 1.0f;
    const float n = reproject_count(sc / sw, max_count);
    const float alpha = 1.0f / n;
    for (uint32_t ch = 0; ch < kC; ++ch) out[ch] = reproject_blend(sv[ch] / sw, cur[ch], alpha);
    return n;
}

}  // namespace rtamd
