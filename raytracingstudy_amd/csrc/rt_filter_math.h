// rt_filter_math.h — the guide-driven layer filter's arithmetic and plan
// (rt_filter_layer; include/rt.h), free of HIP and of the
// renderer's state: the call's validity, one tap's weight, and which buffer each
// pass reads and writes.  f32 operations in a fixed order (built with
// -ffp-contract=off like the rest, IEEE division), no transcendental:
// rt_filter.hip runs it per lane on the device, and
// tests/native/filter_math_dump.cpp prints it for tests/test_filter_cpu.py, which
// holds it to tests/filter_ref.py's numpy restatement bit for bit.
#pragma once
#include "rt_guide_math.h"

namespace rtamd {

constexpr uint32_t kFilterMaxPasses = 5;       // tap spacing 1, 2, 4, 8, 16
constexpr uint32_t kFilterMaxNormalPower = 7;  // exponent 2^7 = 128
constexpr int kFilterReach = 2;                // taps -2..2 on each axis: 25 a pixel

// rt_filter_params (include/rt.h) field by field; a NaN depth_sigma fails the comparison
RT_GUIDE_HD inline bool filter_passes_ok(uint32_t passes) { return passes >= 1u && passes <= kFilterMaxPasses; }
RT_GUIDE_HD inline bool filter_channels_ok(uint32_t channels) { return channels == 1u || channels == 4u; }
RT_GUIDE_HD inline bool filter_depth_sigma_ok(float depth_sigma) { return depth_sigma > 0.0f; }
RT_GUIDE_HD inline bool filter_normal_power_ok(uint32_t normal_power) { return normal_power <= kFilterMaxNormalPower; }
RT_GUIDE_HD inline bool filter_params_ok(uint32_t passes, uint32_t channels, float depth_sigma, uint32_t normal_power,
                                         uint32_t flags) {
    return filter_passes_ok(passes) && filter_channels_ok(channels) && filter_depth_sigma_ok(depth_sigma) &&
           filter_normal_power_ok(normal_power) && flags == 0u;
}
// rt_apply_layer's floor: in [0, 1] (a NaN fails both comparisons)
RT_GUIDE_HD inline bool apply_floor_ok(float floor) { return floor >= 0.0f && floor <= 1.0f; }

// The B3-spline row {1, 4, 6, 4, 1} / 16 by distance from the centre; a tap's k
// is the product of its column's and its row's entry (exact: powers of two and 3).
RT_GUIDE_HD inline float filter_tap_k(int offset) {
    const int a = offset < 0 ? -offset : offset;
    return a == 0 ? 0.375f : a == 1 ? 0.25f : 0.0625f;
}

// A pixel's depth scale, once per pixel: depth_sigma = +inf gives 0 for every
// t_p > 0, and the depth term below is then 1 for every tap.
RT_GUIDE_HD inline float filter_inv_depth(float depth_sigma, float t_p) { return 1.0f / (depth_sigma * t_p); }

// The weight of tap q as seen from pixel p: the kernel entry k, the normals'
// agreement max(n_p.n_q, 0)^(2^normal_power) by repeated squaring, and the
// relative depth difference through 1 / (1 + e^2).
RT_GUIDE_HD inline float filter_weight(float k, const float n_p[3], const float n_q[3], float t_p, float t_q, float iz,
                                       uint32_t normal_power) {
    const float dn = (n_p[0] * n_q[0] + n_p[1] * n_q[1]) + n_p[2] * n_q[2];
    float wn = fmaxf(dn, 0.0f);
    for (uint32_t u = 0; u < normal_power; ++u) wn = wn * wn;
    const float e = (t_q - t_p) * iz;
    const float wz = 1.0f / (1.0f + e * e);
    return (k * wn) * wz;
}

// The pass and buffer plan.  Pass s (0-based) uses tap spacing 1 << s.  The
// caller's input is never written; the handle's one scratch layer and the
// caller's output alternate so that the last pass writes the output whatever the
// parity of `passes`: pass s writes the output iff passes - 1 - s is even, and
// reads what pass s - 1 wrote (pass 0: the input).
enum FilterBuf : uint32_t { kFilterIn = 0, kFilterOut = 1, kFilterScratch = 2 };
RT_GUIDE_HD inline uint32_t filter_pass_step(uint32_t s) { return 1u << s; }
RT_GUIDE_HD inline FilterBuf filter_pass_dst(uint32_t s, uint32_t passes) {
    return ((passes - 1u - s) & 1u) == 0u ? kFilterOut : kFilterScratch;
}
RT_GUIDE_HD inline FilterBuf filter_pass_src(uint32_t s, uint32_t passes) {
    return s == 0u ? kFilterIn : filter_pass_dst(s - 1u, passes);
}
// whether the plan touches the scratch layer at all
RT_GUIDE_HD inline bool filter_needs_scratch(uint32_t passes) { return passes >= 2u; }

}  // namespace rtamd
