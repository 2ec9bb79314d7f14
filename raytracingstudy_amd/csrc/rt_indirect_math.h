// rt_indirect_math.h — the one-bounce diffuse layer's arithmetic
// (rt_render_indirect, rt_add_layer; include/rt.h), free of HIP
// and of the renderer's state: the call's validity, what a bounce ray brings
// back (the frames' miss colour of an escaped ray, the frames' shading of a hit),
// the ordered sum of a pixel's rays, and a layer's pixel added into an RGBA8
// pixel.  The rays themselves are rt_ao_math.h's.  f32 operations in a fixed order
// (built with -ffp-contract=off like the rest), no transcendental:
// rt_indirect.hip and rt_filter.hip run it per lane on the device, and
// tests/native/indirect_math_dump.cpp prints it for tests/test_indirect_cpu.py,
// which holds it to tests/indirect_ref.py's numpy restatement bit for bit.
#pragma once
#include "rt_ao_math.h"

namespace rtamd {

// sky_scale and rt_add_layer's gain: finite and >= 0 (a NaN fails the first comparison)
RT_GUIDE_HD inline bool indirect_scale_ok(float s) { return s >= 0.0f && finite_f32(s); }
// rt_indirect_params (include/rt.h) field by field: rays and radius as rt_render_ao's
RT_GUIDE_HD inline bool indirect_params_ok(uint32_t rays, float radius, float sky_scale, uint32_t flags) {
    return ao_rays_ok(rays) && ao_radius_ok(radius) && indirect_scale_ok(sky_scale) && flags == 0u;
}

// the frames' sat (rt_shade.h), restated for the host
RT_GUIDE_HD inline float indirect_sat(float x) { return x > 0.0f ? (x < 1.0f ? x : 1.0f) : 0.0f; }

// An escaped ray of direction d: the frames' miss colour {200/255, sat(d.y),
// sat(d.z)}, then one multiply each.
RT_GUIDE_HD inline void indirect_sky(float dy, float dz, float sky_scale, float c[3]) {
    c[0] = (200.0f / 255.0f) * sky_scale;
    c[1] = indirect_sat(dy) * sky_scale;
    c[2] = indirect_sat(dz) * sky_scale;
}

// A hit of albedo word `al` under the Lambert term `lam` (0 facing away or
// shadowed): the frames' f = ambient + (1 - ambient) * lam and their three bytes
// (rt_shade.h sample_color_unified, same operands in the same order).
RT_GUIDE_HD inline void indirect_hit_color(uint32_t al, float ambient, float lam, float c[3]) {
    const float f = ambient + (1.0f - ambient) * lam;
    c[0] = static_cast<float>(al & 0xFFu) * (1.0f / 255.0f) * f;
    c[1] = static_cast<float>((al >> 8) & 0xFFu) * (1.0f / 255.0f) * f;
    c[2] = static_cast<float>((al >> 16) & 0xFFu) * (1.0f / 255.0f) * f;
}

// One step of the ordered sum, as lane i sees it: v[i] + v[i ^ m].  The kernel's
// partner comes from __shfl_xor; indirect_tree_sum below runs every lane.
RT_GUIDE_HD inline float indirect_pair(float mine, float partner) { return mine + partner; }
// tree_sum's pairing (rt_shade.h) over a pixel's `rays` values, in place: for
// m = 1, 2, 4, .. < rays every v[i] becomes v[i] + v[i ^ m]; v[0] is the sum.
inline void indirect_tree_sum(float* v, uint32_t rays) {
    float w[kAoMaxRays];
    for (uint32_t m = 1; m < rays; m <<= 1) {
        for (uint32_t i = 0; i < rays; ++i) w[i] = indirect_pair(v[i], v[i ^ m]);
        for (uint32_t i = 0; i < rays; ++i) v[i] = w[i];
    }
}
// the layer's pixel of a summed colour and the count of rays that hit: exact
// scales (rays is a power of two); w has rt_render_ao's dev_ao bits
RT_GUIDE_HD inline float indirect_mean(float sum, uint32_t rays) { return sum * (1.0f / static_cast<float>(rays)); }
RT_GUIDE_HD inline float indirect_open(uint32_t rays, uint32_t hits) {
    return static_cast<float>(rays - hits) * (1.0f / static_cast<float>(rays));
}

// rt_add_layer's pixel: each of R, G and B of the frame's word `px` plus the
// layer's channel times gain (times the albedo byte / 255 where there is an
// albedo), truncated like the frames' conversion; a NaN stores 0; A is kept.
RT_GUIDE_HD inline uint32_t add_layer_channel(uint32_t c, uint32_t a, bool has_albedo, float gain, float layer) {
    const float k = has_albedo ? static_cast<float>(a) * (1.0f / 255.0f) : 1.0f;
    const float v = static_cast<float>(c) + ((k * gain) * layer) * 255.0f;
    return static_cast<uint32_t>(fminf(fmaxf(v, 0.0f), 255.0f));
}
RT_GUIDE_HD inline uint32_t add_layer_pixel(uint32_t px, const float layer[3], uint32_t al, bool has_albedo,
                                            float gain) {
    return add_layer_channel(px & 0xFFu, al & 0xFFu, has_albedo, gain, layer[0]) |
           (add_layer_channel((px >> 8) & 0xFFu, (al >> 8) & 0xFFu, has_albedo, gain, layer[1]) << 8) |
           (add_layer_channel((px >> 16) & 0xFFu, (al >> 16) & 0xFFu, has_albedo, gain, layer[2]) << 16) |
           (px & 0xFF000000u);
}

}  // namespace rtamd
