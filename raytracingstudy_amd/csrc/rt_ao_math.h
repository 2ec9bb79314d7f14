// rt_ao_math.h — the ambient-occlusion layer's arithmetic (rt_render_ao;
// include/rt.h), free of HIP and of the renderer's state: the
// call's validity, the hash words of a ray and the cosine-weighted direction
// about a normal.  Integer operations mod 2^32 and f32 operations in a fixed
// order (built with -ffp-contract=off like the rest, IEEE sqrtf and division),
// no transcendental: rt_ao.hip runs it per lane on the device, and
// tests/native/ao_math_dump.cpp prints it for tests/test_ao_cpu.py, which holds
// it to tests/ao_ref.py's numpy restatement bit for bit.
#pragma once
#include "rt_guide_math.h"

namespace rtamd {

constexpr uint32_t kAoMaxRays = 64;          // a wave's lanes: one pixel's rays are one ballot
constexpr uint32_t kAoTries = 8;             // candidates of a direction before it falls back to n
constexpr float kAoMinLen2 = 1.0f / 1048576.0f;  // 2^-20: the least |c|^2 and |n + s|^2 normalised
// the salt's own word and the three axes' words (the golden ratio and murmur3's finalizer constants)
constexpr uint32_t kAoSaltWord = 0x85EBCA6Bu;
constexpr uint32_t kAoAxisX = 0x9E3779B9u, kAoAxisY = 0x85EBCA6Bu, kAoAxisZ = 0xC2B2AE35u;

// rays per hit pixel: a power of two up to the wave, so that 1.0f / rays and
// (rays - occluded) * (1.0f / rays) are exact
RT_GUIDE_HD inline bool ao_rays_ok(uint32_t rays) {
    return rays >= 1u && rays <= kAoMaxRays && (rays & (rays - 1u)) == 0u;
}
// radius > 0, +inf allowed (a NaN fails the comparison)
RT_GUIDE_HD inline bool ao_radius_ok(float radius) { return radius > 0.0f; }

// the frames' hash and its map to [0, 1) (rt_shade.h mix32 / u01), restated
// for the host
RT_GUIDE_HD inline uint32_t ao_mix32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}
RT_GUIDE_HD inline float ao_u01(uint32_t x) { return static_cast<float>(x >> 8) * (1.0f / 16777216.0f); }

// The call's key: seedmix is the frames' mix32(seed ^ 0x9E3779B9).  mix32 is a
// bijection, so two salts never share a key.
RT_GUIDE_HD inline uint32_t ao_key(uint32_t seedmix, uint32_t salt) {
    return ao_mix32(seedmix ^ ao_mix32(salt ^ kAoSaltWord));
}
// a pixel's word (pid = y * W + x), as the frames' hp
RT_GUIDE_HD inline uint32_t ao_pixel_word(uint32_t key, uint32_t pid) { return ao_mix32(key ^ pid); }
// the word of ray i's candidate `attempt` (i < 64, attempt < 8: nine bits)
RT_GUIDE_HD inline uint32_t ao_try_word(uint32_t hp, uint32_t i, uint32_t attempt) {
    return ao_mix32(hp ^ ((i << 3) | attempt));
}
// one coordinate of the candidate in [-1, 1): 2 * u01 - 1 is exact in f32
RT_GUIDE_HD inline float ao_cube(uint32_t hb, uint32_t axis_word) {
    return 2.0f * ao_u01(ao_mix32(hb ^ axis_word)) - 1.0f;
}

// Direction i of a pixel about the normal n: a point s uniform on the unit
// sphere (the first of up to 8 candidates c of the cube with 2^-20 <= |c|^2 <=
// 1, divided by its length), then (n + s) / |n + s|: cosine-weighted about n.
// No candidate accepted, or |n + s|^2 < 2^-20 (s opposite n): the normal itself.
// Returns whether the direction is that fallback.
RT_GUIDE_HD inline bool ao_direction(uint32_t hp, uint32_t i, float n0, float n1, float n2, float& d0, float& d1,
                                     float& d2) {
    d0 = n0;
    d1 = n1;
    d2 = n2;
    for (uint32_t attempt = 0; attempt < kAoTries; ++attempt) {
        const uint32_t hb = ao_try_word(hp, i, attempt);
        const float c0 = ao_cube(hb, kAoAxisX), c1 = ao_cube(hb, kAoAxisY), c2 = ao_cube(hb, kAoAxisZ);
        const float q = (c0 * c0 + c1 * c1) + c2 * c2;
        if (q >= kAoMinLen2 && q <= 1.0f) {
            const float len = sqrtf(q);
            const float w0 = n0 + c0 / len;
            const float w1 = n1 + c1 / len;
            const float w2 = n2 + c2 / len;
            const float q2 = (w0 * w0 + w1 * w1) + w2 * w2;
            if (!(q2 >= kAoMinLen2)) return true;
            const float l2 = sqrtf(q2);
            d0 = w0 / l2;
            d1 = w1 / l2;
            d2 = w2 / l2;
            return false;
        }
    }
    return true;
}

}  // namespace rtamd
