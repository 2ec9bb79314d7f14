// rt_indirect.hip — the one-bounce diffuse light layer of the current camera
// (rt_render_indirect; include/rt.h).  The reference has no
// counterpart: its render kernel writes one colour per pixel (src/renderer.cu:57-82).
//
// rt_ao.hip's mapping and rays with another payload: a wave owns 64 / rays pixels
// x rays lanes, every lane of a pixel's group walks the pixel-centre ray, then
// each lane of a hit pixel walks its own direction about the hit's normal
// (rt_ao_math.h), here to the NEAREST hit.  A lane whose ray hit shades that hit
// as a frame shades a primary hit (rt_shade.h sample_color_unified: Lambert, one
// any-hit shadow ray along the frame's L, the constant ambient term); a lane whose
// ray escaped brings the frames' miss colour times sky_scale.  Between the walks a
// lane keeps the hit's albedo word, its Lambert term, the shadow origin and d.y /
// d.z for the sky.  The group's colours are summed by tree_sum's pairing over
// __shfl_xor, the hits counted by a popcount of the wave's ballot under the
// group's mask, and the group's first lane stores the pixel.  Nothing but the
// ancestor stack is in LDS; the three walks of a lane use it one after another.
// Compiled like rt_ao.hip (-ffp-contract=off, IEEE division / sqrt).
#include <hip/hip_runtime.h>

#include "rt_indirect_math.h"
#include "rt_params.h"
#include "rt_query_common.h"
#include "rt_shade.h"  // get_ray: Camera::getRay as rt_pick and the frames' unjittered sample cast it
#include "rt_walk.h"

namespace rtamd {

// rt_indirect_out (include/rt.h) as the kernel writes it, and the call's parameters
struct IndirectArgs {
    float4* layer;                // W*H x {r, g, b, open share}, or null
    uint32_t* occluded;           // W*H, or null
    unsigned long long* counters; // stats launches: 8 lines of kStatLineStride words
    uint32_t key;                 // ao_key(seedmix, salt)
    uint32_t lg;                  // log2(rays), 0..6
    float radius;                 // every bounce ray's tmax
    float sky_scale;              // what an escaped ray brings, times the frames' miss colour
};

// The wave tile, the block's 2 x 2 wave tiles and the dynamic LDS are ao_kernel's
// (rt_ao.hip).  FrameArgs leads the argument block (the kernargs() rule of
// DESIGN.md 5.7): a.cam, a.sc (with prim_al), a.W, a.H and the frames' shading
// fields a.L, a.ambient and a.shadows are set, the rest is zero.
// (rt_query_common.h holds what is shared; the stack and the flush stay here: a helper moves registers in the stats instances)
template <bool kStats>
__global__ void __launch_bounds__(kBlockThreads) indirect_kernel(FrameArgs a, IndirectArgs g) {
    extern __shared__ __attribute__((aligned(16))) float4 lds[];
    uint2* stk = reinterpret_cast<uint2*>(lds) + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t lg = g.lg, twl = (7u - lg) >> 1, thl = (6u - lg) >> 1;
    const uint32_t sub_mask = (1u << lg) - 1u;
    const uint32_t pix = lane >> lg, sub = lane & sub_mask;
    const uint32_t x = ((blockIdx.x * 2u + (wave & 1u)) << twl) + (pix & ((1u << twl) - 1u));
    const uint32_t y = ((blockIdx.y * 2u + (wave >> 1)) << thl) + (pix >> twl);
    // a group that starts past the image is skipped whole (its lanes share x and y)
    const bool in_image = x < a.W && y < a.H;
    uint32_t n_nodes = 0, n_prims = 0;
    bool cast = false, hit = false, want = false;
    // what a lane keeps of its bounce ray: the hit's albedo word, Lambert term and
    // shadow-ray origin, or the direction's y and z for the sky
    uint32_t al = 0;
    float lam = 0.0f, sky_y = 0.0f, sky_z = 0.0f;
    float r0 = 0.0f, r1 = 0.0f, r2 = 0.0f;
    if (in_image) {
        float d0, d1, d2;
        get_ray(a.cam, static_cast<float>(x), static_cast<float>(y), d0, d1, d2);
        float t = __builtin_inff();
        uint32_t ref = kNoHit;
        cast = walk<GenericRay<false, kStats>>(a.sc, a.cam.o[0], a.cam.o[1], a.cam.o[2], d0, d1, d2, 0.0f,
                                               __builtin_inff(), t, ref, n_nodes, n_prims, stk);
        // the primary walk counts once per pixel: the group's first lane's
        if (kStats && sub != 0u) n_nodes = n_prims = 0;
        if (cast) {
            // rt_ao.hip's ray: the frames' shadow-ray origin and ao_direction about the normal
            const float4 sp = a.sc.prim_sp[ref];
            const float p0 = a.cam.o[0] + t * d0;
            const float p1 = a.cam.o[1] + t * d1;
            const float p2 = a.cam.o[2] + t * d2;
            const float ir = 1.0f / sp.w;
            const float n0 = (p0 - sp.x) * ir;
            const float n1 = (p1 - sp.y) * ir;
            const float n2 = (p2 - sp.z) * ir;
            const float o0 = p0 + n0 * kShadowEps;
            const float o1 = p1 + n1 * kShadowEps;
            const float o2 = p2 + n2 * kShadowEps;
            ao_direction(ao_pixel_word(g.key, y * a.W + x), sub, n0, n1, n2, d0, d1, d2);
            sky_y = d1;
            sky_z = d2;
            float t2 = g.radius;
            uint32_t ref2 = kNoHit;
            hit = walk<GenericRay<false, kStats>>(a.sc, o0, o1, o2, d0, d1, d2, 0.0f, g.radius, t2, ref2, n_nodes,
                                                  n_prims, stk);
            if (hit) {
                // the frames' shading prep (sample_color_unified) on the bounce hit
                const float4 s2 = a.sc.prim_sp[ref2];
                al = a.sc.prim_al[ref2];
                const float q0 = o0 + t2 * d0;
                const float q1 = o1 + t2 * d1;
                const float q2 = o2 + t2 * d2;
                const float ir2 = 1.0f / s2.w;
                const float m0 = (q0 - s2.x) * ir2;
                const float m1 = (q1 - s2.y) * ir2;
                const float m2 = (q2 - s2.z) * ir2;
                const float ndl = m0 * a.L[0] + m1 * a.L[1] + m2 * a.L[2];
                lam = ndl > 0.0f ? ndl : 0.0f;
                want = ndl > 0.0f && a.shadows;
                r0 = q0 + m0 * kShadowEps;
                r1 = q1 + m1 * kShadowEps;
                r2 = q2 + m2 * kShadowEps;
            }
        }
    }
    // the shadow rays of the lit hits: the frame's L in every lane, read afresh
    // from the kernel arguments; a wave without one skips the walk whole
    const unsigned long long want_wave = __ballot(want);
    if (want_wave != 0ull) {
        if (want) {
            KernArgs* kl = kernargs();
            float ts = __builtin_inff();
            uint32_t rs = kNoHit;
            if (walk<GenericRay<true, kStats>>(a.sc, r0, r1, r2, kl->L[0], kl->L[1], kl->L[2], 0.0f, __builtin_inff(),
                                               ts, rs, n_nodes, n_prims, stk))
                lam = 0.0f;
        }
    }
    // this lane's ray (a lane that cast nothing adds zeros, and only to its own group)
    float c[3] = {0.0f, 0.0f, 0.0f};
    if (hit) indirect_hit_color(al, kernargs()->ambient, lam, c);
    else if (cast) indirect_sky(sky_y, sky_z, g.sky_scale, c);
    // tree_sum's pairing over the group's lanes, `rays` neighbours starting at a multiple of `rays`
    for (uint32_t m = 1u; m <= sub_mask; m <<= 1) {
        c[0] = indirect_pair(c[0], __shfl_xor(c[0], static_cast<int>(m), 64));
        c[1] = indirect_pair(c[1], __shfl_xor(c[1], static_cast<int>(m), 64));
        c[2] = indirect_pair(c[2], __shfl_xor(c[2], static_cast<int>(m), 64));
    }
    const unsigned long long ones = lg == 6u ? ~0ull : (1ull << (1u << lg)) - 1ull;
    const unsigned long long hit_wave = __ballot(hit);
    const uint32_t count = static_cast<uint32_t>(__popcll(hit_wave & (ones << (lane & ~sub_mask))));
    if (in_image && sub == 0u) {
        const size_t at = static_cast<size_t>(y) * a.W + x;
        const uint32_t rays = 1u << lg;
        // (a miss pixel summed zeros and counted 0: {0, 0, 0, 1.0f})
        if (g.layer)
            g.layer[at] = make_float4(indirect_mean(c[0], rays), indirect_mean(c[1], rays), indirect_mean(c[2], rays),
                                      indirect_open(rays, count));
        if (g.occluded) g.occluded[at] = count;
    }
    if (kStats) {
        // per wave, one 128-byte line per XCD group (ao_kernel's layout: the bounce
        // rays and the shadow rays cast in word 1, nodes and tests in words 2 and 3;
        // the primary ray count is the host's W * H)
        const unsigned long long s1 =
            static_cast<unsigned long long>(__popcll(__ballot(cast))) + static_cast<unsigned long long>(__popcll(want_wave));
        const unsigned long long s2 = query_wave_sum(n_nodes);
        const unsigned long long s3 = query_wave_sum(n_prims);
        if (lane == 0) {
            const uint32_t b = blockIdx.y * gridDim.x + blockIdx.x;
            unsigned long long* ctr = g.counters + (b & 7u) * kStatLineStride;
            atomicAdd(ctr + 1, s1);
            atomicAdd(ctr + 2, s2);
            atomicAdd(ctr + 3, s3);
        }
    }
}

// a.cam, a.sc (prim_al made), a.W, a.H, a.L, a.ambient and a.shadows describe the
// frame; the rest of `a` is unused by the kernel.  rays: ao_rays_ok (the caller
// checked).  counters != null: a stats launch (the caller zeroed its 8 lines).
hipError_t launch_indirect(const FrameArgs& a, void* layer, void* occluded, uint32_t rays, float radius, uint32_t key,
                           float sky_scale, unsigned long long* counters, hipStream_t st) {
    if (a.W == 0 || a.H == 0) return hipSuccess;
    IndirectArgs g;
    g.layer = static_cast<float4*>(layer);
    g.occluded = static_cast<uint32_t*>(occluded);
    g.counters = counters;
    g.key = key;
    g.lg = 0;
    while ((1u << g.lg) < rays) ++g.lg;
    g.radius = radius;
    g.sky_scale = sky_scale;
    // a block's tile: 2 x 2 wave tiles
    const uint32_t bw = 2u << ((7u - g.lg) >> 1), bh = 2u << ((6u - g.lg) >> 1);
    const dim3 grid((a.W + bw - 1u) / bw, (a.H + bh - 1u) / bh);
    const dim3 block(kBlockThreads);
    const size_t lds = query_stack_bytes(stack_levels(a.sc));
    if (counters) hipLaunchKernelGGL((indirect_kernel<true>), grid, block, lds, st, a, g);
    else hipLaunchKernelGGL((indirect_kernel<false>), grid, block, lds, st, a, g);
    return hipGetLastError();
}

}  // namespace rtamd
