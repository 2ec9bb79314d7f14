// rt_ao.hip — the ambient-occlusion layer of the current camera (rt_render_ao;
// include/rt.h).  The reference has no counterpart: its render
// kernel writes one colour per pixel (src/renderer.cu:57-82).
//
// A wave owns 64 / rays pixels x rays lanes, the frames' ppw x spw mapping
// (rt_shade.h): lane l works on pixel l / rays of the wave's tile, ray l % rays.
// Every lane of a pixel's group builds the pixel-centre ray in registers
// (Camera::getRay in source order) and walks it through the frame kernels' own
// walk<> (rt_walk.h) in its generic mode, as rt_gbuffer.hip does: the rays of a
// group are identical, so its lanes walk together.  Each lane of a hit pixel then
// builds its own direction about the hit's normal (rt_ao_math.h) from the frames'
// shadow-ray origin and walks it any-hit up to the caller's radius; the pixel's
// count is a popcount of the wave's ballot under the group's aligned mask, and
// the group's first lane stores it.  Nothing but the ancestor stack is in LDS.
// Compiled like rt_gbuffer.hip (-ffp-contract=off, IEEE division / sqrt).
#include <hip/hip_runtime.h>

#include "rt_ao_math.h"
#include "rt_params.h"
#include "rt_query_common.h"
#include "rt_shade.h"  // get_ray: Camera::getRay as rt_pick and the frames' unjittered sample cast it
#include "rt_walk.h"

namespace rtamd {

// rt_ao_out (include/rt.h) as the kernel writes it, and the call's parameters
struct AoArgs {
    float* ao;                    // W*H, or null
    uint32_t* occluded;           // W*H, or null
    unsigned long long* counters; // stats launches: 8 lines of kStatLineStride words
    uint32_t key;                 // ao_key(seedmix, salt)
    uint32_t lg;                  // log2(rays), 0..6
    float radius;                 // every AO ray's tmax
};

// A wave's tile is 2^twl x 2^thl pixels, twl = (7 - lg) / 2, thl = (6 - lg) / 2:
// 8x8 at one ray a pixel, then 8x4, 4x4, 4x2, 2x2, 2x1 and one pixel at 64; a
// block's 4 waves are a 2x2 arrangement of such tiles (launch_ao's grid).
// FrameArgs leads the argument block (the kernargs() rule of DESIGN.md 5.7):
// a.cam, a.sc, a.W and a.H are set, the rest is zero.  The dynamic LDS is the
// per-lane ancestor stack alone: [level][thread], stack_levels(a.sc) levels; the
// two walks of a lane use it one after the other.
// (rt_query_common.h holds what is shared; the stack and the flush stay here: a helper moves registers in the stats instances)
template <bool kStats>
__global__ void __launch_bounds__(kBlockThreads) ao_kernel(FrameArgs a, AoArgs g) {
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
    bool cast = false, occluded = false;
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
            // the frames' shadow-ray construction (rt_shade.h sample_color_unified) on
            // the record the exact test just read
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
            float ta = g.radius;
            uint32_t ra = kNoHit;
            occluded = walk<GenericRay<true, kStats>>(a.sc, o0, o1, o2, d0, d1, d2, 0.0f, g.radius, ta, ra,
                                                      n_nodes, n_prims, stk);
        }
    }
    // the group's lanes are `rays` neighbours starting at a multiple of `rays`
    const unsigned long long ones = lg == 6u ? ~0ull : (1ull << (1u << lg)) - 1ull;
    const unsigned long long occ_wave = __ballot(occluded);
    const uint32_t count = static_cast<uint32_t>(__popcll(occ_wave & (ones << (lane & ~sub_mask))));
    if (in_image && sub == 0u) {
        const size_t at = static_cast<size_t>(y) * a.W + x;
        const uint32_t rays = 1u << lg;
        // exact: rays is a power of two (a miss pixel counted 0: 1.0f)
        if (g.ao) g.ao[at] = static_cast<float>(rays - count) * (1.0f / static_cast<float>(rays));
        if (g.occluded) g.occluded[at] = count;
    }
    if (kStats) {
        // per wave, one 128-byte line per XCD group (query_kernel's layout: the AO
        // rays cast in word 1, nodes and tests in words 2 and 3; the primary
        // ray count is the host's W * H)
        const unsigned long long s1 = static_cast<unsigned long long>(__popcll(__ballot(cast)));
        const unsigned long long s2 = query_wave_sum(n_nodes);
        const unsigned long long s3 = query_wave_sum(n_prims);
        if (lane == 0) {
            const uint32_t b = blockIdx.y * gridDim.x + blockIdx.x;
            unsigned long long* c = g.counters + (b & 7u) * kStatLineStride;
            atomicAdd(c + 1, s1);
            atomicAdd(c + 2, s2);
            atomicAdd(c + 3, s3);
        }
    }
}

// a.cam, a.sc, a.W, a.H describe the frame; the rest of `a` is unused by the
// kernel.  rays: ao_rays_ok (the caller checked).  counters != null: a stats
// launch (the caller zeroed its 8 lines).
hipError_t launch_ao(const FrameArgs& a, void* ao, void* occluded, uint32_t rays, float radius, uint32_t key,
                     unsigned long long* counters, hipStream_t st) {
    if (a.W == 0 || a.H == 0) return hipSuccess;
    AoArgs g;
    g.ao = static_cast<float*>(ao);
    g.occluded = static_cast<uint32_t*>(occluded);
    g.counters = counters;
    g.key = key;
    g.lg = 0;
    while ((1u << g.lg) < rays) ++g.lg;
    g.radius = radius;
    // a block's tile: 2 x 2 wave tiles
    const uint32_t bw = 2u << ((7u - g.lg) >> 1), bh = 2u << ((6u - g.lg) >> 1);
    const dim3 grid((a.W + bw - 1u) / bw, (a.H + bh - 1u) / bh);
    const dim3 block(kBlockThreads);
    const size_t lds = query_stack_bytes(stack_levels(a.sc));
    if (counters) hipLaunchKernelGGL((ao_kernel<true>), grid, block, lds, st, a, g);
    else hipLaunchKernelGGL((ao_kernel<false>), grid, block, lds, st, a, g);
    return hipGetLastError();
}

}  // namespace rtamd
