// rt_gbuffer.hip — first-hit G-buffer of the current camera (rt_render_gbuffer;
// include/rt.h).  The reference has no counterpart: its
// render kernel writes one colour per pixel (src/renderer.cu:57-82).
//
// One pixel per lane: the pixel-centre ray is built in registers
// (Camera::getRay in source order) and walked through the frame kernels' own
// walk<> (rt_walk.h) in its generic mode, the query kernel's: the CPU oracle's
// per-ray results and counters pixel by pixel.  Instead of a colour the lane
// stores its hit {t, sphere}, the hit sphere's normal and its albedo word.
// Compiled like rt_kernels.hip (-ffp-contract=off, IEEE division / sqrt).
#include <hip/hip_runtime.h>

#include "rt_params.h"
#include "rt_query_common.h"
#include "rt_shade.h"  // get_ray: Camera::getRay as rt_pick and the frames' unjittered sample cast it
#include "rt_walk.h"

namespace rtamd {

// rt_gbuffer (include/rt.h) as the kernel writes it; each buffer may be null
struct GBufferArgs {
    uint2* hits;                  // W*H x {t bits, sphere index | kNoHit}
    float4* normals;              // W*H x {n.xyz, 0}
    uint32_t* albedo;             // W*H packed RGBA8
    unsigned long long* counters; // stats launches: 8 lines of kStatLineStride words
};

// A 256-thread block is a 16x16 pixel tile, each of its 4 waves an 8x8 quarter
// (lane = 8 * row + column): a wave's 64 rays are neighbours, and a wave's
// stores are 8 row segments of 64 B (hits), 128 B (normals) and 32 B (albedo).
// FrameArgs leads the argument block (the kernargs() rule of DESIGN.md 5.7):
// a.cam, a.sc, a.W and a.H are set, the rest is zero.  The dynamic LDS is the
// per-lane ancestor stack alone: [level][thread], stack_levels(a.sc) levels.
// (rt_query_common.h holds what is shared; the stack and the flush stay here: a helper moves registers in the stats instances)
template <bool kStats>
__global__ void __launch_bounds__(kBlockThreads) gbuffer_kernel(FrameArgs a, GBufferArgs g) {
    extern __shared__ __attribute__((aligned(16))) float4 lds[];
    uint2* stk = reinterpret_cast<uint2*>(lds) + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t x = blockIdx.x * kTileSide + (wave & 1u) * 8u + (lane & 7u);
    const uint32_t y = blockIdx.y * kTileSide + (wave >> 1) * 8u + (lane >> 3);
    uint32_t n_nodes = 0, n_prims = 0;
    if (x < a.W && y < a.H) {
        float d0, d1, d2;
        get_ray(a.cam, static_cast<float>(x), static_cast<float>(y), d0, d1, d2);
        float t = __builtin_inff();  // a miss reports tmax
        uint32_t ref = kNoHit;
        const bool hit = walk<GenericRay<false, kStats>>(
            a.sc, a.cam.o[0], a.cam.o[1], a.cam.o[2], d0, d1, d2, 0.0f, __builtin_inff(), t, ref,
            n_nodes, n_prims, stk);
        const size_t pix = static_cast<size_t>(y) * a.W + x;
        if (g.hits)  // the caller's sphere index, not the leaf reference
            g.hits[pix] = make_uint2(__float_as_uint(t), hit ? a.sc.prim_idx[ref] : kNoHit);
        if (g.normals) {
            float4 n = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (hit) {
                // hit_shade's operations (rt_kernels.hip) on the record the exact test just read
                const float4 sp = a.sc.prim_sp[ref];
                const float p0 = a.cam.o[0] + t * d0;
                const float p1 = a.cam.o[1] + t * d1;
                const float p2 = a.cam.o[2] + t * d2;
                const float ir = 1.0f / sp.w;
                n.x = (p0 - sp.x) * ir;
                n.y = (p1 - sp.y) * ir;
                n.z = (p2 - sp.z) * ir;
            }
            g.normals[pix] = n;
        }
        if (g.albedo) g.albedo[pix] = hit ? a.sc.prim_al[ref] : 0u;
    }
    if (kStats) {
        // per wave, one 128-byte line per XCD group (query_kernel's layout:
        // words 2 and 3 of a line; the ray count is the host's W * H)
        const unsigned long long s2 = query_wave_sum(n_nodes);
        const unsigned long long s3 = query_wave_sum(n_prims);
        if (lane == 0) {
            const uint32_t b = blockIdx.y * gridDim.x + blockIdx.x;
            unsigned long long* c = g.counters + (b & 7u) * kStatLineStride;
            atomicAdd(c + 2, s2);
            atomicAdd(c + 3, s3);
        }
    }
}

// a.cam, a.sc, a.W, a.H describe the frame; the rest of `a` is unused by the
// kernel.  counters != null: a stats launch (the caller zeroed its 8 lines).
hipError_t launch_gbuffer(const FrameArgs& a, void* hits, void* normals, void* albedo,
                          unsigned long long* counters, hipStream_t st) {
    if (a.W == 0 || a.H == 0) return hipSuccess;
    GBufferArgs g;
    g.hits = static_cast<uint2*>(hits);
    g.normals = static_cast<float4*>(normals);
    g.albedo = static_cast<uint32_t*>(albedo);
    g.counters = counters;
    const dim3 grid((a.W + kTileSide - 1u) / kTileSide, (a.H + kTileSide - 1u) / kTileSide);
    const dim3 block(kBlockThreads);
    const size_t lds = query_stack_bytes(stack_levels(a.sc));
    if (counters) hipLaunchKernelGGL((gbuffer_kernel<true>), grid, block, lds, st, a, g);
    else hipLaunchKernelGGL((gbuffer_kernel<false>), grid, block, lds, st, a, g);
    return hipGetLastError();
}

}  // namespace rtamd
