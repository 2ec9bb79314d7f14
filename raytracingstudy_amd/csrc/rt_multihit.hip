// rt_multihit.hip — ordered multi-hit ray queries (rt_trace_rays_multi,
// rt_pick_multi; include/rt.h): the k nearest spheres along each
// ray, by (t, then the caller's sphere index).  The reference has no
// counterpart (Octree::traverse is a stub, include/octree.h:19-21).
//
// One caller-supplied ray per lane through walk<> (rt_walk.h) in its generic
// mode with a MultiHits<K> buffer: the frames' plane(), isect and step rules,
// the nearest rule's bound taken from the buffer's last entry.  Compiled like
// rt_query.hip (-ffp-contract=off, IEEE division / sqrt).
#include <hip/hip_runtime.h>

#include "rt_params.h"
#include "rt_query_common.h"
#include "rt_walk.h"

namespace rtamd {

struct MultiQueryArgs {
    const float4* rays;            // n x {origin.xyz, tmin}, {dir.xyz, tmax}
    uint2* hits;                   // n x k x {t bits, sphere index | kNoHit}, ray-major
    uint32_t* counts;              // n, or null
    uint32_t n;
    uint32_t k;                    // the caller's k: 1 <= k <= K
    unsigned long long* counters;  // stats launches: 8 lines of kStatLineStride words
};

// One ray per lane, 256-thread blocks, the K-entry buffer in registers (K is
// the caller's k rounded up to a compiled size: the walk keeps the K nearest
// and the lane writes the first k of them, so slots, fillers and counts are
// exact for k).  A ray is two coalesced dwordx4 loads, its hits k dwordx2
// stores.  FrameArgs leads the argument block for rt_query.hip's reason:
// kernargs() reinterprets the argument segment as FrameArgs.  The dynamic LDS
// is the per-lane ancestor stack alone, [level][thread].
// (rt_query_common.h holds what is shared; the stack and the flush stay here: a helper moves registers in the stats instances)
template <int K, bool kStats>
__global__ void __launch_bounds__(kBlockThreads) multihit_kernel(FrameArgs a, MultiQueryArgs q) {
    extern __shared__ __attribute__((aligned(16))) float4 lds[];
    uint2* stk = reinterpret_cast<uint2*>(lds) + threadIdx.x;
    const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
    uint32_t n_nodes = 0, n_prims = 0;
    if (i < q.n) {
        const float4 r0 = q.rays[2u * static_cast<size_t>(i)];
        const float4 r1 = q.rays[2u * static_cast<size_t>(i) + 1u];
        MultiHits<K> mh;
        mh.clear(r1.w);  // a free slot reports the ray's tmax
        float t_unused = 0.0f;
        uint32_t ref_unused = kNoHit;
        walk<MultiHitRay<K, kStats>>(
            a.sc, r0.x, r0.y, r0.z, r1.x, r1.y, r1.z, r0.w, r1.w, t_unused, ref_unused, n_nodes,
            n_prims, stk, false, nullptr, ~0u, &mh);
        uint2* out = q.hits + static_cast<size_t>(i) * q.k;
        uint32_t count = 0;
#pragma unroll
        for (int s = 0; s < K; ++s) {
            if (static_cast<uint32_t>(s) < q.k) {
                const bool hit = mh.ref[s] != kNoHit;
                // the caller's sphere index, not the leaf reference
                const uint32_t sphere = hit ? a.sc.prim_idx[mh.ref[s]] : kNoHit;
                out[s] = make_uint2(__float_as_uint(mh.t[s]), sphere);
                count += hit ? 1u : 0u;
            }
        }
        if (q.counts) q.counts[i] = count;
    }
    if (kStats) {
        // rt_query.hip's layout: words 2 and 3 of one line per XCD group
        const unsigned long long s2 = query_wave_sum(n_nodes);
        const unsigned long long s3 = query_wave_sum(n_prims);
        if ((threadIdx.x & 63u) == 0) {
            unsigned long long* c = q.counters + (blockIdx.x & 7u) * kStatLineStride;
            atomicAdd(c + 2, s2);
            atomicAdd(c + 3, s3);
        }
    }
}

// a.sc is the scene; the rest of `a` is unused by the kernel (see above).
// 1 <= k <= 16 (the caller checked); counts may be null; counters != null: a
// stats launch (the caller zeroed its 8 lines).
hipError_t launch_multihit(const FrameArgs& a, const void* rays, void* hits, void* counts, uint32_t n,
                           uint32_t k, unsigned long long* counters, hipStream_t st) {
    if (n == 0) return hipSuccess;
    if (k == 0 || k > 16u) return hipErrorInvalidValue;
    MultiQueryArgs q;
    q.rays = static_cast<const float4*>(rays);
    q.hits = static_cast<uint2*>(hits);
    q.counts = static_cast<uint32_t*>(counts);
    q.n = n;
    q.k = k;
    q.counters = counters;
    const dim3 grid = query_grid(n), block(kBlockThreads);
    const size_t lds = query_stack_bytes(stack_levels(a.sc));
    // compiled sizes 1, 2, 4, 8, 16: k = 1 runs the nearest walk's own stop rule
    launch_for_k(k, [&](auto K) {
        if (counters) hipLaunchKernelGGL((multihit_kernel<K(), true>), grid, block, lds, st, a, q);
        else hipLaunchKernelGGL((multihit_kernel<K(), false>), grid, block, lds, st, a, q);
    });
    return hipGetLastError();
}

}  // namespace rtamd
