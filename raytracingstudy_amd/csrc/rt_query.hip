// rt_query.hip — batch ray queries against the scene octree (rt_trace_rays,
// rt_pick; include/rt.h).  The reference has no counterpart: its
// Octree::traverse is a stub (include/octree.h:19-21).
//
// One caller-supplied ray per lane through the frame kernels' own walk<>
// (rt_walk.h) in its generic mode: the same plane(), isect, step and tie
// rules, hence the CPU oracle's per-ray results and counters ray by ray.
// Compiled like rt_kernels.hip (-ffp-contract=off, IEEE division / sqrt).
#include <hip/hip_runtime.h>

#include "rt_params.h"
#include "rt_query_common.h"
#include "rt_walk.h"

namespace rtamd {

// rt_ray / rt_hit (include/rt.h) as the kernel reads and writes them
struct QueryArgs {
    const float4* rays;           // n x {origin.xyz, tmin}, {dir.xyz, tmax}
    uint2* hits;                  // n x {t bits, sphere index | kNoHit}
    uint32_t n;
    unsigned long long* counters; // stats launches: 8 lines of kStatLineStride words
};

// One ray per lane, 256-thread blocks; a ray is two coalesced dwordx4 loads,
// a hit one dwordx2 store.  FrameArgs leads the argument block although the
// generic walk compiles every kernargs() read out (rt_walk.h): kernargs()
// reinterprets the running kernel's argument segment as FrameArgs, so with
// this layout a read that a later change lets through finds the scene's
// fields (zero camera and screens), not another struct's bytes.
// The dynamic LDS is the per-lane ancestor stack alone: [level][thread],
// stack_levels(a.sc) levels (launch_query sizes it).
// (rt_query_common.h holds what is shared; the stack and the flush stay here: a helper moves registers in the stats instances)
template <bool kAny, bool kStats>
__global__ void __launch_bounds__(kBlockThreads) query_kernel(FrameArgs a, QueryArgs q) {
    extern __shared__ __attribute__((aligned(16))) float4 lds[];
    uint2* stk = reinterpret_cast<uint2*>(lds) + threadIdx.x;
    const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
    uint32_t n_nodes = 0, n_prims = 0;
    if (i < q.n) {
        const float4 r0 = q.rays[2u * static_cast<size_t>(i)];
        const float4 r1 = q.rays[2u * static_cast<size_t>(i) + 1u];
        float t = r1.w;  // a miss reports the ray's tmax
        uint32_t ref = kNoHit;
        const bool hit = walk<GenericRay<kAny, kStats>>(
            a.sc, r0.x, r0.y, r0.z, r1.x, r1.y, r1.z, r0.w, r1.w, t, ref, n_nodes, n_prims, stk);
        // the caller's sphere index, not the leaf reference
        const uint32_t sphere = hit ? a.sc.prim_idx[ref] : kNoHit;
        q.hits[i] = make_uint2(__float_as_uint(t), sphere);
    }
    if (kStats) {
        // per wave, one 128-byte line per XCD group (flush_counters' layout:
        // words 2 and 3 of a line; the ray counts are the host's n)
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
// counters != null: a stats launch (the caller zeroed its 8 lines).
hipError_t launch_query(const FrameArgs& a, const void* rays, void* hits, uint32_t n, bool any,
                        unsigned long long* counters, hipStream_t st) {
    if (n == 0) return hipSuccess;
    QueryArgs q;
    q.rays = static_cast<const float4*>(rays);
    q.hits = static_cast<uint2*>(hits);
    q.n = n;
    q.counters = counters;
    const dim3 grid = query_grid(n), block(kBlockThreads);
    const size_t lds = query_stack_bytes(stack_levels(a.sc));
    if (counters) {
        if (any) hipLaunchKernelGGL((query_kernel<true, true>), grid, block, lds, st, a, q);
        else hipLaunchKernelGGL((query_kernel<false, true>), grid, block, lds, st, a, q);
    } else {
        if (any) hipLaunchKernelGGL((query_kernel<true, false>), grid, block, lds, st, a, q);
        else hipLaunchKernelGGL((query_kernel<false, false>), grid, block, lds, st, a, q);
    }
    return hipGetLastError();
}

}  // namespace rtamd
