// rt_sweep.hip — swept-sphere queries (rt_sweep_spheres, rt_sweep_at,
// rt_pick_thick; include/rt.h): for each cast, a ball of
// radius R whose centre moves along a ray, the first scene sphere the ball
// touches, by (t, sphere index).  The reference has no counterpart
// (Octree::traverse is a stub, include/octree.h:19-21).
//
// One cast per lane in the guided descent of the octree records
// (rt_descent.h).  This kernel adds its leaf step (the inflated ray-sphere
// test, and the best (t, index) so far) and its guide, SegmentGuide, a segment
// where the other two have a box: a child is visited iff the
// segment tmin < t <= bound meets its cell grown by R and the slack
// (rt_sweep_math.h: a slab test, so an oblique cast visits a tube of cells and
// not its bounding box), the bound is the best t so far, and a node's children
// are visited in the order of the direction's signs, the child nearest the
// origin first, so that early hits shorten the segment.  The walk<> of the ray
// queries cannot answer this: the spheres a ball touches are listed in cells
// its centre never enters.
// Compiled like rt_query.hip (-ffp-contract=off).
#include <hip/hip_runtime.h>

#include "rt_descent.h"
#include "rt_sweep_math.h"

namespace rtamd {

struct SweepArgs {
    const float4* rays;            // n x {origin.xyz, tmin}, {dir.xyz, tmax}
    const float* radii;            // n, or null: every cast uses `radius`
    uint2* hits;                   // n x {t bits, sphere index | kNoHit}
    uint32_t n;
    float radius;
    uint32_t skip_self;            // cast i leaves sphere index i out
    uint32_t levels;               // the LDS stack's levels (the launcher sized it)
    float slack_m;                 // sweep_slack_m of the scene's root box
    unsigned long long* counters;  // stats launches: 8 lines of kStatLineStride words
};

// The children of the cell at corner l (finest-grid units, half-size `half`)
// whose grown cells the segment tmin < t <= bound meets, in visiting order.
// Two slabs an axis (the lower and the upper half), eight combinations; every
// index is a compile-time constant once the loops are unrolled.
__device__ __forceinline__ uint32_t sweep_children(const SweepGuide& sg, float tmin, float bound, uint32_t l0,
                                                   uint32_t l1, uint32_t l2, uint32_t half, uint32_t near) {
    const uint32_t l[3] = {l0, l1, l2};
    SweepSlab s[3][2];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float lo = static_cast<float>(l[i]);  // integers <= 2^16: exact
        const float mid = static_cast<float>(l[i] + half);
        const float hi = static_cast<float>(l[i] + 2u * half);
        s[i][0] = sweep_slab(sg, i, lo, mid);
        s[i][1] = sweep_slab(sg, i, mid, hi);
    }
    uint32_t m = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c)
        m |= sweep_meets(s[0][c & 1], s[1][(c >> 1) & 1], s[2][(c >> 2) & 1], tmin, bound) ? 1u << c : 0u;
    return in_order(m, near);
}

// The guide: the segment tmin < t <= best_t, which every hit shortens; the
// children in the order of the direction's signs.
struct SegmentGuide {
    enum { kReprune = 1 };
    SweepGuide sg;
    float tmin;
    uint32_t near;
    float G;
    float bound;          // the bound the last mask was tested against
    const float& best_t;  // the lane's bound now
    __device__ __forceinline__ bool root_met() const {
        return sweep_meets(sweep_slab(sg, 0, 0.0f, G), sweep_slab(sg, 1, 0.0f, G), sweep_slab(sg, 2, 0.0f, G), tmin,
                           best_t);
    }
    __device__ __forceinline__ ChildOrder children(uint32_t l0, uint32_t l1, uint32_t l2, uint32_t half) {
        bound = best_t;
        return {near, sweep_children(sg, tmin, bound, l0, l1, l2, half, near)};
    }
    __device__ __forceinline__ bool shrank() const { return best_t < bound; }
};

// One cast per lane, 256-thread blocks.  A ray is two coalesced dwordx4 loads,
// a radius a coalesced dword load or the kernel argument, a hit one dwordx2
// store.  FrameArgs leads the argument block as in rt_query.hip.  The dynamic
// LDS is the descent's per-lane stack (rt_descent.h).
template <bool kEntryOnly, bool kStats>
__global__ void __launch_bounds__(kBlockThreads) sweep_kernel(FrameArgs a, SweepArgs q) {
    extern __shared__ __attribute__((aligned(16))) float4 lds[];
    uint2* stk = reinterpret_cast<uint2*>(lds) + threadIdx.x;
    const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
    uint32_t n_nodes = 0, n_prims = 0;
    if (i < q.n) {
        const SceneArgs& S = a.sc;
        const float4 r0 = q.rays[2u * static_cast<size_t>(i)];
        const float4 r1 = q.rays[2u * static_cast<size_t>(i) + 1u];
        const float R = q.radii ? q.radii[i] : q.radius;
        const float tmin = r0.w, tmax = r1.w;
        // the answer so far: a miss reports the cast's tmax.  best_t is the
        // descent's bound too (closed: isect accepts t < tmax only, so a
        // sphere never ties with the miss)
        float best_t = tmax;
        uint32_t best = kNoHit;
        const uint32_t self = q.skip_self ? i : kNoHit;
        const float4* __restrict__ prim_sp = S.prim_sp;
        const uint32_t* __restrict__ prim_idx = S.prim_idx;
        // prim_idx is read only for a sphere whose t passes the bound (closed:
        // an equal t with a smaller index still gets in; a sphere met again in
        // another leaf has the same t bits and the same index, and changes
        // nothing)
        auto test = [&](const float4& s, uint32_t slot) {
            float th;
            if (sweep_isect(r0.x, r0.y, r0.z, r1.x, r1.y, r1.z, s.x, s.y, s.z, s.w, R, tmin, tmax, kEntryOnly, th) &&
                th <= best_t) {
                const uint32_t ci = prim_idx[slot];
                if (ci != self && (th < best_t || ci < best)) {
                    best_t = th;
                    best = ci;
                }
            }
        };
        auto leaf = [&](uint32_t off, uint32_t cnt) { leaf_spheres<kStats>(prim_sp, off, cnt, n_prims, test); };
        // (tmin < tmax: no t lies in any other window, a NaN end included)
        if (sweep_cast_ok(r0.x, r0.y, r0.z, r1.x, r1.y, r1.z, R) && tmin < tmax) {
            const SweepGuide sg = sweep_guide(r0.x, r0.y, r0.z, r1.x, r1.y, r1.z, R, S.rmin, S.scale,
                                              sweep_slack_o(r0.x, r0.y, r0.z) + q.slack_m);
            // the child nearest the origin on each axis: the upper half for a
            // negative direction
            const uint32_t near = (sg.inv[0] < 0.0f ? 1u : 0u) | (sg.inv[1] < 0.0f ? 2u : 0u) |
                                  (sg.inv[2] < 0.0f ? 4u : 0u);
            SegmentGuide guide = {sg, tmin, near, S.G, best_t, best_t};
            descend<kStats>(S, stk, q.levels, guide, leaf, n_nodes);
        }
        q.hits[i] = make_uint2(__float_as_uint(best_t), best);
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

// a.sc is the scene; the rest of `a` is unused by the kernel.  radii may be
// null (every cast uses `radius`); slack_m: sweep_slack_m of the scene's root
// box; counters != null: a stats launch (the caller zeroed its 8 lines).
hipError_t launch_sweep(const FrameArgs& a, const void* rays, const void* radii, float radius, void* hits,
                        uint32_t n, bool entry_only, bool skip_self, float slack_m,
                        unsigned long long* counters, hipStream_t st) {
    if (n == 0) return hipSuccess;
    SweepArgs q;
    q.rays = static_cast<const float4*>(rays);
    q.radii = static_cast<const float*>(radii);
    q.hits = static_cast<uint2*>(hits);
    q.n = n;
    q.radius = radius;
    q.skip_self = skip_self ? 1u : 0u;
    q.levels = descent_levels(a.sc);
    q.slack_m = slack_m;
    q.counters = counters;
    const dim3 grid = query_grid(n), block(kBlockThreads);
    const size_t lds = query_stack_bytes(q.levels);
    if (counters) {
        if (entry_only) hipLaunchKernelGGL((sweep_kernel<true, true>), grid, block, lds, st, a, q);
        else hipLaunchKernelGGL((sweep_kernel<false, true>), grid, block, lds, st, a, q);
    } else {
        if (entry_only) hipLaunchKernelGGL((sweep_kernel<true, false>), grid, block, lds, st, a, q);
        else hipLaunchKernelGGL((sweep_kernel<false, false>), grid, block, lds, st, a, q);
    }
    return hipGetLastError();
}

}  // namespace rtamd
