// rt_closest.hip — closest-sphere queries (rt_query_closest, rt_closest_at;
// include/rt.h): for each probe point, the k scene spheres
// whose surfaces are nearest, by (signed surface distance, sphere index), within
// the probe's search radius.  The reference has no counterpart
// (Octree::traverse is a stub, include/octree.h:19-21).
//
// One probe per lane in the guided descent of the octree records
// (rt_descent.h).  This kernel adds its guide, ShrinkingBoxGuide (a cell is
// visited iff it meets the grown box of the lane's bound, rt_closest_math.h,
// which shrinks as answers come in; a node's children are visited nearest
// octant first, so that the first leaves reached are near the probe and the
// bound is small early), and its leaf step (the key, and the K nearest
// accepted spheres in ClosestSet).
// Compiled like rt_query.hip (-ffp-contract=off).
#include <hip/hip_runtime.h>

#include "rt_closest_math.h"
#include "rt_descent.h"

namespace rtamd {

struct ClosestArgs {
    const float4* probes;          // n x {point.xyz, search radius}
    uint2* near;                   // n x k {key bits, sphere index | kNoHit}, probe-major
    uint32_t* counts;              // n x min(k, |set|), or null
    uint32_t n;
    uint32_t k;                    // the caller's k: 1 <= k <= K
    uint32_t skip_self;            // probe i leaves sphere index i out
    uint32_t levels;               // the LDS stack's levels (the launcher sized it)
    float slack_m;                 // closest_slack_m of the scene's root box
    unsigned long long* counters;  // stats launches: 8 lines of kStatLineStride words
};

// One lane's K nearest accepted spheres: {key, the caller's sphere index},
// sorted by (key, index), a free slot {the probe's radius as given, kNoHit}.
// Every accepted key is <= the radius and every index < kNoHit, so a free slot
// sorts after every sphere and key[K - 1] is the lane's bound either way: the
// radius until the buffer is full, the K-th key after.  Every index below is a
// compile-time constant once the loops are unrolled: the arrays are
// registers, never scratch.
template <int K>
struct ClosestSet {
    float key[K];
    uint32_t idx[K];
    __device__ __forceinline__ void clear(float radius) {
#pragma unroll
        for (int i = 0; i < K; ++i) {
            key[i] = radius;
            idx[i] = kNoHit;
        }
    }
    // A sphere with kc <= key[K - 1] (the caller tested).  It enters iff it
    // sorts before the K-th entry and is not held already: a sphere met again
    // in another leaf has the same key bits and the same index.
    __device__ __forceinline__ void offer(float kc, uint32_t ci) {
        uint32_t pos = 0;  // entries that sort before the candidate
        bool held = false;
#pragma unroll
        for (int i = 0; i < K; ++i) {
            const bool tie = key[i] == kc;
            pos += (key[i] < kc || (tie && idx[i] < ci)) ? 1u : 0u;
            held |= tie && idx[i] == ci;
        }
        if (held || pos >= static_cast<uint32_t>(K)) return;
#pragma unroll
        for (int i = K - 1; i >= 0; --i) {
            const bool below = static_cast<uint32_t>(i) > pos;  // shifts down one slot
            const bool here = static_cast<uint32_t>(i) == pos;
            const int up = i > 0 ? i - 1 : 0;
            key[i] = here ? kc : below ? key[up] : key[i];
            idx[i] = here ? ci : below ? idx[up] : idx[i];
        }
    }
};

// For the cell at corner l (finest-grid units) and half-size `half`: the
// octant of the probe's grid coordinates g against its mid planes, and the
// children the box meets, in visiting order.  rt_overlap.hip's children_met
// (per axis the lower half unless lo >= mid, the upper unless hi < mid) with
// every prune written so that a NaN comparison visits.  The two stay two: one
// form for both would change what a NaN corner does in one of the kernels,
// and its comparisons with it.
__device__ __forceinline__ ChildOrder children_in_order(const ClosestBox& b, const float g[3], uint32_t l0,
                                                        uint32_t l1, uint32_t l2, uint32_t half) {
    const float m0 = static_cast<float>(l0 + half);  // integers <= 2^16: exact
    const float m1 = static_cast<float>(l1 + half);
    const float m2 = static_cast<float>(l2 + half);
    const uint32_t x = (!(b.lo[0] >= m0) ? 0x55u : 0u) | (!(b.hi[0] < m0) ? 0xAAu : 0u);
    const uint32_t y = (!(b.lo[1] >= m1) ? 0x33u : 0u) | (!(b.hi[1] < m1) ? 0xCCu : 0u);
    const uint32_t z = (!(b.lo[2] >= m2) ? 0x0Fu : 0u) | (!(b.hi[2] < m2) ? 0xF0u : 0u);
    ChildOrder o;
    o.near = (g[0] >= m0 ? 1u : 0u) | (g[1] >= m1 ? 2u : 0u) | (g[2] >= m2 ? 4u : 0u);
    o.met = in_order(x & y & z, o.near);
    return o;
}

// The guide: the grown box of the lane's bound, rebuilt when a leaf lowered
// the K-th key; the children nearest octant first.
struct ShrinkingBoxGuide {
    enum { kReprune = 1 };
    float4 p;
    float g[3];  // the probe's grid coordinates: they only order the children
    ClosestBox b;
    float bound;  // the bound the box was built for: the radius, then the K-th key
    const SceneArgs& S;
    float slack_m;
    const float& kth;  // the lane's bound now (ClosestSet::key[K - 1])
    __device__ __forceinline__ bool root_met() const {
        const bool out_of_root = b.lo[0] >= S.G || b.lo[1] >= S.G || b.lo[2] >= S.G || b.hi[0] < 0.0f ||
                                 b.hi[1] < 0.0f || b.hi[2] < 0.0f;
        return !out_of_root;
    }
    __device__ __forceinline__ ChildOrder children(uint32_t l0, uint32_t l1, uint32_t l2, uint32_t half) const {
        return children_in_order(b, g, l0, l1, l2, half);
    }
    __device__ __forceinline__ bool shrank() {
        if (!(kth < bound)) return false;
        bound = kth;
        b = closest_box(p.x, p.y, p.z, bound, S.rmin, S.scale, slack_m);
        return true;
    }
};

// One probe per lane, 256-thread blocks, the K-entry buffer in registers (K is
// the caller's k rounded up to a compiled size).  A probe is one coalesced
// dwordx4 load.  FrameArgs leads the argument block as in rt_query.hip.  The
// dynamic LDS is the descent's per-lane stack (rt_descent.h).
template <int K, bool kStats>
__global__ void __launch_bounds__(kBlockThreads) closest_kernel(FrameArgs a, ClosestArgs q) {
    extern __shared__ __attribute__((aligned(16))) float4 lds[];
    uint2* stk = reinterpret_cast<uint2*>(lds) + threadIdx.x;
    const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
    uint32_t n_nodes = 0, n_prims = 0;
    if (i < q.n) {
        const SceneArgs& S = a.sc;
        const float4 p = q.probes[i];
        ClosestSet<K> set;
        set.clear(p.w);
        const uint32_t self = q.skip_self ? i : kNoHit;
        const float4* __restrict__ prim_sp = S.prim_sp;
        const uint32_t* __restrict__ prim_idx = S.prim_idx;
        // prim_idx is read only for a sphere whose key passes the bound
        // (closed: an equal key with a smaller index still gets in)
        auto test = [&](const float4& s, uint32_t slot) {
            const float kc = closest_key(p.x, p.y, p.z, s.x, s.y, s.z, s.w);
            if (kc <= set.key[K - 1]) {
                const uint32_t ci = prim_idx[slot];
                if (ci != self) set.offer(kc, ci);
            }
        };
        auto leaf = [&](uint32_t off, uint32_t cnt) { leaf_spheres<kStats>(prim_sp, off, cnt, n_prims, test); };
        if (closest_probe_ok(p.x, p.y, p.z, p.w)) {
            ShrinkingBoxGuide guide = {p,
                                       {(p.x - S.rmin[0]) * S.scale[0], (p.y - S.rmin[1]) * S.scale[1],
                                        (p.z - S.rmin[2]) * S.scale[2]},
                                       closest_box(p.x, p.y, p.z, p.w, S.rmin, S.scale, q.slack_m),
                                       p.w,
                                       S,
                                       q.slack_m,
                                       set.key[K - 1]};
            descend<kStats>(S, stk, q.levels, guide, leaf, n_nodes);
        }
        uint2* out = q.near + static_cast<size_t>(i) * q.k;
        uint32_t held = 0;
#pragma unroll
        for (int s = 0; s < K; ++s) {
            if (static_cast<uint32_t>(s) < q.k) {
                held += set.idx[s] != kNoHit ? 1u : 0u;
                out[s] = make_uint2(__float_as_uint(set.key[s]), set.idx[s]);
            }
        }
        if (q.counts) q.counts[i] = held;
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

// a.sc is the scene; the rest of `a` is unused by the kernel.  1 <= k <= 16
// (the caller checked); counts may be null; slack_m: closest_slack_m of the
// scene's root box; counters != null: a stats launch (the caller zeroed its 8
// lines).
hipError_t launch_closest(const FrameArgs& a, const void* probes, void* near, void* counts, uint32_t n,
                          uint32_t k, bool skip_self, float slack_m, unsigned long long* counters,
                          hipStream_t st) {
    if (n == 0) return hipSuccess;
    if (k == 0 || k > 16u) return hipErrorInvalidValue;
    ClosestArgs q;
    q.probes = static_cast<const float4*>(probes);
    q.near = static_cast<uint2*>(near);
    q.counts = static_cast<uint32_t*>(counts);
    q.n = n;
    q.k = k;
    q.skip_self = skip_self ? 1u : 0u;
    q.levels = descent_levels(a.sc);
    q.slack_m = slack_m;
    q.counters = counters;
    const dim3 grid = query_grid(n), block(kBlockThreads);
    const size_t lds = query_stack_bytes(q.levels);
    launch_for_k(k, [&](auto K) {
        if (counters) hipLaunchKernelGGL((closest_kernel<K(), true>), grid, block, lds, st, a, q);
        else hipLaunchKernelGGL((closest_kernel<K(), false>), grid, block, lds, st, a, q);
    });
    return hipGetLastError();
}

}  // namespace rtamd
