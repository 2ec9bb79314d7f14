// rt_overlap.hip — sphere-overlap queries (rt_query_overlaps, rt_overlaps_at;
// include/rt.h): for each probe sphere, the k smallest indices
// of the scene spheres it touches, and whether there are more.  The reference
// has no counterpart (Octree::traverse is a stub, include/octree.h:19-21).
//
// One probe per lane in the guided descent of the octree records
// (rt_descent.h).  This kernel adds its guide, BoxGuide (a cell is visited iff
// it meets the probe's grown box, rt_overlap_math.h; the children in index
// order; the box never changes), and its leaf step (the exact predicate, and
// the K smallest accepted indices in OverlapSet).
// Compiled like rt_query.hip (-ffp-contract=off).
#include <hip/hip_runtime.h>

#include "rt_descent.h"
#include "rt_overlap_math.h"

namespace rtamd {

struct OverlapArgs {
    const float4* probes;          // n x {centre.xyz, radius}
    uint32_t* indices;             // n x k sphere indices | kNoHit, probe-major
    uint32_t* counts;              // n x {min(k, |set|) | kOverlapMore}, or null
    uint32_t n;
    uint32_t k;                    // the caller's k: 1 <= k <= K
    uint32_t skip_self;            // probe i leaves sphere index i out
    uint32_t levels;               // the LDS stack's levels (the launcher sized it)
    float slack_m;                 // overlap_slack_m of the scene's root box
    unsigned long long* counters;  // stats launches: 8 lines of kStatLineStride words
};

constexpr uint32_t kOverlapMore = 0x80000000u;  // RT_OVERLAP_MORE

// One lane's K smallest accepted sphere indices, ascending, a free slot
// kNoHit (which sorts after every index).  `more`: a sphere that is not held
// was turned away from a full buffer, or an entry was pushed out, so the set
// is larger than K.  It is a word, not a bool: a bool that lives across the
// descent is a lane mask, and the compiler lost that mask's initial value for
// the lanes that skip the descent (a probe beside a root that is a leaf could
// report MORE with nothing held; profiles/r24/README.md).  Every index below
// is a compile-time constant once the loops are unrolled: the array is
// registers, never scratch.
template <int K>
struct OverlapSet {
    uint32_t idx[K];
    uint32_t more;  // 0 | 1
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int i = 0; i < K; ++i) idx[i] = kNoHit;
        more = 0u;
    }
    __device__ __forceinline__ void offer(uint32_t ci) {
        if (ci > idx[K - 1]) {  // (the last slot is taken, or ci could not exceed it)
            more = 1u;
            return;
        }
        uint32_t pos = 0;  // entries that sort before the candidate
        bool held = false;
#pragma unroll
        for (int i = 0; i < K; ++i) {
            pos += idx[i] < ci ? 1u : 0u;
            held |= idx[i] == ci;
        }
        if (held) return;  // met again in another leaf
        more |= idx[K - 1] != kNoHit ? 1u : 0u;
#pragma unroll
        for (int i = K - 1; i >= 0; --i) {
            const bool below = static_cast<uint32_t>(i) > pos;  // shifts down one slot
            const bool here = static_cast<uint32_t>(i) == pos;
            const int up = i > 0 ? i - 1 : 0;
            idx[i] = here ? ci : below ? idx[up] : idx[i];
        }
    }
};

// The children of the cell at corner l (finest-grid units) and half-size
// `half` that the box meets: per axis the lower half iff lo < mid, the upper
// iff hi >= mid; child c's bits are x = 1, y = 2, z = 4.
__device__ __forceinline__ uint32_t children_met(const OverlapBox& b, uint32_t l0, uint32_t l1,
                                                 uint32_t l2, uint32_t half) {
    const float m0 = static_cast<float>(l0 + half);  // integers <= 2^16: exact
    const float m1 = static_cast<float>(l1 + half);
    const float m2 = static_cast<float>(l2 + half);
    const uint32_t x = (b.lo[0] < m0 ? 0x55u : 0u) | (b.hi[0] >= m0 ? 0xAAu : 0u);
    const uint32_t y = (b.lo[1] < m1 ? 0x33u : 0u) | (b.hi[1] >= m1 ? 0xCCu : 0u);
    const uint32_t z = (b.lo[2] < m2 ? 0x0Fu : 0u) | (b.hi[2] >= m2 ? 0xF0u : 0u);
    return x & y & z;
}

// The guide: the probe's grown box, the same for the whole descent (the set
// only grows), the children in index order.
struct BoxGuide {
    enum { kReprune = 0 };  // the mask a pop finds is still right
    OverlapBox b;
    float G;
    __device__ __forceinline__ bool root_met() const {
        return b.lo[0] < G && b.lo[1] < G && b.lo[2] < G && b.hi[0] >= 0.0f && b.hi[1] >= 0.0f && b.hi[2] >= 0.0f;
    }
    __device__ __forceinline__ ChildOrder children(uint32_t l0, uint32_t l1, uint32_t l2, uint32_t half) const {
        return {0u, children_met(b, l0, l1, l2, half)};
    }
    __device__ __forceinline__ bool shrank() const { return false; }
};

// One probe per lane, 256-thread blocks, the K-entry buffer in registers (K is
// the caller's k rounded up to a compiled size).  A probe is one coalesced
// dwordx4 load.  FrameArgs leads the argument block as in rt_query.hip.  The
// dynamic LDS is the descent's per-lane stack (rt_descent.h).
// (rt_query_common.h: the stack's declaration and the flush stay here: a helper moves registers in the stats instances)
template <int K, bool kStats>
__global__ void __launch_bounds__(kBlockThreads) overlap_kernel(FrameArgs a, OverlapArgs q) {
    extern __shared__ __attribute__((aligned(16))) float4 lds[];
    uint2* stk = reinterpret_cast<uint2*>(lds) + threadIdx.x;
    const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
    uint32_t n_nodes = 0, n_prims = 0;
    if (i < q.n) {
        const SceneArgs& S = a.sc;
        const float4 p = q.probes[i];
        OverlapSet<K> set;
        set.clear();
        const uint32_t self = q.skip_self ? i : kNoHit;
        const float4* __restrict__ prim_sp = S.prim_sp;
        const uint32_t* __restrict__ prim_idx = S.prim_idx;
        // prim_idx is read for accepted spheres only
        auto test = [&](const float4& s, uint32_t slot) {
            if (overlap_accepts(p.x, p.y, p.z, p.w, s.x, s.y, s.z, s.w)) {
                const uint32_t ci = prim_idx[slot];
                if (ci != self) set.offer(ci);
            }
        };
        auto leaf = [&](uint32_t off, uint32_t cnt) { leaf_spheres<kStats>(prim_sp, off, cnt, n_prims, test); };
        if (overlap_probe_ok(p.x, p.y, p.z, p.w)) {
            BoxGuide guide = {overlap_box(p.x, p.y, p.z, p.w, S.rmin, S.scale, q.slack_m), S.G};
            descend<kStats>(S, stk, q.levels, guide, leaf, n_nodes);
        }
        uint32_t* out = q.indices + static_cast<size_t>(i) * q.k;
        uint32_t held = 0;
#pragma unroll
        for (int s = 0; s < K; ++s) {
            held += set.idx[s] != kNoHit ? 1u : 0u;
            if (static_cast<uint32_t>(s) < q.k) out[s] = set.idx[s];
        }
        if (q.counts) {
            const bool more = set.more != 0u || held > q.k;
            q.counts[i] = min(held, q.k) | (more ? kOverlapMore : 0u);
        }
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
// (the caller checked); counts may be null; slack_m: overlap_slack_m of the
// scene's root box; counters != null: a stats launch (the caller zeroed its 8
// lines).
hipError_t launch_overlap(const FrameArgs& a, const void* probes, void* indices, void* counts,
                          uint32_t n, uint32_t k, bool skip_self, float slack_m,
                          unsigned long long* counters, hipStream_t st) {
    if (n == 0) return hipSuccess;
    if (k == 0 || k > 16u) return hipErrorInvalidValue;
    OverlapArgs q;
    q.probes = static_cast<const float4*>(probes);
    q.indices = static_cast<uint32_t*>(indices);
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
        if (counters) hipLaunchKernelGGL((overlap_kernel<K(), true>), grid, block, lds, st, a, q);
        else hipLaunchKernelGGL((overlap_kernel<K(), false>), grid, block, lds, st, a, q);
    });
    return hipGetLastError();
}

}  // namespace rtamd
