// rt_descent.h — the guided depth-first descent of the octree records that
// rt_overlap.hip, rt_closest.hip and rt_sweep.hip answer their queries with,
// stated once: the loop (descend), the scan of a leaf's spheres (leaf_spheres)
// and the rule that sizes the per-lane stack (descent_levels).  The ray units
// use walk<> (rt_walk.h), which enters through the cell table and follows one
// ray; this descent starts at the root and visits every cell that a kernel's
// guide says its query can reach.
//
// A kernel adds two things: its guide (which cells are met, in which order,
// and whether an answer shrank the region) and its leaf step (the exact test
// of one sphere, and what it does with an accepted one).
#pragma once
#include <hip/hip_runtime.h>

#include "rt_params.h"
#include "rt_query_common.h"
#include "rt_walk.h"

namespace rtamd {

// The stack's levels: one per depth that can hold an internal node, from the
// deepest leaf itself (SceneArgs::stack_depth), not from stack_levels(): that
// one shrinks with the cell table, which this descent does not enter through.
inline uint32_t descent_levels(const SceneArgs& sc) { return sc.stack_depth ? sc.stack_depth : 1u; }

// A leaf's spheres in list order, kLeafChunk loads in flight: fn(sphere, slot)
// for each, slot its place in prim_sp (and in prim_idx, which a kernel reads
// for the spheres it accepts only).  A slot past the leaf's end reads the next
// leaf or the kPrimPad tail (in bounds) and is never tested.
template <bool kStats, typename Fn>
__device__ __forceinline__ void leaf_spheres(const float4* __restrict__ prim_sp, uint32_t off, uint32_t cnt,
                                             uint32_t& n_prims, Fn&& fn) {
    static_assert(kLeafChunk <= static_cast<int>(kPrimPad) + 1, "leaf loads may run past a leaf");
    for (uint32_t j = 0; j < cnt; j += kLeafChunk) {
        float4 sv[kLeafChunk];
#pragma unroll
        for (int s = 0; s < kLeafChunk; ++s) sv[s] = prim_sp[off + j + s];
#pragma unroll
        for (int s = 0; s < kLeafChunk; ++s) {
            if (j + s < cnt) {
                if (kStats) n_prims += 1;
                fn(sv[s], off + j + s);
            }
        }
    }
}

// What a guide says of a cell: the octant its visit starts from, and the
// children it meets in visiting order (in_order: bit j is child j ^ near).
struct ChildOrder {
    uint32_t near, met;
};

// The descent.  stk is the lane's column of the dynamic LDS, [level][thread]:
// level d holds the node at depth d while the lane is below it: {first child
// slot, valid | leaf << 8 | children still to visit, in visiting order << 16}.
// leaf(off, cnt) scans a leaf's list.  The guide:
//   root_met()                   whether the query reaches the root box at all
//   children(l0, l1, l2, half)   the ChildOrder of the cell at corner l
//                                (finest-grid units) with half-size `half`
//   shrank()                     after a leaf: whether the region is smaller
//                                now; then children() prunes the siblings
//   kReprune                     whether a pop asks children() again, for the
//                                siblings queued before the region shrank
// It is taken by value: what it keeps between calls (a bound, a box) lives for
// this descent, and what the leaf step changes it reads through a reference.
//
// How the loop is written decides its registers (profiles/r24/README.md).  The
// pop is a loop of its own, as the compiler made it in the kernels that had
// this loop written out; as `if (rem == 0) { ...; continue; }` in here it stays
// merged with the outer loop, and overlap_kernel<16> goes from 94 to 110 VGPRs
// (5 waves a SIMD to 4).  The guide by reference costs closest_kernel 20 to 36
// VGPRs at K = 8 and 16 against by value.
template <bool kStats, typename Guide, typename Leaf>
__device__ __forceinline__ void descend(const SceneArgs& S, uint2* stk, uint32_t levels, Guide guide,
                                        Leaf&& leaf, uint32_t& n_nodes) {
    if (guide.root_met()) {
        if (kStats) n_nodes += 1;  // the root record
        if (S.root_is_leaf) {
            if (S.root.y) leaf(S.root.x, S.root.y);  // an empty scene's root holds 0
        } else {
            // the node the lane iterates: its record, depth, corner and size,
            // its order, and the children still to visit (a mask that only
            // loses bits: no child is visited twice)
            uint2 node = S.root;
            uint32_t depth = 0, l0 = 0, l1 = 0, l2 = 0, size = 1u << S.max_depth;
            ChildOrder o = guide.children(l0, l1, l2, size >> 1);
            uint32_t rem = o.met & in_order(node.y & 0xFFu, o.near);
            for (;;) {
                while (rem == 0u) {  // pop
                    if (depth == 0u) return;
                    depth -= 1;
                    size <<= 1;
                    l0 &= ~(size - 1u);
                    l1 &= ~(size - 1u);
                    l2 &= ~(size - 1u);
                    node = stk[depth * kBlockThreads];
                    if (Guide::kReprune) {
                        o = guide.children(l0, l1, l2, size >> 1);
                        rem = (node.y >> 16) & o.met;
                    } else {
                        rem = node.y >> 16;
                    }
                }
                const uint32_t c = static_cast<uint32_t>(__builtin_ctz(rem)) ^ o.near;
                rem &= rem - 1u;
                const uint32_t valid = node.y & 0xFFu;
                const uint2 rec = S.nodes[node.x + __builtin_popcount(valid & ((1u << c) - 1u))];
                if (kStats) n_nodes += 1;
                if ((node.y >> 8) & (1u << c)) {
                    leaf(rec.x, rec.y);
                    if (guide.shrank()) rem &= guide.children(l0, l1, l2, size >> 1).met;
                } else if (depth < levels) {  // (always: the stack holds every internal depth)
                    stk[depth * kBlockThreads] = make_uint2(node.x, (node.y & 0xFFFFu) | (rem << 16));
                    const uint32_t half = size >> 1;
                    l0 += (c & 1u) ? half : 0u;
                    l1 += (c & 2u) ? half : 0u;
                    l2 += (c & 4u) ? half : 0u;
                    size = half;
                    depth += 1;
                    node = rec;
                    o = guide.children(l0, l1, l2, size >> 1);
                    rem = o.met & in_order(node.y & 0xFFu, o.near);
                }
            }
        }
    }
}

}  // namespace rtamd
