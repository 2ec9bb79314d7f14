// rt_query_common.h — what the query units (rt_query.hip, rt_multihit.hip,
// rt_overlap.hip, rt_closest.hip, rt_sweep.hip, rt_gbuffer.hip, rt_ao.hip, rt_indirect.hip) share: the stats launches' wave
// sum and the visiting-order permutation of a child mask on the device, and the launchers' grid,
// stack size and k dispatch on the host.  rt_descent.h holds what the overlap, closest and sweep
// units share beyond that: their descent, leaf scan and stack levels.
//
// Two more things look shared and stay written out in each kernel: the
// `extern __shared__` stack declaration and the stats flush block.  Behind a
// helper here they move registers in the stats instances (the stack: 7 kernels
// with renamed registers; the flush: another schedule for overlap_kernel's,
// next_free_sgpr 54 -> 56; profiles/r16/README.md).
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "rt_params.h"

namespace rtamd {

// the sum of v over the wave's 64 lanes, in every lane
__device__ __forceinline__ unsigned long long query_wave_sum(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// A child mask (bit c: child c, x = 1, y = 2, z = 4) in visiting order: bit j
// is child j ^ near, so that ctz walks the children from `near` outward
// (rt_closest.hip: the probe's octant; rt_sweep.hip: the direction's signs;
// rt_overlap.hip: 0, the index order).
// Three conditional swaps, of bits, pairs and nibbles.
__device__ __forceinline__ uint32_t in_order(uint32_t m, uint32_t near) {
    m = (near & 1u) ? ((m & 0x55u) << 1) | ((m >> 1) & 0x55u) : m;
    m = (near & 2u) ? ((m & 0x33u) << 2) | ((m >> 2) & 0x33u) : m;
    m = (near & 4u) ? ((m & 0x0Fu) << 4) | ((m >> 4) & 0x0Fu) : m;
    return m;
}

// one item (ray, probe) per lane, 256-thread blocks
inline dim3 query_grid(uint32_t n) {
    return dim3(static_cast<uint32_t>((static_cast<uint64_t>(n) + kBlockThreads - 1u) / kBlockThreads));
}

// the dynamic LDS of a per-lane stack of `levels` levels: [level][thread]
inline size_t query_stack_bytes(uint32_t levels) {
    return static_cast<size_t>(levels) * kBlockThreads * sizeof(uint2);
}

// fn(std::integral_constant<int, K>) for the compiled buffer size K that holds
// the caller's k: 1, 2, 4, 8 or 16 (1 <= k <= 16: each launcher checked)
template <typename Fn>
void launch_for_k(uint32_t k, Fn fn) {
    if (k == 1) fn(std::integral_constant<int, 1>{});
    else if (k == 2) fn(std::integral_constant<int, 2>{});
    else if (k <= 4) fn(std::integral_constant<int, 4>{});
    else if (k <= 8) fn(std::integral_constant<int, 8>{});
    else fn(std::integral_constant<int, 16>{});
}

}  // namespace rtamd
