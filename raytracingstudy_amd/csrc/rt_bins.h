// rt_bins.h — a frame's primary rays answered from the screen-space bins
// (screen_bins.hip).  Device code only; included by
// rt_kernels.hip after rt_walk.h.
//
// All primary rays leave the camera origin, so the only spheres a wave's rays
// can meet are those whose pixel rectangle overlaps the wave's tile.  The
// frame's builder lists them per 8x8-pixel bin, nearest first by a lower bound
// on t; a wave tile lies in one bin, so the list's address is the same in
// every lane and its entries are read by scalar loads (the constant address
// space below), which cost the vector-memory path nothing.  Each entry that
// overlaps the tile runs the walk's own isect in every lane, with the walk's
// rule for equal t (the smaller sphere index), so the nearest hit is the
// walk's: DESIGN.md 2.2 defines it over the spheres the ray meets, however
// they are found.
#pragma once
#include <hip/hip_runtime.h>

#include "rt_bins_math.h"
#include "rt_params.h"
#include "rt_walk.h"

namespace rtamd {

// (native vectors: HIP's uint4 has no constructor from another address space)
typedef uint32_t bin_u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t bin_u32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(4))) const bin_u32x4 BinWords;

struct BinBest {
    float t;
    uint32_t idx, ref;
};

// One list (a bin's, or the wide list): entries [0, cnt) at `ent`, in
// ascending near-bound order.  trect: the wave tile's pixels, bin-local
// {x0, x1, y0, y1}.  A lane that takes no part holds best.t = -inf.
__device__ __forceinline__ void bin_list(BinWords* ent, uint32_t cnt, uint32_t tx0, uint32_t tx1,
                                         uint32_t ty0, uint32_t ty1, float o0, float o1, float o2,
                                         float d0, float d1, float d2, BinBest& best) {
    for (uint32_t k = 0; k < cnt; ++k) {
        const bin_u32x4 m = ent[2u * k + 1u];  // {idx, ref, rect, near}
        // no lane can still be improved, or tied, by this entry or a later one
        if (!__any(best.t >= __uint_as_float(m.w))) break;
        const uint32_t rc = m.z;
        if ((rc & 15u) > tx1 || ((rc >> 4) & 15u) < tx0 || ((rc >> 8) & 15u) > ty1 || ((rc >> 12) & 15u) < ty0)
            continue;
        const bin_u32x4 s = ent[2u * k];
        const float4 sp = make_float4(__uint_as_float(s.x), __uint_as_float(s.y), __uint_as_float(s.z),
                                      __uint_as_float(s.w));
        float th;
        if (isect(o0, o1, o2, d0, d1, d2, sp, 0.0f, INFINITY, th)) {
            if (th < best.t || (th == best.t && m.x < best.idx)) {
                best.t = th;
                best.idx = m.x;
                best.ref = m.y;
            }
        }
    }
}

// The nearest hit of the lanes' primary rays (origin o, the camera's; lanes
// with active = false take no part) from bin header `hdr` and the wide list:
// {hit, t, leaf reference} as walk<> returns them.  (tox, toy): the wave
// tile's origin pixel, tw x th its size, all wave-uniform.
__device__ __forceinline__ bool bin_nearest(uint2 hdr, uint32_t tox, uint32_t toy, uint32_t tw,
                                            uint32_t th, bool active, float o0, float o1, float o2,
                                            float d0, float d1, float d2, float& tout, uint32_t& iout) {
    KernArgs* ka = kernargs();
    BinBest best{active ? INFINITY : -INFINITY, kNoHit, kNoHit};
    const uint32_t tx0 = tox & (kBinSide - 1u), ty0 = toy & (kBinSide - 1u);
    BinWords* ent = reinterpret_cast<BinWords*>(reinterpret_cast<uintptr_t>(ka->bin_ent)) + 2ull * hdr.x;
    bin_list(ent, hdr.y, tx0, tx0 + tw - 1u, ty0, ty0 + th - 1u, o0, o1, o2, d0, d1, d2, best);
    const uint32_t nw = *reinterpret_cast<__attribute__((address_space(4))) const uint32_t*>(
        reinterpret_cast<uintptr_t>(ka->bin_info + kBinInfoWide));
    if (nw) {
        BinWords* wide = reinterpret_cast<BinWords*>(reinterpret_cast<uintptr_t>(ka->bin_wide));
        bin_list(wide, nw, 0u, kBinSide - 1u, 0u, kBinSide - 1u, o0, o1, o2, d0, d1, d2, best);
    }
    if (best.ref == kNoHit) return false;
    tout = best.t;
    iout = best.ref;
    return true;
}

// This wave tile's bin header and the frame's fallback flag (scalar loads):
// true when the tile's primary rays must walk (the frame's flag, or a bin
// over the cap).
__device__ __forceinline__ bool bin_header(uint32_t tox, uint32_t toy, uint2& hdr) {
    KernArgs* ka = kernargs();
    const uint32_t flag = *reinterpret_cast<__attribute__((address_space(4))) const uint32_t*>(
        reinterpret_cast<uintptr_t>(ka->bin_info + kBinInfoFlag));
    // a packed edge tile's wave tiles may lie off the image: no lane of such a
    // tile is valid and no bin covers it; an empty list
    if (tox >= ka->W || toy >= ka->H) {
        hdr = make_uint2(0u, 0u);
        return flag != 0u;
    }
    const uint32_t b = (toy >> kBinShift) * ka->bin_nbx + (tox >> kBinShift);
    const bin_u32x2 h = *reinterpret_cast<__attribute__((address_space(4))) const bin_u32x2*>(
        reinterpret_cast<uintptr_t>(ka->bin_hdr + b));
    hdr = make_uint2(h.x, h.y);
    return flag != 0u || h.y == kBinWalk;
}

}  // namespace rtamd
