// rt_bins.h — a frame's primary rays answered from the screen-space bins
// (screen_bins.hip).  Device code only; included by
// rt_kernels.hip after rt_walk.h.
//
// All primary rays leave the camera origin, so the only spheres a wave's rays
// can meet are those whose pixel rectangle overlaps the wave's tile.  The
// frame's builder lists them per 8x8-pixel bin, nearest first by a lower bound
// on t; a wave tile lies in one bin, so the list's address is the same in
// every lane and its entries are read by scalar loads (the constant address
// space below), which cost the vector-memory path nothing.  Which entries
// overlap which wave tile is known when the lists are built: the builder
// leaves one 64-bit word per wave tile (round 15), and the kernel visits its
// set bits only, with no rectangle arithmetic of its own.  Each such entry
// runs the walk's own isect in every lane, with the walk's
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
typedef uint32_t bin_u32x8 __attribute__((ext_vector_type(8)));
typedef uint32_t bin_u32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(4))) const bin_u32x8 BinEntries;  // BinEntry, one scalar load each

struct BinBest {
    float t;
    uint32_t idx, ref;
};

// One entry e = {cx, cy, cz, r, idx, ref, rect, near} against the lanes' rays.
// False: no lane can still be improved, or tied, by this entry or a later one
// of its list (ascending near bounds).  A lane that takes no part holds
// best.t = -inf.
__device__ __forceinline__ bool bin_entry(const bin_u32x8 e, float o0, float o1, float o2, float d0,
                                          float d1, float d2, BinBest& best) {
    if (!__any(best.t >= __uint_as_float(e[7]))) return false;
    const float4 sp = make_float4(__uint_as_float(e[0]), __uint_as_float(e[1]), __uint_as_float(e[2]),
                                  __uint_as_float(e[3]));
    float th;
    if (isect(o0, o1, o2, d0, d1, d2, sp, 0.0f, INFINITY, th)) {
        if (th < best.t || (th == best.t && e[4] < best.idx)) {
            best.t = th;
            best.idx = e[4];
            best.ref = e[5];
        }
    }
    return true;
}

// The nearest hit of the lanes' primary rays (origin o, the camera's; lanes
// with active = false take no part) from bin header `hdr`, the wave tile's
// word `word` (bin_header) and the wide list, whose length is in the frame's
// constants `consts` (bin_frame_consts): {hit, t, leaf reference} as
// walk<> returns them.  The tile's entries are the word's set bits, visited
// lowest first: the list's order, so the near-bound break ends the visit where
// a scan of the whole list would have ended it.
__device__ __forceinline__ bool bin_nearest(uint2 hdr, unsigned long long word, bool active, float o0,
                                            float o1, float o2, float d0, float d1, float d2,
                                            float& tout, uint32_t& iout, uint32_t consts) {
    KernArgs* ka = kernargs();
    BinBest best{active ? INFINITY : -INFINITY, kNoHit, kNoHit};
    BinEntries* ent = reinterpret_cast<BinEntries*>(reinterpret_cast<uintptr_t>(ka->bin_ent)) + hdr.x;
    // (the next set bit's entry requested before this one's test, eight more
    // SGPRs under the build's cap of 80: C3 +1.9%, round 19, not kept)
    while (word) {
        const uint32_t k = static_cast<uint32_t>(__builtin_ctzll(word));
        word &= word - 1ull;
        if (!bin_entry(ent[k], o0, o1, o2, d0, d1, d2, best)) break;
    }
    const uint32_t nw = bin_consts_wide(consts);
    if (nw) {  // every tile tests the wide list: a plain loop
        BinEntries* wide = reinterpret_cast<BinEntries*>(reinterpret_cast<uintptr_t>(ka->bin_wide));
        for (uint32_t k = 0; k < nw; ++k)
            if (!bin_entry(wide[k], o0, o1, o2, d0, d1, d2, best)) break;
    }
    if (best.ref == kNoHit) return false;
    tout = best.t;
    iout = best.ref;
    return true;
}

// The frame's constants as one wave-uniform word (bin_consts_pack,
// rt_bins_math.h): the fallback flag and the wide list's length, read from
// bin_info by scalar loads, and the logarithms of the wave tile's sides (powers
// of two: wave_tile_shape).  Read once per wave (scene_body); bin_header and
// bin_nearest take the word and read none of these again.  (A frame whose wide
// list overflowed has its flag set and walks: the clamped count is not used.)
__device__ __forceinline__ uint32_t bin_frame_consts(uint32_t ltw, uint32_t lth) {
    typedef __attribute__((address_space(4))) const uint32_t ConstWord;
    ConstWord* info = reinterpret_cast<ConstWord*>(reinterpret_cast<uintptr_t>(kernargs()->bin_info));
    return bin_consts_pack(info[kBinInfoFlag], min(info[kBinInfoWide], kBinWideCap), ltw, lth);
}

// This wave tile's bin header and its tile word (scalar loads): true when the
// tile's primary rays must walk (the frame's flag, or a bin over the cap).
// (tox, toy): the wave tile's origin pixel, wave-uniform; consts: the frame's
// (bin_frame_consts).
__device__ __forceinline__ bool bin_header(uint32_t tox, uint32_t toy, uint32_t consts, uint2& hdr,
                                           unsigned long long& word) {
    KernArgs* ka = kernargs();
    const bool flag = bin_consts_flag(consts);
    const uint32_t ltw = bin_consts_ltw(consts), lth = bin_consts_lth(consts);
    // a packed edge tile's wave tiles may lie off the image: no lane of such a
    // tile is valid and no bin covers it; an empty list
    word = 0ull;
    if (tox >= ka->W || toy >= ka->H) {
        hdr = make_uint2(0u, 0u);
        return flag;
    }
    const uint32_t b = (toy >> kBinShift) * ka->bin_nbx + (tox >> kBinShift);
    const bin_u32x2 h = *reinterpret_cast<__attribute__((address_space(4))) const bin_u32x2*>(
        reinterpret_cast<uintptr_t>(ka->bin_hdr + b));
    // (an empty bin's words are not written: masked by its count)
    const size_t wi = (static_cast<size_t>(b) << (2u * kBinShift - ltw - lth)) + bin_tile_index_log2(tox, toy, ltw, lth);
    const bin_u32x2 w = *reinterpret_cast<__attribute__((address_space(4))) const bin_u32x2*>(
        reinterpret_cast<uintptr_t>(ka->bin_hdr + ka->bin_nb + wi));  // (the words follow the headers)
    hdr = make_uint2(h.x, h.y);
    if (h.y) word = (static_cast<unsigned long long>(w.y) << 32) | w.x;
    return flag || h.y == kBinWalk;
}

}  // namespace rtamd
