// rt_shade.h — a frame's samples: the sample mapping and its hashes, the
// camera ray, one sample's colour (sample_color_unified) and a wave tile's
// pixels with their ordered sums (shade_wave_tile).  Device code of the scene
// kernels; included by rt_kernels.hip only.
#pragma once
#include <hip/hip_runtime.h>

#include "rt_params.h"
#include "rt_walk.h"  // the octree walk (shared with the ray-query kernels)
#include "rt_bins.h"  // primary rays from the frame's screen-space bins

namespace rtamd {

__device__ __forceinline__ float sat(float x) { return x > 0.0f ? (x < 1.0f ? x : 1.0f) : 0.0f; }

__device__ __forceinline__ uint32_t mix32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

__device__ __forceinline__ float u01(uint32_t x) {
    return static_cast<float>(x >> 8) * (1.0f / 16777216.0f);
}

// include/camera.h:24-41 — Camera::getRay, camera passed by value.
__device__ __forceinline__ void get_ray(const CamArgs& c, float u, float v, float& wx, float& wy,
                                        float& wz) {
    const float dx = (u - c.K[2]) / c.K[0];
    const float dy = (v - c.K[5]) / c.K[4];
    const float dz = 1.0f;
    wx = c.R[0] * dx + c.R[3] * dy + c.R[6] * dz;
    wy = c.R[1] * dx + c.R[4] * dy + c.R[7] * dz;
    wz = c.R[2] * dx + c.R[5] * dy + c.R[8] * dz;
    const float len = sqrtf(wx * wx + wy * wy + wz * wz);
    wx /= len;
    wy /= len;
    wz /= len;
}

// ---------------------------------------------------------------------------
// Frame mapping, shading, ordered accumulation
//
// A wave owns `ppw` pixels x `spw` samples (host: spw = min(spp, 64),
// ppw = pow2floor(64 / spw)); lane l works on pixel l / spw, sample
// round * spw + l % spw.  At spp >= 64 all 64 lanes of a wave trace jittered
// samples of ONE pixel: their primary rays stay within one pixel footprint and
// their shadow rays start from nearly the same point with the same direction,
// so the wave's lanes follow nearly the same octree path (little SIMD
// divergence, and coherent packets).  The per-pixel mean keeps the oracle's
// exact summation order: every lane parks its sample colour in LDS and the
// pixel's leader lane adds them in sample order.
// ---------------------------------------------------------------------------

struct PixelOut {
    float r, g, b;
};

__device__ __forceinline__ uint32_t pack_rgba8(const PixelOut& p) {
    const uint32_t r = static_cast<uint32_t>(sat(p.r) * 255.0f);
    const uint32_t g = static_cast<uint32_t>(sat(p.g) * 255.0f);
    const uint32_t b = static_cast<uint32_t>(sat(p.b) * 255.0f);
    return r | (g << 8) | (b << 16) | (255u << 24);
}

// Unified lane path: one walk instance run twice (primary, then the shadow ray
// of the lanes that need one), so the register allocator sees one walk.
// kBin: the primary ray is answered from the frame's screen-space bins
// (rt_bins.h; (tox, toy): the wave tile's origin pixel, wave-uniform); a tile
// whose bin is over the cap, or a frame whose builder raised its flag, walks
// under a wave-uniform branch.  binc: the frame's constants of the bins
// (bin_frame_consts, read once per wave).
// C: the frame's switches (Frame<>, rt_sched.h).
template <class C>
__device__ __forceinline__ PixelOut sample_color_unified(const FrameArgs& a, uint32_t x,
                                                         uint32_t y, uint32_t hp, uint32_t s,
                                                         bool valid, uint32_t& n_shadow,
                                                         uint32_t& n_nodes, uint32_t& n_prims,
                                                         void* stk, uint32_t* bs, uint32_t lbs,
                                                         uint32_t tox = 0, uint32_t toy = 0,
                                                         uint32_t binc = 0) {
    constexpr bool kStats = C::stats, kCam8 = C::cam8, kOcc = C::occ, kBin = C::bin;
    const SceneArgs& S = a.sc;
    KernArgs* ka = kernargs();
    float u = static_cast<float>(x), v = static_cast<float>(y);
    if (ka->jitter) {
        u = u + u01(mix32(hp ^ (s << 1)));
        v = v + u01(mix32(hp ^ ((s << 1) | 1u)));
    }
    float r0 = ka->cam.o[0], r1 = ka->cam.o[1], r2 = ka->cam.o[2];
    float d0, d1, d2;
    {
        CamArgs cam;
        for (int i = 0; i < 9; ++i) cam.K[i] = ka->cam.K[i], cam.R[i] = ka->cam.R[i];
        get_ray(cam, u, v, d0, d1, d2);
    }
    const float miss_g = sat(d1), miss_b = sat(d2);
    bool active = valid, hit0 = false;
    float lam = 0.0f;
    uint32_t al = 0;
    uint2 occ_hdr = make_uint2(0u, 0u);  // kOcc: the hit sphere's occluder-list header
    // the primary and the shadow walk as two instances (the phase loop was
    // always unrolled into two copies; written out so that the primary one
    // keeps the camera-relative screen, a compile-time choice)
#pragma unroll
    for (int phase = 0; phase < 2; ++phase) {
        float t = 0.0f;
        uint32_t idx = 0;
        bool hit = false;
        bool binned = false;
        if (kBin && phase == 0) {
            uint2 bh;
            unsigned long long bw;
            binned = !bin_header(tox, toy, binc, bh, bw);
            if (binned) hit = bin_nearest(bh, bw, active, r0, r1, r2, d0, d1, d2, t, idx, binc);
        }
        if (active && !binned) {
            RT_BS(kBsPhase);
            if (phase) RT_BS(kBsPhaseShadow);
            if (phase == 0)
                hit = walk<FramePrimary<kStats, kCam8>>(S, r0, r1, r2, d0, d1, d2, 0.0f, INFINITY, t, idx,
                                                        n_nodes, n_prims, static_cast<uint2*>(stk),
                                                        false, bs, lbs);
            else if (kOcc) {
                // answered from the hit sphere's occluder list (round 7)
                hit = shadow_occluded<false>(S, occ_hdr, true, r0, r1, r2, static_cast<uint2*>(stk));
            } else {
                // the shadow direction L is the frame's, the same in every
                // lane: read afresh from the kernel arguments (SGPRs), not the
                // lanes' d registers
                KernArgs* kl = kernargs();
                hit = walk<FrameShadow<kStats>>(
                    S, r0, r1, r2, kl->L[0], kl->L[1], kl->L[2], 0.0f, INFINITY, t, idx, n_nodes,
                    n_prims, static_cast<uint2*>(stk), true, bs);
            }
        }
        if (phase == 0) {
            hit0 = active && hit;
            bool want_shadow = false;
            KernArgs* kb = kernargs();
            if (hit0) {
                RT_BS(kBsShadeLoad);  // the sphere record
                RT_BS(kBsShadeLoad);  // the albedo
                const float4 sp = kb->sc.prim_sp[idx];
                // the albedo and the occluder header depend on idx alone:
                // requested with the sphere, in front of one wait (round 19).
                // A lane facing away from the light loads a header it ignores
                // (prim_occ holds one for every reference).
                al = kb->sc.prim_al[idx];
                if (kOcc) occ_hdr = kb->sc.prim_occ[idx];
                const float p0 = r0 + t * d0;
                const float p1 = r1 + t * d1;
                const float p2 = r2 + t * d2;
                const float ir = 1.0f / sp.w;
                const float n0 = (p0 - sp.x) * ir;
                const float n1 = (p1 - sp.y) * ir;
                const float n2 = (p2 - sp.z) * ir;
                const float ndl = n0 * kb->L[0] + n1 * kb->L[1] + n2 * kb->L[2];
                lam = ndl > 0.0f ? ndl : 0.0f;
                want_shadow = ndl > 0.0f && kb->shadows;
                r0 = p0 + n0 * kShadowEps;
                r1 = p1 + n1 * kShadowEps;
                r2 = p2 + n2 * kShadowEps;
                d0 = kb->L[0];
                d1 = kb->L[1];
                d2 = kb->L[2];
            }
            active = want_shadow;
            n_shadow += static_cast<uint32_t>(__popcll(__ballot(active)));  // wave-uniform
            if (!__any(active)) break;
        } else if (active && hit) {
            lam = 0.0f;
        }
    }
    PixelOut c{200.0f / 255.0f, miss_g, miss_b};
    if (hit0) {
        const float amb = kernargs()->ambient;
        const float f = amb + (1.0f - amb) * lam;
        c.r = static_cast<float>(al & 0xFFu) * (1.0f / 255.0f) * f;
        c.g = static_cast<float>((al >> 8) & 0xFFu) * (1.0f / 255.0f) * f;
        c.b = static_cast<float>((al >> 16) & 0xFFu) * (1.0f / 255.0f) * f;
    }
    return c;
}

// Wave tile (tw x th pixels x spw samples, launch_scene) at pixel origin
// (ox, oy); for a packed tile list also obase: image pixel (x, y) of this
// tile is packed word obase + y * tile_size + x (mod 2^32; one value kept
// live across the walks instead of the slot and the tile-local origin).
// Rounds of spw samples, pairwise butterfly per round, rounds added in
// order in the leader's LDS slot, then the mean is written.
template <class C>
__device__ __forceinline__ void shade_wave_tile(const FrameArgs& a, float4* acc, void* stk,
                                                uint32_t ox, uint32_t oy, uint32_t obase,
                                                uint32_t& n_primary,
                                                uint32_t& n_shadow, uint32_t& n_nodes,
                                                uint32_t& n_prims, uint32_t* bs, uint32_t lbs,
                                                uint32_t binc = 0) {
    constexpr bool kTiles = C::tiles, kProg = C::prog;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t spw = a.spw, g = a.g;
    const uint32_t pix = lane / g, sub = lane & (g - 1u);
    const uint32_t qx = pix % a.tw, qy = pix / a.tw;
    const uint32_t x = ox + qx, y = oy + qy;
    const bool lane_pix = pix < a.ppw && x < a.W && y < a.H;
    const bool leader = lane_pix && sub == 0;
    const uint32_t pid = y * a.W + x;
    const uint32_t hp = mix32(a.seedmix ^ pid);
    // progressive: the stored sum seeds the leader's LDS slot, so round 0
    // adds onto it like any later round (nothing extra live in the walk)
    if (kProg && a.accum_in && leader) acc[threadIdx.x] = a.accum[(size_t)y * a.W + x];
    // sample index across accumulated frames: s_base + r*spw + sub
    const uint32_t s_base = kProg ? a.s_base : 0u;
    const uint32_t sub_base = s_base + sub;
    const uint32_t s_end = s_base + a.spp;
    const bool lane_ok = lane_pix && sub < spw;
    for (uint32_t r = 0; r < a.rounds; ++r) {
        const uint32_t sg = r * spw + sub_base;
        const bool valid = lane_ok && sg < s_end;
        n_primary += static_cast<uint32_t>(__popcll(__ballot(valid)));  // wave-uniform
        PixelOut c = sample_color_unified<C>(a, x, y, hp, sg, valid, n_shadow, n_nodes, n_prims, stk,
                                             bs, lbs, ox, oy, binc);
        // Pixel sum of this round: pairwise butterfly over the pixel's g
        // lanes (missing samples are 0) = oracle.c:tree_sum; rounds are then
        // added in order in the leader's LDS slot.
        // (Round 19, neither kept: the steps up to m = 8 as DPP operands and 16,
        // 32 as row and half swaps, no LDS round trip, C3 +1.5%; the leader's
        // slot not written and read back in a frame of one round, C3 +0.5%.)
        if (!valid) c = PixelOut{0.0f, 0.0f, 0.0f};
        for (uint32_t m = 1; m < g; m <<= 1) {
            c.r += __shfl_xor(c.r, static_cast<int>(m), 64);
            c.g += __shfl_xor(c.g, static_cast<int>(m), 64);
            c.b += __shfl_xor(c.b, static_cast<int>(m), 64);
        }
        if (leader) {
            if (r || (kProg && a.accum_in)) {
                const float4 A = acc[threadIdx.x];
                c.r = A.x + c.r;
                c.g = A.y + c.g;
                c.b = A.z + c.b;
            }
            acc[threadIdx.x] = make_float4(c.r, c.g, c.b, 0.0f);
        }
    }
    // outputs: fields read afresh (kernargs()), not kept live across the walks
    KernArgs* ko = kernargs();
    if (leader) {
        const float4 A = acc[threadIdx.x];
        if (kProg) ko->accum[(size_t)y * ko->W + x] = A;
        const float isp = ko->inv_spp;
        const PixelOut p{A.x * isp, A.y * isp, A.z * isp};
        const uint32_t rgba = pack_rgba8(p);
        if (kTiles) {
            ko->out8[obase + y * ko->tile_size + x] = rgba;
        } else {
            ko->out8[(size_t)y * ko->W + x] = rgba;
            if (ko->out32) ko->out32[(size_t)y * ko->W + x] = make_float4(p.r, p.g, p.b, 1.0f);
        }
    } else if (kTiles && sub == 0 && pix < ko->ppw) {
        ko->out8[obase + y * ko->tile_size + x] = 0u;  // off-image pixel of an edge tile
    }
}

// ---------------------------------------------------------------------------
// Pixel pairs (Frame<kFPair>)
//
// A binned plain frame of 33 .. 64 spp gives a wave one pixel: everything
// wave-uniform (the bin's header, the entries' scalar loads and loop control,
// the kernel-argument reads, the butterfly's trips, the output address) is
// paid once a pixel.  Here a lane carries sample s of pixel A = (x, y) AND of
// pixel B = (x + 1, y), x even: the two lie in one bin, so the wave does that
// work once for both.  Per pixel nothing changes: the same ray, the entries of
// its own tile word in the list's order with its own near-bound break, the
// same tie rule, the same shading operands and the butterfly's pairing.
//
// False: the pair was not shaded and nothing was written or counted (the
// frame's flag, a bin over the cap, a hit sphere whose
// shadow rays walk the octree): the caller shades A and B by the one-pixel
// path, which holds the kernel's only copies of the walks.
// ---------------------------------------------------------------------------

typedef uint32_t pair_u32x4 __attribute__((ext_vector_type(4), aligned(8)));

// one pixel's samples of a pair
struct PairRay {
    float d0, d1, d2;
};

__device__ __forceinline__ PairRay pair_ray(KernArgs* ka, uint32_t x, uint32_t y, uint32_t hp, uint32_t s) {
    float u = static_cast<float>(x), v = static_cast<float>(y);
    if (ka->jitter) {
        u = u + u01(mix32(hp ^ (s << 1)));
        v = v + u01(mix32(hp ^ ((s << 1) | 1u)));
    }
    CamArgs cam;
    for (int i = 0; i < 9; ++i) cam.K[i] = ka->cam.K[i], cam.R[i] = ka->cam.R[i];
    PairRay r;
    get_ray(cam, u, v, r.d0, r.d1, r.d2);
    return r;
}

// A hit's shading (sample_color_unified's, same operands in the same order):
// Lambert term, whether a shadow ray is wanted and its origin.
struct PairShade {
    float lam, o0, o1, o2;
    bool want;
};
__device__ __forceinline__ PairShade pair_shade(KernArgs* kb, float4 sp, float r0, float r1, float r2,
                                                const PairRay& d, float t, bool hit) {
    const float p0 = r0 + t * d.d0;
    const float p1 = r1 + t * d.d1;
    const float p2 = r2 + t * d.d2;
    const float ir = 1.0f / sp.w;
    const float n0 = (p0 - sp.x) * ir;
    const float n1 = (p1 - sp.y) * ir;
    const float n2 = (p2 - sp.z) * ir;
    const float ndl = n0 * kb->L[0] + n1 * kb->L[1] + n2 * kb->L[2];
    PairShade s;
    s.lam = hit && ndl > 0.0f ? ndl : 0.0f;
    s.want = hit && ndl > 0.0f && kb->shadows;
    s.o0 = p0 + n0 * kShadowEps;
    s.o1 = p1 + n1 * kShadowEps;
    s.o2 = p2 + n2 * kShadowEps;
    return s;
}

__device__ __forceinline__ PixelOut pair_color(float amb, bool hit, float lam, uint32_t al, const PairRay& d) {
    PixelOut c{200.0f / 255.0f, sat(d.d1), sat(d.d2)};
    if (hit) {
        const float f = amb + (1.0f - amb) * lam;
        c.r = static_cast<float>(al & 0xFFu) * (1.0f / 255.0f) * f;
        c.g = static_cast<float>((al >> 8) & 0xFFu) * (1.0f / 255.0f) * f;
        c.b = static_cast<float>((al >> 16) & 0xFFu) * (1.0f / 255.0f) * f;
    }
    return c;
}

// (ox, oy): pixel A, ox even; binc: bin_frame_consts.
template <class C>
__device__ __forceinline__ bool shade_pixel_pair(uint32_t ox, uint32_t oy, uint32_t& n_primary,
                                                 uint32_t& n_shadow, uint32_t binc) {
    static_assert(C::pair && !C::tiles, "a frame instance with the pair path");
    KernArgs* ka = kernargs();
    const uint32_t W = ka->W;
    if (bin_consts_flag(binc)) return false;
    // the bin's header and both tile words: adjacent, A's first (x even)
    const uint32_t b = (oy >> kBinShift) * ka->bin_nbx + (ox >> kBinShift);
    const bin_u32x2 h = *reinterpret_cast<__attribute__((address_space(4))) const bin_u32x2*>(
        reinterpret_cast<uintptr_t>(ka->bin_hdr + b));
    const size_t wi = (static_cast<size_t>(b) << (2u * kBinShift)) + bin_tile_index_log2(ox, oy, 0u, 0u);
    const pair_u32x4 w = *reinterpret_cast<__attribute__((address_space(4))) const pair_u32x4*>(
        reinterpret_cast<uintptr_t>(ka->bin_hdr + ka->bin_nb + wi));
    if (h.y == kBinWalk) return false;
    const bool b_on = ox + 1u < W;  // B off the image (an odd width): its lanes take no part
    unsigned long long wa = h.y ? (static_cast<unsigned long long>(w.y) << 32) | w.x : 0ull;
    unsigned long long wb = h.y && b_on ? (static_cast<unsigned long long>(w.w) << 32) | w.z : 0ull;

    // (made here from the thread index each time: as a loop invariant of the
    // queue loop the lane index was spilled to scratch and reloaded per pair)
    uint32_t tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const uint32_t lane = tid & 63u;
    const bool va = lane < ka->spw, vb = va && b_on;
    const uint32_t pid = oy * W + ox;
    const uint32_t seedmix = ka->seedmix;
    const PairRay da = pair_ray(ka, ox, oy, mix32(seedmix ^ pid), lane);
    const PairRay db = pair_ray(ka, ox + 1u, oy, mix32(seedmix ^ (pid + 1u)), lane);
    const float r0 = ka->cam.o[0], r1 = ka->cam.o[1], r2 = ka->cam.o[2];

    // the entries of wa | wb, lowest first; a pixel takes part in those of its
    // own word until its near-bound break (bin_nearest's loop, per pixel)
    BinBest ba{va ? INFINITY : -INFINITY, kNoHit, kNoHit};
    BinBest bb{vb ? INFINITY : -INFINITY, kNoHit, kNoHit};
    BinEntries* ent = reinterpret_cast<BinEntries*>(reinterpret_cast<uintptr_t>(ka->bin_ent)) + h.x;
    while (wa | wb) {
        const uint32_t k = static_cast<uint32_t>(__builtin_ctzll(wa | wb));
        const unsigned long long bit = 1ull << k;
        const bin_u32x8 e = ent[k];
        const bool in_a = (wa & bit) != 0ull, in_b = (wb & bit) != 0ull;
        wa &= ~bit;
        wb &= ~bit;
        if (in_a && !bin_entry(e, r0, r1, r2, da.d0, da.d1, da.d2, ba)) wa = 0ull;
        if (in_b && !bin_entry(e, r0, r1, r2, db.d0, db.d1, db.d2, bb)) wb = 0ull;
    }
    const uint32_t nw = bin_consts_wide(binc);
    if (nw) {  // the wide list: every entry against both pixels, each to its own break
        BinEntries* wide = reinterpret_cast<BinEntries*>(reinterpret_cast<uintptr_t>(ka->bin_wide));
        bool on_a = true, on_b = b_on;
        for (uint32_t k = 0; k < nw && (on_a || on_b); ++k) {
            const bin_u32x8 e = wide[k];
            if (on_a) on_a = bin_entry(e, r0, r1, r2, da.d0, da.d1, da.d2, ba);
            if (on_b) on_b = bin_entry(e, r0, r1, r2, db.d0, db.d1, db.d2, bb);
        }
    }
    const bool hit_a = ba.ref != kNoHit, hit_b = bb.ref != kNoHit;

    // shading: one region for "A or B hit", the six records in front of one
    // wait.  A pixel that missed reads the other's reference (a valid one) and
    // keeps none of what it computes from it.
    float lam_a = 0.0f, lam_b = 0.0f;
    uint32_t al_a = 0, al_b = 0;
    uint2 occ_a = make_uint2(0u, 0u), occ_b = make_uint2(0u, 0u);
    PairShade sa{0.0f, 0.0f, 0.0f, 0.0f, false}, sb = sa;
    if (hit_a || hit_b) {
        KernArgs* kb = kernargs();
        const uint32_t ia = hit_a ? ba.ref : bb.ref, ib = hit_b ? bb.ref : ba.ref;
        const float4 sp_a = kb->sc.prim_sp[ia];
        const float4 sp_b = kb->sc.prim_sp[ib];
        al_a = kb->sc.prim_al[ia];
        al_b = kb->sc.prim_al[ib];
        occ_a = kb->sc.prim_occ[ia];
        occ_b = kb->sc.prim_occ[ib];
        sa = pair_shade(kb, sp_a, r0, r1, r2, da, ba.t, hit_a);
        sb = pair_shade(kb, sp_b, r0, r1, r2, db, bb.t, hit_b);
        lam_a = sa.lam, lam_b = sb.lam;
    }
    const bool want_a = sa.want, want_b = sb.want;
    // a hit sphere without a list: its rays walk, by the one-pixel path (decided
    // by the whole wave, outside the lanes' region)
    if (__any((want_a && occ_a.y == kOccWalk) || (want_b && occ_b.y == kOccWalk))) return false;
    if (want_a || want_b) {
        // both pixels' occluder lists in one loop, each lane to its own list's
        // end or first occluder (shadow_occluded's loop, per pixel); a lane
        // with no candidate left reads occ_sp[0] and keeps nothing of it
        KernArgs* kl = kernargs();
        const float l0 = kl->L[0], l1 = kl->L[1], l2 = kl->L[2];
        const float4* __restrict__ lst = kl->sc.occ_sp;
        const uint32_t cnt_a = want_a ? occ_a.y : 0u, cnt_b = want_b ? occ_b.y : 0u;
        // The state carried round the loop is plain data: a list end per pixel,
        // which its first occluder sets to 0 (so "occluded" is end != cnt), and
        // the wave leaves together once no lane has a candidate left.  (Round
        // 27: with each lane leaving on its own and "occluded" carried as
        // bools, the loop's body block held 26 scalar instructions of
        // exec-mask bookkeeping against 7, and 6 more VALU: C3 -2.8%.)
        uint32_t end_a = cnt_a, end_b = cnt_b;
        for (uint32_t k = 0;; ++k) {
            const bool go_a = k < end_a, go_b = k < end_b;
            if (!__any(go_a | go_b)) break;
            const float4 ca = lst[go_a ? occ_a.x + k : 0u];
            const float4 cb = lst[go_b ? occ_b.x + k : 0u];
            float th;
            const bool xa = isect(sa.o0, sa.o1, sa.o2, l0, l1, l2, ca, 0.0f, INFINITY, th);
            const bool xb = isect(sb.o0, sb.o1, sb.o2, l0, l1, l2, cb, 0.0f, INFINITY, th);
            end_a = (go_a & xa) ? 0u : end_a;
            end_b = (go_b & xb) ? 0u : end_b;
        }
        if (end_a != cnt_a) lam_a = 0.0f;
        if (end_b != cnt_b) lam_b = 0.0f;
    }
    n_primary += static_cast<uint32_t>(__popcll(__ballot(va)) + __popcll(__ballot(vb)));
    n_shadow += static_cast<uint32_t>(__popcll(__ballot(want_a)) + __popcll(__ballot(want_b)));

    // both pixels' sums in the butterfly's six trips (tree_sum's pairing for
    // each); every lane ends with both sums, bit for bit the leader's
    const float amb = kernargs()->ambient;
    PixelOut ca = pair_color(amb, hit_a, lam_a, al_a, da);
    PixelOut cb = pair_color(amb, hit_b, lam_b, al_b, db);
    if (!va) ca = PixelOut{0.0f, 0.0f, 0.0f};
    if (!vb) cb = PixelOut{0.0f, 0.0f, 0.0f};
#pragma unroll
    for (uint32_t m = 1; m < 64u; m <<= 1) {
        const float ar = __shfl_xor(ca.r, static_cast<int>(m), 64), ag = __shfl_xor(ca.g, static_cast<int>(m), 64),
                    ab = __shfl_xor(ca.b, static_cast<int>(m), 64), br = __shfl_xor(cb.r, static_cast<int>(m), 64),
                    bg = __shfl_xor(cb.g, static_cast<int>(m), 64), bl = __shfl_xor(cb.b, static_cast<int>(m), 64);
        ca.r += ar, ca.g += ag, ca.b += ab;
        cb.r += br, cb.g += bg, cb.b += bl;
    }
    // lane 0 writes A and lane 1 writes B: adjacent words, one store
    KernArgs* ko = kernargs();
    if (lane < 2u) {
        const bool second = lane != 0u;
        const float isp = ko->inv_spp;
        const PixelOut p{(second ? cb.r : ca.r) * isp, (second ? cb.g : ca.g) * isp, (second ? cb.b : ca.b) * isp};
        const uint32_t rgba = pack_rgba8(p);
        if (!second || b_on) {
            const size_t o = (size_t)oy * ko->W + ox + lane;
            ko->out8[o] = rgba;
            if (ko->out32) ko->out32[o] = make_float4(p.r, p.g, p.b, 1.0f);
        }
    }
    return true;
}

}  // namespace rtamd
