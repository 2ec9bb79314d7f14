// rt_sorted.h — quadrant-sorted rounds: the scene kernels' path for one pixel
// per wave and 2..4 rounds of samples.  Device code; included by
// rt_kernels.hip only, after rt_shade.h.
#pragma once
#include "rt_shade.h"

namespace rtamd {

// ---------------------------------------------------------------------------
// Quadrant-sorted rounds (DESIGN.md 5.1 "Sorted rounds")
//
// At spp > 64 a pixel's samples run in rounds of 64, and a round costs its
// slowest lane.  Where a pixel is about one sphere wide (C5: pixel 0.0017,
// sphere diameter ~0.003 world units) its samples hit different spheres and
// their walks diverge; the oracle's walks put the slowest lane at 1.6x the
// mean (tools/shadow_sim.py).  Samples whose jitter falls in the same pixel
// quadrant are closer, so this path traces a pixel's samples grouped by
// quadrant (stable: a quadrant's samples in index order), 64 at a time,
// parks each colour in the wave's LDS under its sample index, and then sums
// the rounds exactly as shade_wave_tile does: round r = samples 64r..64r+63,
// pairwise, rounds in order.  Same colours, same sums, same image; the model
// predicts 11% fewer primary and 13% fewer shadow trips on C5.
// ---------------------------------------------------------------------------


// Morton cell of sample sg's jitter on a 2^kSortCellBits grid per axis (the
// top bits of each hash are its u01 in those steps): the top two bits are
// the quadrant, and so on down
__device__ __forceinline__ uint32_t jitter_cell(uint32_t hp, uint32_t sg) {
    const uint32_t qu = mix32(hp ^ (sg << 1)) >> (32u - kSortCellBits);
    const uint32_t qv = mix32(hp ^ ((sg << 1) | 1u)) >> (32u - kSortCellBits);
    uint32_t c = 0;
#pragma unroll
    for (uint32_t b = 0; b < kSortCellBits; ++b)
        c |= (((qu >> b) & 1u) << (2u * b)) | (((qv >> b) & 1u) << (2u * b + 1u));
    return c;
}

// Primary ray direction of sample sg of pixel (x, y) (sample_color_unified's).
__device__ __forceinline__ void sample_dir(uint32_t x, uint32_t y, uint32_t hp, uint32_t sg,
                                           float& d0, float& d1, float& d2) {
    KernArgs* ka = kernargs();
    float u = static_cast<float>(x), v = static_cast<float>(y);
    if (ka->jitter) {
        u = u + u01(mix32(hp ^ (sg << 1)));
        v = v + u01(mix32(hp ^ ((sg << 1) | 1u)));
    }
    CamArgs cam;
    for (int i = 0; i < 9; ++i) cam.K[i] = ka->cam.K[i], cam.R[i] = ka->cam.R[i];
    get_ray(cam, u, v, d0, d1, d2);
}

// Hit point and normal of a primary hit (sample_color_unified's shading prep).
struct HitShade {
    float p0, p1, p2, n0, n1, n2, ndl;
};
__device__ __forceinline__ HitShade hit_shade(float d0, float d1, float d2, float t, uint32_t idx,
                                              uint32_t* bs = nullptr) {
    KernArgs* kb = kernargs();
    const float4 sp = kb->sc.prim_sp[idx];
    RT_BS(kBsShadeLoad);
    HitShade h;
    h.p0 = kb->cam.o[0] + t * d0;
    h.p1 = kb->cam.o[1] + t * d1;
    h.p2 = kb->cam.o[2] + t * d2;
    const float ir = 1.0f / sp.w;
    h.n0 = (h.p0 - sp.x) * ir;
    h.n1 = (h.p1 - sp.y) * ir;
    h.n2 = (h.p2 - sp.z) * ir;
    h.ndl = h.n0 * kb->L[0] + h.n1 * kb->L[1] + h.n2 * kb->L[2];
    return h;
}

// One pixel (spw = 64: the wave is one pixel), 2..4 rounds, at pixel (x, y):
//  1. order: the pixel's samples grouped by jitter quadrant;
//  2. primary rays 64 at a time in that order; a miss or an unlit hit is
//     final (its slot holds the colour's inputs), a lit hit parks {t, sphere}
//     and joins the list of lit samples;
//  3. the lit samples' shadow rays 64 at a time (dense: one pixel's lit
//     samples of all rounds together, in quadrant order), each recomputing
//     its hit point from {t, sphere} with the same operations;
//  4. per round in sample order: colours, pairwise sums, rounds in order.
template <class C>
__device__ __forceinline__ void shade_pixel_sorted(const FrameArgs& a, float* wl, void* stk,
                                                   uint32_t x, uint32_t y, uint32_t obase,
                                                   uint32_t& n_primary, uint32_t& n_shadow,
                                                   uint32_t& n_nodes, uint32_t& n_prims,
                                                   uint32_t* bs) {
    constexpr bool kTiles = C::tiles, kStats = C::stats, kProg = C::prog, kOcc = C::occ, kBin = C::bin;
    const SceneArgs& S = a.sc;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t R = a.rounds;
    const bool lane_pix = x < a.W && y < a.H;
    const uint32_t n = lane_pix ? a.spp : 0u;  // this pixel's samples (local indices)
    const uint32_t hp = mix32(a.seedmix ^ (y * a.W + x));
    const uint32_t s_base = kProg ? a.s_base : 0u;
    uint2* slot = reinterpret_cast<uint2*>(wl);
    uint8_t* kind = reinterpret_cast<uint8_t*>(slot + kSortMax);  // 0 miss, 1 hit, 2 lit (in flight)
    uint8_t* ord = kind + kSortMax;
    uint8_t* lit = ord + kSortMax;
    // 1. tracing order: local samples s = 64 j + lane grouped by 4x4 Morton
    //    cell of their jitter (quadrants first): a counting sort over LDS
    //    counters (an LDS atomic gives a sample its place in its cell)
    uint32_t* bcnt = reinterpret_cast<uint32_t*>(lit + kSortMax);
    const bool jit = kernargs()->jitter != 0u;
    if (lane < kSortCells) bcnt[lane] = 0u;
    // (cell << 8 | place in the cell) parked in the sample's slot until placed
    for (uint32_t j = 0; j < R; ++j) {
        const uint32_t sl = 64u * j + lane;
        if (sl < n) {
            const uint32_t cell = jit ? jitter_cell(hp, s_base + sl) : 0u;
            slot[sl].x = (cell << 8) | atomicAdd(bcnt + cell, 1u);
        }
    }
    {  // exclusive prefix of the cells' counts (one per lane)
        const uint32_t v = lane < kSortCells ? bcnt[lane] : 0u;
        uint32_t incl = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t o = __shfl_up(incl, static_cast<unsigned>(d), 64);
            if (static_cast<int>(lane) >= d) incl += o;
        }
        if (lane < kSortCells) bcnt[lane] = incl - v;
    }
    for (uint32_t j = 0; j < R; ++j) {
        const uint32_t sl = 64u * j + lane;
        if (sl < n) {
            const uint32_t kp = slot[sl].x;
            ord[bcnt[kp >> 8] + (kp & 0xFFu)] = static_cast<uint8_t>(sl);
        }
    }
    // (a wave's LDS operations complete in order: no barrier needed)
    // 2. primary rays in that order
    uint32_t nl = 0;  // lit samples listed (wave-uniform)
    for (uint32_t r = 0; r < R; ++r) {
        const uint32_t i = 64u * r + lane;
        const bool valid = i < n;
        const uint32_t sl = valid ? static_cast<uint32_t>(ord[i]) : 0u;
        n_primary += static_cast<uint32_t>(__popcll(__ballot(valid)));  // wave-uniform
        float d0, d1, d2;
        sample_dir(x, y, hp, s_base + sl, d0, d1, d2);
        float t = 0.0f;
        uint32_t idx = 0;
        bool hit = false;
        bool binned = false;
        if (kBin) {  // (x, y) is the wave's one pixel: a 1x1 tile of its bin
            uint2 bh;
            unsigned long long bw;
            const uint32_t bc = bin_frame_consts(0u, 0u);
            binned = !bin_header(x, y, bc, bh, bw);
            if (binned) {
                KernArgs* kc = kernargs();
                hit = bin_nearest(bh, bw, valid, kc->cam.o[0], kc->cam.o[1], kc->cam.o[2], d0, d1, d2, t,
                                  idx, bc);
            }
        }
        if (valid && !binned) {
            RT_BS(kBsPhase);
            KernArgs* kc = kernargs();
            hit = walk<SortedPrimary<kStats>>(S, kc->cam.o[0], kc->cam.o[1], kc->cam.o[2], d0, d1, d2,
                                              0.0f, INFINITY, t, idx, n_nodes, n_prims,
                                              static_cast<uint2*>(stk), false, bs);
        }
        bool is_lit = false;
        if (valid) {
            uint2 sv = make_uint2(__float_as_uint(sat(d1)), __float_as_uint(sat(d2)));
            uint8_t kd = 0;
            if (hit) {
                const HitShade h = hit_shade(d0, d1, d2, t, idx, bs);
                is_lit = h.ndl > 0.0f && kernargs()->shadows;
                if (is_lit) {
                    sv = make_uint2(__float_as_uint(t), idx);
                    kd = 2;
                } else {
                    RT_BS(kBsShadeLoad);
                    sv = make_uint2(__float_as_uint(h.ndl > 0.0f ? h.ndl : 0.0f),
                                    kernargs()->sc.prim_al[idx]);
                    kd = 1;
                }
            }
            slot[sl] = sv;
            kind[sl] = kd;
        }
        const uint64_t lm = __ballot(is_lit);
        if (is_lit) lit[nl + lane_rank(lm)] = static_cast<uint8_t>(sl);
        nl += static_cast<uint32_t>(__popcll(lm));
    }
    n_shadow += nl;
    // 3. the lit samples' shadow rays, 64 at a time
    for (uint32_t c0 = 0; c0 < nl; c0 += 64u) {
        const uint32_t j = c0 + lane;
        const bool has = j < nl;
        const uint32_t sl = has ? static_cast<uint32_t>(lit[j]) : 0u;
        float o0 = 0.f, o1 = 0.f, o2 = 0.f, lam = 0.0f;
        uint32_t idx = 0;
        uint2 occ_hdr = make_uint2(0u, 0u);
        if (has) {
            float d0, d1, d2;
            sample_dir(x, y, hp, s_base + sl, d0, d1, d2);
            const uint2 sv = slot[sl];
            idx = sv.y;
            if (kOcc) occ_hdr = kernargs()->sc.prim_occ[idx];
            const HitShade h = hit_shade(d0, d1, d2, __uint_as_float(sv.x), idx, bs);
            lam = h.ndl > 0.0f ? h.ndl : 0.0f;
            o0 = h.p0 + h.n0 * kShadowEps;
            o1 = h.p1 + h.n1 * kShadowEps;
            o2 = h.p2 + h.n2 * kShadowEps;
        }
        bool occ = false;
        if (kOcc) {
            // answered from the hit spheres' occluder lists (round 7)
            occ = shadow_occluded<true>(S, occ_hdr, has, o0, o1, o2, static_cast<uint2*>(stk));
        } else if (has) {
            RT_BS(kBsPhase);
            RT_BS(kBsPhaseShadow);
            KernArgs* kl = kernargs();
            float ts;
            uint32_t is;
            occ = walk<SortedShadow<kStats>>(
                S, o0, o1, o2, kl->L[0], kl->L[1], kl->L[2], 0.0f, INFINITY, ts, is, n_nodes,
                n_prims, static_cast<uint2*>(stk), true, bs);
        }
        if (has) {
            RT_BS(kBsShadeLoad);
            slot[sl] = make_uint2(__float_as_uint(occ ? 0.0f : lam), kernargs()->sc.prim_al[idx]);
            kind[sl] = 1;
        }
    }
    // 4. the rounds in sample order: colours, pairwise sums (oracle.c:tree_sum),
    //    added in order (shade_wave_tile's arithmetic)
    KernArgs* ko = kernargs();
    float4 A = make_float4(0.f, 0.f, 0.f, 0.f);
    for (uint32_t r = 0; r < R; ++r) {
        const uint32_t i = 64u * r + lane;
        PixelOut c{0.0f, 0.0f, 0.0f};
        if (i < n) {
            const uint2 sv = slot[i];
            if (kind[i]) {
                const float lam = __uint_as_float(sv.x);
                const uint32_t al = sv.y;
                const float amb = ko->ambient;
                const float f = amb + (1.0f - amb) * lam;
                c.r = static_cast<float>(al & 0xFFu) * (1.0f / 255.0f) * f;
                c.g = static_cast<float>((al >> 8) & 0xFFu) * (1.0f / 255.0f) * f;
                c.b = static_cast<float>((al >> 16) & 0xFFu) * (1.0f / 255.0f) * f;
            } else {
                c = PixelOut{200.0f / 255.0f, __uint_as_float(sv.x), __uint_as_float(sv.y)};
            }
        }
        for (uint32_t m = 1; m < 64u; m <<= 1) {
            c.r += __shfl_xor(c.r, static_cast<int>(m), 64);
            c.g += __shfl_xor(c.g, static_cast<int>(m), 64);
            c.b += __shfl_xor(c.b, static_cast<int>(m), 64);
        }
        if (r == 0u) {
            if (kProg && ko->accum_in && lane_pix) {
                const float4 P = ko->accum[(size_t)y * ko->W + x];
                A = make_float4(P.x + c.r, P.y + c.g, P.z + c.b, 0.0f);
            } else {
                A = make_float4(c.r, c.g, c.b, 0.0f);
            }
        } else {
            A = make_float4(A.x + c.r, A.y + c.g, A.z + c.b, 0.0f);
        }
    }
    if (lane == 0u) {
        if (lane_pix) {
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
        } else if (kTiles) {
            ko->out8[obase + y * ko->tile_size + x] = 0u;  // off-image pixel of an edge tile
        }
    }
}

}  // namespace rtamd
