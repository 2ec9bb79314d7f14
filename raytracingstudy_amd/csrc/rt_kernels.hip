// rt_kernels.hip — hand-written HIP kernels for gfx950 (MI355X, CDNA4).
//
// Replaces the reference's single CUDA kernel `raytracing`
// (src/renderer.cu:57-82, grid (W/32+1, H/32+1) x block (32,32)) and its
// <<<1,1>>> setup kernels (src/renderer.cu:84-109):
//   * compat_kernel : byte-exact restatement of `raytracing` (root-box slab
//                     test, R = Octree::traverse() = 200, miss colour).
//   * scene_kernel  : the build-defined octree path (DESIGN.md "Scene mode").
//   * unpack_kernel : scatters packed per-rank tiles into the frame.
// Compiled with -ffp-contract=off: every f32/f64 expression is evaluated in
// source order with IEEE division/sqrt, exactly like oracle/oracle.c.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <utility>
#include <vector>

#include "rt_params.h"
#include "rt_walk.h"  // scene mode: the octree walk (shared with rt_query.hip)
#include "rt_bins.h"  // scene mode: primary rays from the frame's screen-space bins

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

// src/renderer.cu:3-55 — `hit_sphere`: slab test of the root box [0,1.28]^3
// with the negative-direction axes mirrored about the centre 0.64 (f32
// origin/inverse widened to f64, f64 slab products rounded to f32, NaN-dropping
// fmaxf/fminf, no t >= 0 test).
__device__ __forceinline__ double mirror_o(float o, float d) {
    return d < 0.0f ? static_cast<double>(0.64f * 2.0f - o) : static_cast<double>(o);
}
__device__ __forceinline__ double mirror_inv(float d) {
    return d < 0.0f ? static_cast<double>(-(1.0f / d)) : static_cast<double>(1.0f / d);
}
__device__ __forceinline__ bool hit_root_box(const float o[3], float d0, float d1, float d2) {
    const double bmin = static_cast<double>(0.0f);
    const double bmax = static_cast<double>(1.28f);
    const double rx = mirror_o(o[0], d0), ry = mirror_o(o[1], d1), rz = mirror_o(o[2], d2);
    const double ix = mirror_inv(d0), iy = mirror_inv(d1), iz = mirror_inv(d2);
    const float tx0 = static_cast<float>((bmin - rx) * ix);
    const float tx1 = static_cast<float>((bmax - rx) * ix);
    const float ty0 = static_cast<float>((bmin - ry) * iy);
    const float ty1 = static_cast<float>((bmax - ry) * iy);
    const float tz0 = static_cast<float>((bmin - rz) * iz);
    const float tz1 = static_cast<float>((bmax - rz) * iz);
    return fmaxf(fmaxf(tx0, ty0), tz0) < fminf(fminf(tx1, ty1), tz1);
}

// getRay under ONE CANDIDATE contraction of include/camera.h:31-34 (dz = 1
// folds; an fadd of two products fused through its first operand), a guess at
// what nvcc's default -fmad=true does to the reference binary.  Which order
// that binary really uses cannot be checked without nvcc: unpinned
// (DESIGN.md 2.1).  The default (get_ray) is the SOURCE semantics.  Same
// operations as the oracle's contracted getRay, contract = 1.
__device__ __forceinline__ void get_ray_fma(const CamArgs& c, float u, float v, float& wx,
                                            float& wy, float& wz) {
    const float dx = (u - c.K[2]) / c.K[0];
    const float dy = (v - c.K[5]) / c.K[4];
    wx = fmaf(c.R[0], dx, c.R[3] * dy) + c.R[6];
    wy = fmaf(c.R[1], dx, c.R[4] * dy) + c.R[7];
    wz = fmaf(c.R[2], dx, c.R[5] * dy) + c.R[8];
    const float len = sqrtf(fmaf(wz, wz, fmaf(wx, wx, wy * wy)));
    wx /= len;
    wy /= len;
    wz /= len;
}

__device__ __forceinline__ uint32_t compat_pixel(const CamArgs& cam, uint32_t x, uint32_t y,
                                                 uint32_t contract) {
    float d0, d1, d2;
    if (contract)
        get_ray_fma(cam, static_cast<float>(x), static_cast<float>(y), d0, d1, d2);
    else
        get_ray(cam, static_cast<float>(x), static_cast<float>(y), d0, d1, d2);
    if (hit_root_box(cam.o, d0, d1, d2)) return 0xFFFFFFFFu;
    const uint32_t g = static_cast<uint32_t>(sat(d1) * 255.0f);
    const uint32_t b = static_cast<uint32_t>(sat(d2) * 255.0f);
    return 200u | (g << 8) | (b << 16) | (255u << 24);
}

// One wave = 64 consecutive pixels of a row; one packed 32-bit store per lane.
__global__ void __launch_bounds__(kBlockThreads) compat_kernel(FrameArgs a) {
    const uint32_t x = blockIdx.x * 64u + (threadIdx.x & 63u);
    const uint32_t y = blockIdx.y * 4u + (threadIdx.x >> 6);
    if (x >= a.W || y >= a.H) return;
    __builtin_nontemporal_store(compat_pixel(a.cam, x, y, a.contract), a.out8 + (size_t)y * a.W + x);
}

// Tile-packed compat: block = 64 x 4 strip of one tile.
__global__ void __launch_bounds__(kBlockThreads) compat_tiles_kernel(FrameArgs a) {
    const uint32_t ts = a.tile_size;
    const uint32_t strips = ts / 4u * (ts / 64u);
    const uint32_t k = blockIdx.x / strips;
    const uint32_t sidx = blockIdx.x % strips;
    const uint32_t lx = (sidx % (ts / 64u)) * 64u + (threadIdx.x & 63u);
    const uint32_t ly = (sidx / (ts / 64u)) * 4u + (threadIdx.x >> 6);
    const uint32_t tile = a.tiles[k];
    const uint32_t x = (tile % a.tiles_x) * ts + lx;
    const uint32_t y = (tile / a.tiles_x) * ts + ly;
    const uint32_t v = (x < a.W && y < a.H) ? compat_pixel(a.cam, x, y, a.contract) : 0u;
    a.out8[(size_t)k * ts * ts + ly * ts + lx] = v;
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

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// Stats frames only.  Every wave adds its counts as it exits, so the adds
// all land in the frame's tail: on ONE cache line they serialise there and
// stall the last waves' loads behind them (plain frames that still flushed
// were 4.3% slower on C3 and 17% on a 1/8 tile share, profiles/r02/flush_ab.log).
// One line per XCD group cuts the queue per line 8x; the host sums the lines.
__device__ __forceinline__ void flush_counters(const FrameArgs& a, uint32_t prim, uint32_t shadow,
                                               uint32_t nodes, uint32_t prims) {
    // ray counts are wave-uniform already (ballot counts); the work counters
    // are per lane
    const unsigned long long s0 = prim;
    const unsigned long long s1 = shadow;
    const unsigned long long s2 = wave_sum(nodes);
    const unsigned long long s3 = wave_sum(prims);
    if ((threadIdx.x & 63u) == 0) {
        unsigned long long* c = a.counters + kStatLineBase + (blockIdx.x & 7u) * kStatLineStride;
        atomicAdd(c + 0, s0);
        atomicAdd(c + 1, s1);
        atomicAdd(c + 2, s2);
        atomicAdd(c + 3, s3);
    }
}

// The hit record a nearest walk returned (`iout`, a leaf reference): its
// sphere and its packed albedo.
// (SA: SceneArgs, or the kernel arguments' copy behind kernargs())
template <typename SA>
__device__ __forceinline__ float4 hit_sphere_rec(SA& S, uint32_t h) {
    return S.prim_sp[h];
}
template <typename SA>
__device__ __forceinline__ uint32_t hit_albedo(SA& S, uint32_t h) {
    return S.prim_al[h];
}

// Unified lane path: one walk instance run twice (primary, then the shadow ray
// of the lanes that need one), so the register allocator sees one walk.
// kBin: the primary ray is answered from the frame's screen-space bins
// (rt_bins.h; (tox, toy): the wave tile's origin pixel, wave-uniform); a tile
// whose bin is over the cap, or a frame whose builder raised its flag, walks
// under a wave-uniform branch.
template <int kChunk, bool kStats, bool kCam8 = false, bool kOcc = false, bool kBin = false>
__device__ __forceinline__ PixelOut sample_color_unified(const FrameArgs& a, uint32_t x,
                                                         uint32_t y, uint32_t hp, uint32_t s,
                                                         bool valid, uint32_t& n_shadow,
                                                         uint32_t& n_nodes, uint32_t& n_prims,
                                                         void* stk, uint32_t* bs, uint32_t lbs,
                                                         uint32_t tox = 0, uint32_t toy = 0) {
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
            binned = !bin_header(tox, toy, bh);
            if (binned)
                hit = bin_nearest(bh, tox, toy, kernargs()->tw, kernargs()->th, active, r0, r1, r2, d0,
                                  d1, d2, t, idx);
        }
        if (active && !binned) {
            RT_BS(kBsPhase);
            if (phase) RT_BS(kBsPhaseShadow);
            if (phase == 0)
                hit = walk<false, kChunk, false, kStats, false, false, kCam8>(S, r0, r1, r2, d0, d1, d2, 0.0f, INFINITY, t,
                                                         idx, n_nodes, n_prims,
                                                         static_cast<uint2*>(stk), false, bs, lbs);
            else if (kOcc) {
                // answered from the hit sphere's occluder list (round 7)
                hit = shadow_occluded<false>(S, occ_hdr, true, r0, r1, r2, static_cast<uint2*>(stk));
            } else {
                // the shadow direction L is the frame's, the same in every
                // lane: read afresh from the kernel arguments (SGPRs), not the
                // lanes' d registers
                KernArgs* kl = kernargs();
                // (2 spheres a chunk, one dwordx4 of 8-byte records: 4 spills
                // 48-100 B, C3 +6%, C5 +8%, C5d +5%, profiles/r06/ab_shd_chunk4.log)
                hit = walk<true, 2, false, kStats, false, true>(
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
                const float4 sp = hit_sphere_rec(kb->sc, idx);
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
                al = hit_albedo(kb->sc, idx);
                if (kOcc && want_shadow) occ_hdr = kb->sc.prim_occ[idx];
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
template <bool kTiles, int kChunk, bool kStats, bool kProg, bool kCam8 = false, bool kOcc = false,
          bool kBin = false>
__device__ __forceinline__ void shade_wave_tile(const FrameArgs& a, float4* acc, void* stk,
                                                uint32_t ox, uint32_t oy, uint32_t obase,
                                                uint32_t& n_primary,
                                                uint32_t& n_shadow, uint32_t& n_nodes,
                                                uint32_t& n_prims, uint32_t* bs, uint32_t lbs) {
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
        PixelOut c = sample_color_unified<kChunk, kStats, kCam8, kOcc, kBin>(a, x, y, hp, sg, valid, n_shadow,
                                                          n_nodes, n_prims, stk, bs, lbs, ox, oy);
        // Pixel sum of this round: pairwise butterfly over the pixel's g
        // lanes (missing samples are 0) = oracle.c:tree_sum; rounds are then
        // added in order in the leader's LDS slot.
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
    const float4 sp = hit_sphere_rec(kb->sc, idx);
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
template <bool kTiles, int kChunk, bool kStats, bool kProg, bool kOcc = false, bool kBin = false>
__device__ __forceinline__ void shade_pixel_sorted(const FrameArgs& a, float* wl, void* stk,
                                                   uint32_t x, uint32_t y, uint32_t obase,
                                                   uint32_t& n_primary, uint32_t& n_shadow,
                                                   uint32_t& n_nodes, uint32_t& n_prims,
                                                   uint32_t* bs) {
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
            binned = !bin_header(x, y, bh);
            if (binned) {
                KernArgs* kc = kernargs();
                hit = bin_nearest(bh, x, y, 1u, 1u, valid, kc->cam.o[0], kc->cam.o[1], kc->cam.o[2], d0, d1,
                                  d2, t, idx);
            }
        }
        if (valid && !binned) {
            RT_BS(kBsPhase);
            KernArgs* kc = kernargs();
            hit = walk<false, kChunk, true, kStats, true, false, true>(S, kc->cam.o[0], kc->cam.o[1], kc->cam.o[2],
                                                          d0, d1, d2, 0.0f, INFINITY, t, idx, n_nodes,
                                                          n_prims, static_cast<uint2*>(stk), false, bs);
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
                                    hit_albedo(kernargs()->sc, idx));
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
            occ = walk<false, 2, true, kStats, true, true>(
                S, o0, o1, o2, kl->L[0], kl->L[1], kl->L[2], 0.0f, INFINITY, ts, is, n_nodes,
                n_prims, static_cast<uint2*>(stk), true, bs);
        }
        if (has) {
            RT_BS(kBsShadeLoad);
            slot[sl] = make_uint2(__float_as_uint(occ ? 0.0f : lam), hit_albedo(kernargs()->sc, idx));
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

// Work scheduling (persistent workgroups: grid = resident workgroups):
//
// kWaveQ = false: workgroups pull bts x bts block tiles from ONE device-wide
//   queue head (a returning atomic per tile); the tile's wave tiles are dealt
//   to the 4 waves round-robin, and the workgroup syncs per tile.
// kWaveQ = true: every WAVE pulls tickets of 1-4 wave tiles on its own.  The
//   wave tiles are numbered in 8x8 blocks (spatially coherent) of 8x8-block
//   superblocks; whole superblocks go to XCD groups (blockIdx % 8: blocks are
//   dealt round-robin over the 8 XCDs, MI355X_MICROARCH.md "Workgroup
//   dispatch") in claim order, and each XCD has its own ticket head on its
//   own cache line (one head saturates near 88 dequeues/us) over the
//   superblocks it claimed: the two-level queue below.  No workgroup barrier;
//   the tail is one ticket.
//
// kMinW = minimum waves per SIMD requested from the register allocator.
// kProg: progressive frame (a.accum set); compiled separately so plain frames
// keep their register budget.
// Residency of the wave-queue builds is set by SGPRs, not VGPRs: at 60-65
// VGPRs and 94 SGPRs (112 allocated) a SIMD holds 7 waves.  The 8-wave build
// caps its SGPRs at 80 (the rest spill into VGPR lanes, no scratch), and 8
// waves fit: C3 -1.9%, its tile path -3.3%, C5 -2.4% (84: 8 do not fit; 76
// and 72: the extra spills cost more; profiles/r02/sgpr_ab.log).
// scene_kernel_w8 below is that build of the timed default.
template <bool kTiles, int kChunk, bool kStats = true, bool kProg = false, bool kWaveQ = false,
          bool kSort = false, bool kOcc = false, bool kBin = false>
__device__ __forceinline__ void scene_body(FrameArgs a) {
    static_assert(!kOcc || !kStats, "stats frames walk: their counters are the oracle's");
    static_assert(!kBin || (!kStats && kWaveQ), "bins: plain frames of the wave queue");
    extern __shared__ __attribute__((aligned(16))) float4 lds[];
    float4* acc = lds;  // [256] running pixel sums (leader lanes' slots)
    const uint32_t wave = threadIdx.x >> 6;
    // sorted rounds: no per-thread pixel sums; stacks first, then each wave's
    // colours and tracing order (sort_lds_bytes)
    void* stk = reinterpret_cast<uint2*>(lds + (kSort ? 0u : kBlockThreads)) + threadIdx.x;
    float* wl = kSort ? reinterpret_cast<float*>(reinterpret_cast<uint2*>(lds) +
                                                 stack_levels(a.sc, true) * kBlockThreads) +
                            wave * (kSortWaveBytes / 4u)
                      : nullptr;
    // the walks' LDS leaf buffer base as a wave-uniform value (an SGPR, or a
    // lane of the SGPR spill VGPR), handed down to walk(): computed from
    // threadIdx inside the walk it lived in a VGPR, which the sorted 64-VGPR
    // build spilled to scratch and reloaded (a scratch load and a vmcnt(0)
    // wait) on every staged leaf.  C5 -1.2%, C5d -0.3% (sorted), C3 -0.4%
    // (profiles/r06/ab_leaf_base_*.log)
    const uint32_t lbs = __builtin_amdgcn_readfirstlane(leaf_buf_base(a.sc, kSort));
    // the next frame's counters, queue heads and slot table (the other set,
    // FrameArgs::ctr_next): zeroed here by the first workgroup, so frames run
    // back to back with no memset launch between them.  The previous frame,
    // which used that set, completed before this one started.
    // (fields read through kernargs(): nothing of this stays live in SGPRs)
    if (blockIdx.x == 0) {
        KernArgs* kz = kernargs();
        for (uint32_t i = threadIdx.x; i < kz->ctr_next_words; i += kBlockThreads) kz->ctr_next[i] = 0ull;
    }
    const uint32_t tw = a.tw, th = a.th;
    uint32_t n_shadow = 0, n_nodes = 0, n_prims = 0, n_primary = 0;
#ifdef RT_BLOCK_STATS
    uint32_t bs[2 * kBlockStats] = {};
#else
    uint32_t* bs = nullptr;
#endif
#ifdef RT_TIMELINE
    // diagnostic build only (tools/timeline.sh): per-wave {start, first empty
    // range, exit, units} in wall-clock ticks
    const unsigned long long tl_start = wall_clock64();
    unsigned long long tl_empty = 0, tl_units = 0;
#endif
    if (kWaveQ) {
        // wave-tile grid of the frame, or of one packed tile
        const uint32_t gw = kTiles ? a.tile_size / tw : (a.W + tw - 1) / tw;
        const uint32_t gh = kTiles ? a.tile_size / th : (a.H + th - 1) / th;
        const uint32_t nbx = (gw + 7u) / 8u, nby = (gh + 7u) / 8u;
        // superblock = 8x8 blocks of 8x8 wave tiles (one 64x64 tile at 64 spp)
        const uint32_t nsx = (nbx + 7u) / 8u, nsy = (nby + 7u) / 8u;
        const uint32_t sb_grid = nsx * nsy;  // superblocks per grid
        const uint32_t n_sb = kTiles ? a.n_tiles * sb_grid : sb_grid;
        // Two-level queue.  Level 1 hands whole superblocks (4096 wave tiles,
        // one 64x64 tile at 64 spp) to XCDs in claim order from one counter;
        // level 2 is a per-XCD ticket head over the XCD's own sequence of
        // superblocks ("slots": slot s = units [4096 s, 4096 s + 4096) of that
        // head).  An XCD's waves thus share one image region at a time (its
        // L2 holds that region's part of the scene), no unit ever runs on
        // another XCD (a stolen unit runs 3-6x slower, L2-cold), and the XCDs
        // still balance dynamically at superblock granularity (uneven scenes).
        // The ticket holding the middle unit of slot s claims slot s + 1 half
        // a slot early, so waves arriving at a new slot find it published;
        // ticket 0 claims slot 0.  A claim past the last superblock publishes
        // kSlotNone and the waves that reach it exit.  Launches of fewer
        // than 192 superblocks (a multi-GPU tile share, small frames) claim
        // single 8x8 blocks instead (slot = 64 units), numbered over the
        // blocks that hold wave tiles: the XCDs then run dry within a block
        // of each other, not within a superblock (1/8 C3 share -4%), and a
        // small frame never dequeues a superblock of padding.
        const uint32_t q = blockIdx.x & 7u;  // this workgroup's XCD (round-robin dispatch)
        unsigned long long* head = a.counters + kWaveQueueBase + q * kWaveQueueStride;
        unsigned long long* claims = a.counters + kWaveQueueClaim;
        uint32_t* slots = a.wq_slots + q * a.wq_slot_stride;
        const uint32_t chunk = a.wq_chunk;  // wave tiles per ticket (divides 32)
        const uint32_t ks = a.wq_slot_shift;  // 12: superblock slots, 6: block slots
        const uint32_t nbb = nbx * nby;       // blocks per grid
        const uint32_t n1 = ks == 12u ? n_sb : (kTiles ? a.n_tiles : 1u) * nbb;  // level-1 units
        const uint32_t half = 1u << (ks - 1u);
        // the current slot's grid (packed tile) and origin in wave tiles
        uint32_t cached_s = ~0u, k = 0, sx0 = 0, sy0 = 0, tox = 0, toy = 0, obase = 0;
        uint32_t owed = 0;  // the last real slot this wave claimed (see below)
        for (;;) {
            uint32_t t = 0;
            if ((threadIdx.x & 63u) == 0) t = static_cast<uint32_t>(atomicAdd(head, 1ull));
            const uint32_t u0 = __builtin_amdgcn_readfirstlane(t) * chunk;
            const uint32_t s = u0 >> ks, w0 = u0 & ((1u << ks) - 1u);
            const bool lead = (threadIdx.x & 63u) == 0;
            // The ticket holding slot s's middle unit claims slot s + 1 as soon
            // as it has its ticket (ticket 0 claims slot 0), before it waits
            // on anything, so claims run in parallel and land half a slot
            // early.  Two claims of one XCD can then be taken from the
            // counter out of slot order: at the counter's end slot s may hold
            // kSlotNone while slot s + 1 holds the last block.  Round 4's
            // waves all left at their first empty slot, and that block was
            // lost when every wave of the XCD had drawn one of slot s's
            // tickets (13 of 1,800 first frames; test_gpu_variants.py
            // test_wave_queue_claims_in_slot_order).  Now the wave that
            // claimed a real slot t (`owed` = t) does not leave before its
            // tickets reach slot t: every ticket up to there is drawn by a
            // live wave, so slot t's units all run.  The other waves leave at
            // their first empty slot as before.  Claiming in slot order (each
            // claim after the previous slot is published) is correct too but
            // chains the claims into serial memory round trips, C2 +5..19%;
            // keeping every wave until two empty slots in a row costs C2
            // +12% in head atomics (profiles/r05/queue_order_ab.log).
            uint32_t mine = 0;  // the slot this ticket claimed, if it got a real one
            if (lead && (u0 == 0u || (w0 <= half && half < w0 + chunk))) {
                // (test only: hold XCD 0's first claim back until the other
                // claims of its first slots would have been taken)
                if (q == 0u && u0 == 0u) {
                    for (uint32_t d = kernargs()->wq_claim_delay; d; --d) __builtin_amdgcn_s_sleep(127);
                    // (test only, RT_TEST_FAULT=queue:k: report this frame as failed)
                    if (kernargs()->test_fault_queue) frame_failed();
                }
                const uint32_t slot = u0 == 0u ? 0u : s + 1u;
                const uint32_t g = static_cast<uint32_t>(atomicAdd(claims, 1ull));
                if (slot < a.wq_slot_stride)
                    __hip_atomic_store(slots + slot, g < n1 ? g + 1u : kSlotNone, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
                if (g < n1) mine = slot;
            }
            owed = max(owed, __builtin_amdgcn_readfirstlane(mine));
            uint32_t e = kSlotNone;
            if (s != cached_s) {  // resolve the slot's superblock or block (published, or soon)
                if (lead && s < a.wq_slot_stride) {
                    // the claimer holds a ticket already and publishes before it
                    // waits on anything; the cap (~1 s) only turns a broken
                    // invariant into a flagged, visibly wrong frame, not a hang
                    for (uint32_t spin = 0;; ++spin) {
                        e = __hip_atomic_load(slots + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        if (e != 0u) break;
                        if (spin == (1u << 22)) {
                            frame_failed();
                            e = kSlotNone;
                            break;
                        }
                        __builtin_amdgcn_s_sleep(8);
                    }
                }
                e = __builtin_amdgcn_readfirstlane(e);
#ifndef RT_TEST_CLAIM_RULE_R4  // (test-only build of round 4's rule: the negative
                               // control of tests/test_gpu_queue_report.py)
                if (e == kSlotNone && s < owed) continue;  // a slot this wave claimed is ahead
#endif
            }
            if (s != cached_s) {
#ifdef RT_TIMELINE
                if (e == kSlotNone && !tl_empty) tl_empty = wall_clock64();
#endif
                if (e == kSlotNone) break;
                cached_s = s;
                const uint32_t g = e - 1u;
                if (ks == 12u) {
                    k = kTiles ? g / sb_grid : 0u;
                    uint32_t sg = g - k * sb_grid;
                    // claim order -> superblock: row-major, or a space-filling
                    // order (FrameArgs::sb_order, RT_SB_ORDER) in which an
                    // XCD's successive claims lie near each other
                    if (!kTiles) {
                        const uint32_t* so = kernargs()->sb_order;
                        if (so) sg = so[sg];
                    }
                    sx0 = (sg % nsx) * 64u;
                    sy0 = (sg / nsx) * 64u;
                } else {
                    // the grid's blocks that hold wave tiles, numbered
                    // superblock by superblock (row-major superblocks; edge
                    // superblocks hold vr x vc blocks)
                    k = kTiles ? g / nbb : 0u;
                    const uint32_t r = g - k * nbb;
                    const uint32_t sy = r / (8u * nbx);
                    const uint32_t vr = min(8u, nby - sy * 8u);
                    const uint32_t r1 = r - sy * 8u * nbx;
                    const uint32_t sx = r1 / (vr * 8u);
                    const uint32_t vc = min(8u, nbx - sx * 8u);
                    const uint32_t r2 = r1 - sx * vr * 8u;
                    sx0 = (sx * 8u + r2 % vc) * 8u;
                    sy0 = (sy * 8u + r2 / vc) * 8u;
                }
                if (kTiles) {  // the packed tile's origin in the image, once per slot
                    const uint32_t tile = a.tiles[k];
                    const uint32_t ts = a.tile_size;
                    tox = (tile % a.tiles_x) * ts;
                    toy = (tile / a.tiles_x) * ts;
                    obase = k * ts * ts - toy * ts - tox;
                }
            }
            for (uint32_t cur = w0; cur < w0 + chunk; ++cur) {
                const uint32_t b = cur >> 6, w = cur & 63u;  // b = 0 in block slots
                const uint32_t wx = sx0 + (b & 7u) * 8u + (w & 7u);
                const uint32_t wy = sy0 + (b >> 3) * 8u + (w >> 3);
                if (wx >= gw || wy >= gh) continue;  // padding of an edge block
                const uint32_t olx = wx * tw, oly = wy * th;
                const uint32_t ox = olx + tox, oy = oly + toy;
#ifdef RT_TIMELINE
                const unsigned long long tu0 = wall_clock64();
#endif
                if (kSort)
                    shade_pixel_sorted<kTiles, kChunk, kStats, kProg, kOcc, kBin>(
                        a, wl, stk, ox, oy, obase, n_primary, n_shadow, n_nodes, n_prims, bs);
                else
                    shade_wave_tile<kTiles, kChunk, kStats, kProg, !kSort, kOcc, kBin>(
                        a, acc, stk, ox, oy, obase, n_primary, n_shadow, n_nodes, n_prims, bs, lbs);
#ifdef RT_TIMELINE
                // per unit {start, end, hw_id << 32 | xcc << 16 | wave index}
                // after the 65536 per-wave records
                const uint32_t sbt = k * sb_grid + (wy >> 6) * nsx + (wx >> 6);
                const unsigned long long uid = (unsigned long long)sbt * 4096u +
                                               (((wy >> 3) & 7u) * 8u + ((wx >> 3) & 7u)) * 64u +
                                               (wy & 7u) * 8u + (wx & 7u);
                if (a.timeline && (threadIdx.x & 63u) == 0 && uid < (1ull << 22)) {
                    const unsigned hw = __builtin_amdgcn_s_getreg((31 << 11) | 4);   // HW_ID
                    const unsigned xcc = __builtin_amdgcn_s_getreg((3 << 11) | 20);  // XCC_ID
                    a.timeline[4ull * 65536 + 3 * uid] = tu0;
                    a.timeline[4ull * 65536 + 3 * uid + 1] = wall_clock64();
                    a.timeline[4ull * 65536 + 3 * uid + 2] =
                        ((unsigned long long)hw << 32) | (xcc << 16) | (blockIdx.x * 4u + wave);
                }
#endif
            }
        }
    } else {
        __shared__ uint32_t tile_slot;
        const uint32_t bts = a.bts;  // block-tile side (16, or 8/4 for small frames)
        const uint32_t wtx = bts / tw, wtiles = wtx * (bts / th);
        const uint32_t per_tile = kTiles ? (a.tile_size / bts) * (a.tile_size / bts) : 0u;
        const uint32_t bx_n = (a.W + bts - 1) / bts;
        const uint32_t n_bt = kTiles ? a.n_tiles * per_tile : bx_n * ((a.H + bts - 1) / bts);
        for (;;) {
            __syncthreads();  // every wave is done with the previous tile_slot
            if (threadIdx.x == 0)
                tile_slot = static_cast<uint32_t>(atomicAdd(a.counters + kQueueSlot, 1ull));
            __syncthreads();
            const uint32_t bt = tile_slot;
            if (bt >= n_bt) break;
            uint32_t ox, oy, obase = 0;  // block-tile origin (frame / packed tile)
            if (kTiles) {
                const uint32_t ts = a.tile_size, tpr = ts / bts;
                const uint32_t k = bt / per_tile;
                const uint32_t b = bt - k * per_tile;
                const uint32_t tile = a.tiles[k];
                const uint32_t tox = (tile % a.tiles_x) * ts, toy = (tile / a.tiles_x) * ts;
                ox = tox + (b % tpr) * bts;
                oy = toy + (b / tpr) * bts;
                obase = k * ts * ts - toy * ts - tox;
            } else {
                ox = (bt % bx_n) * bts;
                oy = (bt / bx_n) * bts;
            }
            for (uint32_t wt = wave; wt < wtiles; wt += kBlockThreads / 64) {
                const uint32_t wox = (wt % wtx) * tw, woy = (wt / wtx) * th;
#ifdef RT_TIMELINE
                const unsigned long long tu0 = wall_clock64();
#endif
                shade_wave_tile<kTiles, kChunk, kStats, kProg, false, kOcc>(
                    a, acc, stk, ox + wox, oy + woy, obase, n_primary, n_shadow, n_nodes,
                    n_prims, bs, lbs);
#ifdef RT_TIMELINE
                // per wave tile of a block tile: {start, end, hw_id << 32 | xcc << 16 |
                // wave index}, unit id = block tile * 16 + wave tile (tools/timeline.py)
                const unsigned long long uid = (unsigned long long)bt * 16u + wt;
                if (a.timeline && (threadIdx.x & 63u) == 0 && uid < (1ull << 22)) {
                    const unsigned hw = __builtin_amdgcn_s_getreg((31 << 11) | 4);   // HW_ID
                    const unsigned xcc = __builtin_amdgcn_s_getreg((3 << 11) | 20);  // XCC_ID
                    a.timeline[4ull * 65536 + 3 * uid] = tu0;
                    a.timeline[4ull * 65536 + 3 * uid + 1] = wall_clock64();
                    a.timeline[4ull * 65536 + 3 * uid + 2] =
                        ((unsigned long long)hw << 32) | (xcc << 16) | (blockIdx.x * 4u + wave);
                }
#endif
            }
        }
    }
    if (kStats) flush_counters(a, n_primary, n_shadow, n_nodes, n_prims);
#ifdef RT_BLOCK_STATS
    if (a.bstats) {
#pragma unroll
        for (uint32_t i = 0; i < 2 * kBlockStats; ++i) {
            const unsigned long long v = wave_sum(bs[i]);
            if ((threadIdx.x & 63u) == 0) atomicAdd(a.bstats + i, v);
        }
    }
#endif
#ifdef RT_TIMELINE
    tl_units = n_primary / 64u;  // samples cast by the wave / 64
    if (a.timeline && (threadIdx.x & 63u) == 0) {
        unsigned long long* e = a.timeline + 4ull * (blockIdx.x * (kBlockThreads / 64) + wave);
        e[0] = tl_start;
        e[1] = tl_empty;
        e[2] = wall_clock64();
        e[3] = tl_units;
    }
#endif
}

template <bool kTiles, int kMinW, int kChunk, bool kStats = true, bool kProg = false,
          bool kWaveQ = false, bool kSort = false, bool kOcc = false>
__global__ void __launch_bounds__(kBlockThreads, kMinW) scene_kernel(FrameArgs a) {
    scene_body<kTiles, kChunk, kStats, kProg, kWaveQ, kSort, kOcc>(a);
}

// The timed default for spp >= 8 (variant 13, plain frames): 8 waves per SIMD,
// SGPRs capped so that they fit (see above).
// kOcc: shadow rays answered from the occluder lists (a scene that has them)
// kBin: primary rays answered from the frame's screen-space bins (a frame that built them)
template <bool kTiles, bool kProg = false, bool kSort = false, bool kOcc = false, bool kBin = false>
__global__ void __launch_bounds__(kBlockThreads, 8) __attribute__((amdgpu_num_sgpr(80)))
    scene_kernel_w8(FrameArgs a) {
    scene_body<kTiles, 2, false, kProg, true, kSort, kOcc, kBin>(a);
}

// Camera-relative screen records of every leaf reference (and the kPrimPad
// tail) for camera origin o (SceneArgs::prim_cam):
// {o - c in f32, exactly isect's oc}, and C' = |o - c|^2 - r^2 minus the
// slack, computed in f64 and rounded toward -inf, so C' <= the bound the
// screen's soundness needs.  One thread per reference: 16 B read, 16 B written.
__global__ void __launch_bounds__(kBlockThreads)
    cam_screen_kernel(const float4* __restrict__ prim_sp, uint32_t n, float ox, float oy, float oz,
                      float4* __restrict__ out) {
    const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
    if (i >= n) return;
    const float4 c = prim_sp[i];
    const float x = ox - c.x, y = oy - c.y, z = oz - c.z;
    const double oo = static_cast<double>(x) * x + static_cast<double>(y) * y + static_cast<double>(z) * z;
    const double rr = static_cast<double>(c.w) * c.w;
    const double u = 1.0 / 16777216.0;  // 2^-24, the f32 unit roundoff
    const double cd = oo - rr - (kScreenSlackOc * u) * oo - (kScreenSlackR * u) * rr;
    out[i] = make_float4(x, y, z, __double2float_rd(cd));
}

// Light-plane screen records (SceneArgs::prim_shd8): per
// reference the centre's {u, v} = {c.e1, c.e2} (f64, rounded to nearest); the
// radius term is the largest rr' = ((r (1 + 4u) + delta)^2 (1 + 4u)) rounded
// up, delta = the slack for this scene (kShadowSlackM u M).  One thread per
// reference.
__global__ void __launch_bounds__(kBlockThreads)
    shd_screen_kernel(const float4* __restrict__ prim_sp, uint32_t n, float e0, float e1, float e2,
                      float e3, float e4, float e5, double delta, float2* __restrict__ out8,
                      uint32_t* __restrict__ rr_max) {
    const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
    uint32_t rb = 0u;
    if (i < n) {
        const float4 c = prim_sp[i];
        const double u = static_cast<double>(c.x) * e0 + static_cast<double>(c.y) * e1 + static_cast<double>(c.z) * e2;
        const double v = static_cast<double>(c.x) * e3 + static_cast<double>(c.y) * e4 + static_cast<double>(c.z) * e5;
        const double ur = 1.0 / 16777216.0;
        const double rg = static_cast<double>(c.w) * (1.0 + 4.0 * ur) + delta;
        const float rr = __double2float_ru(rg * rg * (1.0 + 4.0 * ur));
        out8[i] = make_float2(static_cast<float>(u), static_cast<float>(v));
        rb = __float_as_uint(rr);
    }
    // the largest rr' (non-negative floats order as their bits; a NaN
    // radius, the test-only pad fill, orders above every number): the
    // block's maximum into rr_max[blockIdx.x], reduced by max_bits_kernel
    // (atomics on one word serialise across the XCDs: one per record, or one
    // per wave, took C5d's 4.9 M records 0.87 ms)
    __shared__ uint32_t wmax[kBlockThreads / 64];
    for (int d = 32; d > 0; d >>= 1) rb = max(rb, static_cast<uint32_t>(__shfl_xor(static_cast<int>(rb), d, 64)));
    if ((threadIdx.x & 63u) == 0u) wmax[threadIdx.x >> 6] = rb;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t m = 0u;
        for (uint32_t w = 0; w < kBlockThreads / 64; ++w) m = max(m, wmax[w]);
        rr_max[blockIdx.x] = m;
    }
}

// out[0] = the largest of in[0 .. n) (one block)
__global__ void __launch_bounds__(kBlockThreads)
    max_bits_kernel(const uint32_t* __restrict__ in, uint32_t n, uint32_t* __restrict__ out) {
    __shared__ uint32_t wmax[kBlockThreads / 64];
    uint32_t m = 0u;
    for (uint32_t i = threadIdx.x; i < n; i += kBlockThreads) m = max(m, in[i]);
    for (int d = 32; d > 0; d >>= 1) m = max(m, static_cast<uint32_t>(__shfl_xor(static_cast<int>(m), d, 64)));
    if ((threadIdx.x & 63u) == 0u) wmax[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t w = 1; w < kBlockThreads / 64; ++w) m = max(m, wmax[w]);
        out[0] = m;
    }
}

hipError_t launch_shd_screen(const float4* prim_sp, uint32_t n, const float e[6], double delta,
                             float2* out8, uint32_t* rr_max, hipStream_t st) {
    // rr_max: (blocks + 1) words, the scene's largest rr' bits in the last
    if (n) {
        const uint32_t nb = (n + kBlockThreads - 1) / kBlockThreads;
        hipLaunchKernelGGL(shd_screen_kernel, dim3(nb), dim3(kBlockThreads), 0, st, prim_sp, n, e[0],
                           e[1], e[2], e[3], e[4], e[5], delta, out8, rr_max);
        hipLaunchKernelGGL(max_bits_kernel, dim3(1), dim3(kBlockThreads), 0, st, rr_max, nb, rr_max + nb);
    }
    return hipGetLastError();
}

hipError_t launch_cam_screen(const float4* prim_sp, uint32_t n, const float o[3], float4* out,
                             hipStream_t st) {
    if (n) {
        hipLaunchKernelGGL(cam_screen_kernel, dim3((n + kBlockThreads - 1) / kBlockThreads),
                           dim3(kBlockThreads), 0, st, prim_sp, n, o[0], o[1], o[2], out);
    }
    return hipGetLastError();
}

// Image-plane screen records (SceneArgs::prim_cam8).
// For basis B (f32 rows, orthonormal to f32 rounding) and camera origin o,
// a sphere's centre direction a = B(c - o)/|c - o| projects to q = a.xy/a.z.
// A ray the exact test accepts passes within r' = r (1 + 1e-6) of c, so its
// direction b is within theta (sin theta = r'/|c - o|) of a, and for unit
// vectors |q_a - q_b| <= |a x b| / (a_z b_z) <= sin theta / (a_z cos(beta +
// theta)), beta the angle of a from B's z axis.  rho adds the f32 errors of
// the lane's point (4e-6 (1 + |q| + rho)^2, ~5x the bound), the stored
// centre's (its 8 low mantissa bits carry rho^2: <= 2^-14 |q| a component)
// and 1e-5 relative; rho^2 is rounded up to bf16.  Spheres near or behind
// the camera plane, or a frame whose rays B does not keep in front (ok = 0),
// get rho^2 = +inf: always passed.
__global__ void __launch_bounds__(kBlockThreads)
    cam8_screen_kernel(const float4* __restrict__ prim_sp, uint32_t n, float ox, float oy, float oz,
                       float b0, float b1, float b2, float b3, float b4, float b5, float b6, float b7,
                       float b8, uint32_t ok, float2* __restrict__ out) {
    const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
    if (i >= n) return;
    const float4 c = prim_sp[i];
    const double vx = static_cast<double>(c.x) - ox, vy = static_cast<double>(c.y) - oy,
                 vz = static_cast<double>(c.z) - oz;
    const double X = static_cast<double>(b0) * vx + static_cast<double>(b1) * vy + static_cast<double>(b2) * vz;
    const double Y = static_cast<double>(b3) * vx + static_cast<double>(b4) * vy + static_cast<double>(b5) * vz;
    const double Z = static_cast<double>(b6) * vx + static_cast<double>(b7) * vy + static_cast<double>(b8) * vz;
    const double dist = sqrt(vx * vx + vy * vy + vz * vz);
    const double rp = static_cast<double>(c.w) * (1.0 + 1e-6);
    uint32_t hx = 0u, hy = 0u, rb = 0x7F800000u;  // rho^2 = +inf: always pass
    bool pass_all = !ok || !(dist > rp * 1.0001) || !(Z > 0.0) || !isfinite(dist) || !(c.w >= 0.0f);
    if (!pass_all) {
        const double az = Z / dist;
        const double beta = acos(fmin(1.0, az));
        const double th = asin(fmin(1.0, rp / dist));
        if (!(beta + th < 1.45)) {  // ~83 degrees: the bound's cos(beta + theta) too small
            pass_all = true;
        } else {
            const float qx = static_cast<float>(X / Z), qy = static_cast<float>(Y / Z);
            const double q = fabs(static_cast<double>(qx)) + fabs(static_cast<double>(qy));
            const double rho_g = sin(th) / (az * cos(beta + th));
            const double eps_c = 1.5 * (1.0 / 16384.0) * q;
            const double m = 1.0 + q + rho_g;
            const double rho = rho_g * (1.0 + 1e-5) + eps_c + 4e-6 * m * m;
            const float r2 = __double2float_ru(rho * rho * (1.0 + 1e-6));
            uint32_t bits = __float_as_uint(r2);
            if (bits & 0xFFFFu) bits = (bits & 0xFFFF0000u) + 0x10000u;  // bf16, rounded up
            if (isfinite(r2) && bits < 0x7F800000u) {
                rb = bits;
                hx = __float_as_uint(qx);
                hy = __float_as_uint(qy);
            } else {
                pass_all = true;
            }
        }
    }
    // low bytes: rho^2's bf16, high byte in x, low byte in y
    const uint32_t sx = (hx & ~0xFFu) | (rb >> 24), sy = (hy & ~0xFFu) | ((rb >> 16) & 0xFFu);
    out[i] = make_float2(__uint_as_float(sx), __uint_as_float(sy));
}

hipError_t launch_cam8_screen(const float4* prim_sp, uint32_t n, const float o[3], const float B[9],
                              uint32_t ok, float2* out, hipStream_t st) {
    if (n) {
        hipLaunchKernelGGL(cam8_screen_kernel, dim3((n + kBlockThreads - 1) / kBlockThreads),
                           dim3(kBlockThreads), 0, st, prim_sp, n, o[0], o[1], o[2], B[0], B[1], B[2],
                           B[3], B[4], B[5], B[6], B[7], B[8], ok, out);
    }
    return hipGetLastError();
}

// Albedo by leaf reference (SceneArgs::prim_al): out[i] = albedo[prim_idx[i]]
// for the n real reference slots (a packed layout's gaps name sphere 0).
__global__ void __launch_bounds__(kBlockThreads)
    albedo_refs_kernel(const uint32_t* __restrict__ prim_idx, const uint32_t* __restrict__ albedo,
                       uint32_t n, uint32_t n_spheres, uint32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t k = prim_idx[i];
    out[i] = k < n_spheres ? albedo[k] : 0u;
}

hipError_t launch_albedo_refs(const uint32_t* prim_idx, const uint32_t* albedo, uint32_t n,
                              uint32_t n_spheres, uint32_t* out, hipStream_t st) {
    if (n) {
        hipLaunchKernelGGL(albedo_refs_kernel, dim3((n + kBlockThreads - 1) / kBlockThreads),
                           dim3(kBlockThreads), 0, st, prim_idx, albedo, n, n_spheres, out);
    }
    return hipGetLastError();
}

__global__ void __launch_bounds__(kBlockThreads)
    unpack_kernel(const uint32_t* __restrict__ packed, const uint32_t* __restrict__ tiles,
                  uint32_t n_tiles, uint32_t ts, uint32_t tiles_x, uint32_t W, uint32_t H,
                  uint32_t* __restrict__ img) {
    const size_t i = (size_t)blockIdx.x * kBlockThreads + threadIdx.x;
    const size_t per = (size_t)ts * ts;
    if (i >= per * n_tiles) return;
    const uint32_t k = static_cast<uint32_t>(i / per);
    const uint32_t r = static_cast<uint32_t>(i % per);
    const uint32_t tile = tiles[k];
    if (tile == 0xFFFFFFFFu) return;  // RT_TILE_SKIP: a padding slot
    const uint32_t x = (tile % tiles_x) * ts + r % ts;
    const uint32_t y = (tile / tiles_x) * ts + r / ts;
    if (x < W && y < H) img[(size_t)y * W + x] = packed[i];
}

// ---------------------------------------------------------------------------
// launchers (called from rt_capi.cpp)
// ---------------------------------------------------------------------------

hipError_t launch_compat(const FrameArgs& a, hipStream_t st) {
    if (a.tiles) {
        const uint32_t strips = a.tile_size / 4u * (a.tile_size / 64u);
        hipLaunchKernelGGL(compat_tiles_kernel, dim3(a.n_tiles * strips), dim3(kBlockThreads), 0,
                           st, a);
    } else {
        hipLaunchKernelGGL(compat_kernel, dim3((a.W + 63) / 64, (a.H + 3) / 4), dim3(kBlockThreads),
                           0, st, a);
    }
    return hipGetLastError();
}

size_t scene_lds_bytes(const FrameArgs& a) {
    const size_t colours = kBlockThreads * sizeof(float4);  // pixel sums
    const uint32_t levels = stack_levels(a.sc);
    return colours + static_cast<size_t>(levels) * kBlockThreads * sizeof(uint2) + kLeafBufBytes;
}

// Resident workgroups on the device for a kernel at a given LDS size.  The
// occupancy query is a host call: cache it per (kernel, LDS bytes, device) so
// the launch path stays a single hipLaunchKernelGGL.
template <typename K>
static uint32_t resident_blocks(K kernel, size_t lds) {
    struct Key {
        const void* k;
        size_t lds;
        int dev;
    };
    static std::mutex mu;
    static std::vector<std::pair<Key, uint32_t>> cache;
    int dev = 0;
    (void)hipGetDevice(&dev);
    const void* kp = reinterpret_cast<const void*>(kernel);
    {
        std::lock_guard<std::mutex> g(mu);
        for (const auto& e : cache)
            if (e.first.k == kp && e.first.lds == lds && e.first.dev == dev) return e.second;
    }
    hipDeviceProp_t prop;
    int cus = 256;
    if (hipGetDeviceProperties(&prop, dev) == hipSuccess) cus = prop.multiProcessorCount;
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, kBlockThreads, lds) != hipSuccess ||
        per_cu <= 0)
        per_cu = 4;
    const uint32_t n = static_cast<uint32_t>(cus * per_cu);
    std::lock_guard<std::mutex> g(mu);
    cache.push_back({{kp, lds, dev}, n});
    return n;
}

static uint32_t cus_of_device() {
    static std::mutex mu;
    static std::vector<std::pair<int, uint32_t>> cache;
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> g(mu);
    for (const auto& e : cache)
        if (e.first == dev) return e.second;
    hipDeviceProp_t prop;
    const uint32_t n = hipGetDeviceProperties(&prop, dev) == hipSuccess ? prop.multiProcessorCount : 256;
    cache.push_back({dev, n});
    return n;
}

constexpr size_t kOneSppLds = (160u * 1024u / 3u) & ~size_t(15);  // 3 workgroups per CU

// Block tiles in the frame (or in the packed tile list) for block-tile side b.
static uint32_t count_block_tiles(const FrameArgs& a, uint32_t b) {
    if (a.tiles) return a.n_tiles * (a.tile_size / b) * (a.tile_size / b);
    return ((a.W + b - 1) / b) * ((a.H + b - 1) / b);
}

// Persistent launch: grid = resident workgroups; the block-tile side shrinks
// (16 -> 8 -> 4 pixels, never below two wave tiles) until the tile queue holds
// >= 8 tiles per resident workgroup, so the dynamic queue can even out costly
// image regions to the end (A/B, profiles/r01/bts_ab.log: 1080p 64 spp picks
// 8x8 tiles, -6.4% vs 16x16; a 1/4 or 1/8 multi-GPU share picks 4x4).
template <typename K>
static void launch_persistent(K kernel, const FrameArgs& a_in, uint32_t, size_t lds,
                              hipStream_t st) {
    FrameArgs a = a_in;
    // 1 spp: a wave's 64 lanes are 64 different pixels, whose walks thrash
    // the L1 when 5 workgroups share a CU; the dynamic LDS is padded so that
    // at most 3 are resident (C2: 0.358 -> 0.274 ms; 2 or 4 per CU slower,
    // 4 spp unchanged; profiles/r01/c2_wg_cap_ab.log)
    if (a.spw == 1u && !(a.sc.opt & kOptNoWgCap)) lds = std::max(lds, kOneSppLds);
    const uint32_t res = resident_blocks(kernel, lds);
    const uint32_t min_side = 2u * std::max(a.tw, a.th);
    a.bts = kTileSide;
    const uint32_t force = (a.sc.opt >> kOptBtsShift) & 7u;
    if (force && (kTileSide >> (force - 1u)) >= min_side)
        a.bts = kTileSide >> (force - 1u);
    else
        while (a.bts / 2u >= min_side && count_block_tiles(a, a.bts) < 8u * res) a.bts /= 2u;
    const uint32_t grid = std::min(count_block_tiles(a, a.bts), res);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlockThreads), lds, st, a);
}

// Per-wave queue launch: grid = resident workgroups, capped by the work.
template <typename K>
static void launch_waveq(K kernel, const FrameArgs& a, size_t lds, hipStream_t st,
                         uint32_t per_simd = 7) {
    const uint32_t res = resident_blocks(kernel, lds);
    uint64_t units;
    if (a.tiles)
        units = (uint64_t)a.n_tiles * (a.tile_size / a.tw) * (a.tile_size / a.th);
    else
        units = (uint64_t)((a.W + a.tw - 1) / a.tw) * ((a.H + a.th - 1) / a.th);
    // (the grid only sizes the launch; padding units of edge blocks are skipped)
    const uint64_t want = (units + kBlockThreads / 64 - 1) / (kBlockThreads / 64);
    // The occupancy query counts 8 workgroups per CU for the 7-wave builds
    // (60-65 VGPRs), but their 94 SGPRs leave room for 7: the 8th per CU
    // only starts when another exits, finds nothing and adds 8 queue atomics
    // to the tail (profiles/r02/timeline_hwid.log).  Capped at the build's
    // waves per SIMD: C3 -0.8%, 1/8 share -5% (profiles/r02/steal_ab.log,
    // measured with the static per-XCD ranges that preceded the two-level queue)
    const uint64_t cap = per_simd ? static_cast<uint64_t>(cus_of_device()) * per_simd : res;
    const uint32_t grid =
        static_cast<uint32_t>(std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(res, cap), want)));
    FrameArgs b = a;
    if (!((a.sc.opt >> kOptChunkShift) & 7u)) {
        // auto ticket size, second half: a small launch (a multi-GPU share)
        // has few units per wave, and big tickets lengthen its tail. N-way
        // C3 shares: 4 per ticket best at 1/2 and 1/4, 2 at 1/8 (36 units a
        // wave; profiles/r01/shard_chunk.log)
        const uint64_t per_wave = units / (static_cast<uint64_t>(grid) * (kBlockThreads / 64));
        const uint32_t cap = per_wave >= 64 ? 4u : per_wave >= 16 ? 2u : 1u;
        b.wq_chunk = std::min(b.wq_chunk, cap);
    }
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlockThreads), lds, st, b);
}

// Sorted rounds (above): a wave-queue frame of one pixel per wave and 2..4
// rounds, wherever the per-wave LDS still lets 8 workgroups share a CU.
// `on`: false under the test hook RT_SORT=0 (images and counters are the same).
size_t sort_lds_bytes(const FrameArgs& a) {
    return static_cast<size_t>(stack_levels(a.sc, true)) * kBlockThreads * sizeof(uint2) +
           (kBlockThreads / 64) * kSortWaveBytes + kLeafBufBytes;
}
static bool sorted_rounds(const FrameArgs& a, bool on) {
    return on && a.spp >= 8u && a.spw == 64u && a.rounds >= 2u && a.rounds <= kSortMaxRounds &&
           sort_lds_bytes(a) * 8u <= 160u * 1024u &&
           (a.accum != nullptr || a.variant == kVariantWaveQ);
}

// kOcc: the plain (counter-free) instances answer shadow rays from the
// scene's occluder lists; stats frames walk either way
template <bool kTiles, bool kOcc, bool kBin>
static void launch_scene_o(const FrameArgs& a, bool sort, uint32_t n_bt, size_t lds, hipStream_t st) {
    if (sorted_rounds(a, sort)) {
        const size_t sl = sort_lds_bytes(a);
        if (a.accum) {
            if (a.count_work)
                launch_waveq(scene_kernel<kTiles, 7, 2, true, true, true, true>, a, sl, st);
            else
                launch_waveq(scene_kernel_w8<kTiles, true, true, kOcc, kBin>, a, sl, st, 8);
        } else if (a.count_work) {
            launch_waveq(scene_kernel<kTiles, 7, 2, true, false, true, true>, a, sl, st);
        } else {
            launch_waveq(scene_kernel_w8<kTiles, false, true, kOcc, kBin>, a, sl, st, 8);
        }
        return;
    }
    if (a.accum) {  // progressive frames: the unified walk, whatever the variant
        if (a.spp >= 8u) {  // the wave queue, like variant 13
            if (a.count_work)
                launch_waveq(scene_kernel<kTiles, 7, 2, true, true, true>, a, lds, st);
            else
                launch_waveq(scene_kernel_w8<kTiles, true, false, kOcc, kBin>, a, lds, st, 8);
        } else if (a.count_work) {
            launch_persistent(scene_kernel<kTiles, 1, 2, true, true>, a, n_bt, lds, st);
        } else {
            launch_persistent(scene_kernel<kTiles, 1, 2, false, true, false, false, kOcc>, a, n_bt, lds, st);
        }
        return;
    }
    switch (a.variant) {
        case kVariantLaneUnified:  // block-tile queue, counting in every frame
            launch_persistent(scene_kernel<kTiles, 1, 2>, a, n_bt, lds, st);
            break;
        case kVariantLaneUnified2NoStats:  // the spp < 8 default: 7 with counters only in stats frames
            if (a.count_work)
                launch_persistent(scene_kernel<kTiles, 1, 2, true>, a, n_bt, lds, st);
            else
                launch_persistent(scene_kernel<kTiles, 1, 2, false, false, false, false, kOcc>, a, n_bt, lds, st);
            break;
        case kVariantWaveQLow:  // the spp < 8 default (round 4): the per-wave queue, 8 waves/SIMD
            // No workgroup barrier per block tile: the timeline of the block-tile
            // queue (variant 10) showed waves idle 28% of the C2 launch, mostly
            // waiting at that barrier for the slowest of a tile's 4 wave tiles
            // (gaps p90 5.2 us against units of p50 5.8 us,
            // profiles/r04/c2_timeline.log).  With it C2 0.155 -> 0.107 ms; the
            // 3-workgroups-per-CU cap of the block-tile queue costs it again
            // here (0.152 ms), so it has none (profiles/r04/c2_waveq_ab.log).
            if (a.count_work)
                launch_waveq(scene_kernel<kTiles, 7, 2, true, false, true>, a, lds, st);
            else
                launch_waveq(scene_kernel_w8<kTiles, false, false, kOcc, kBin>, a, lds, st, 8);
            break;
        case kVariantWaveQ:  // the spp >= 8 default: per-wave scheduling over per-XCD queues.
            // Timed (plain) frames: 8 waves/SIMD with SGPRs capped at 80
            // (kSceneSgprs); stats frames keep 7 (their counters need the
            // registers; C3 -2.8%, C5 -5.4% against 6, profiles/r01/occupancy_ab.log)
            if (a.count_work)
                launch_waveq(scene_kernel<kTiles, 7, 2, true, false, true>, a, lds, st);
            else
                launch_waveq(scene_kernel_w8<kTiles, false, false, kOcc, kBin>, a, lds, st, 8);
            break;
        default:  // rejected by variant_available() before any launch
            break;
    }
}

// Variants compiled into this build (rt_create refuses the others).  The
// measured-and-rejected alternatives of DESIGN.md 5.1 (packets, LDS / scalar /
// one-lane uniform leaves, bundle prefilter, 6- and 8-wave builds) were
// removed in round 3; their A/B logs stay under profiles/.
template <bool kTiles>
static void launch_scene_t(const FrameArgs& a, bool sort, uint32_t n_bt, size_t lds, hipStream_t st) {
    // (bins: set only for a frame whose instance reads them, frame_reads_bins)
    const bool bin = a.bin_hdr && a.bin_ent && a.bin_info && !a.count_work;
    const bool occ = a.sc.prim_occ && a.sc.occ_sp && a.shadows && !a.count_work;
    if (occ && bin)
        launch_scene_o<kTiles, true, true>(a, sort, n_bt, lds, st);
    else if (occ)
        launch_scene_o<kTiles, true, false>(a, sort, n_bt, lds, st);
    else if (bin)
        launch_scene_o<kTiles, false, true>(a, sort, n_bt, lds, st);
    else
        launch_scene_o<kTiles, false, false>(a, sort, n_bt, lds, st);
}

// Whether launch_scene runs this plain frame on a scene_kernel_w8 instance
// (the ones that read bins): launch_scene_o's choices, restated.
bool frame_reads_bins(const FrameArgs& a_in, bool sort) {
    FrameArgs a = a_in;
    if (a.count_work) return false;
    if (a.accum) a.variant = kVariantLaneUnified;
    wave_tile_shape(a.spp, a.spw, a.g, a.ppw, a.tw, a.th);
    a.rounds = (a.spp + a.spw - 1) / a.spw;
    if (sorted_rounds(a, sort)) return true;
    if (a.accum) return a.spp >= 8u;
    return a.variant == kVariantWaveQ || a.variant == kVariantWaveQLow;
}

bool variant_available(uint32_t v) {
    return v == 0 || v == kVariantLaneUnified || v == kVariantLaneUnified2NoStats ||
           v == kVariantWaveQ || v == kVariantWaveQLow;
}

// sort: sorted rounds where they apply (the renderer's; off only under a test hook)
hipError_t launch_scene(const FrameArgs& a_in, bool sort, hipStream_t st) {
    FrameArgs a = a_in;
    if (a.accum) a.variant = kVariantLaneUnified;  // what launch_scene_t runs (LDS sizing)
    // wave mapping: spw samples x ppw pixels per wave (see scene_kernel)
    wave_tile_shape(a.spp, a.spw, a.g, a.ppw, a.tw, a.th);
    a.rounds = (a.spp + a.spw - 1) / a.spw;
    // wave-queue ticket size: adjacent wave tiles back to back on one wave
    // reuse its CU's L1; a ticket of about four rounds of work balances that
    // against the queue tail (C3, 1 round: 4 per ticket -4.1%; C5, 4 rounds:
    // 1 per ticket, more is slower; profiles/r01/chunk_ab.log)
    const uint32_t ck = (a.sc.opt >> kOptChunkShift) & 7u;
    a.wq_chunk = ck ? 1u << (ck - 1u) : std::max(1u, 4u / std::max(1u, std::min(a.rounds, 4u)));
    const size_t lds = scene_lds_bytes(a);
    if (a.tiles)
        launch_scene_t<true>(a, sort, 0, lds, st);
    else
        launch_scene_t<false>(a, sort, 0, lds, st);
    return hipGetLastError();
}

hipError_t launch_unpack(const uint32_t* packed, const uint32_t* tiles, uint32_t n_tiles,
                         uint32_t ts, uint32_t tiles_x, uint32_t W, uint32_t H, uint32_t* img,
                         hipStream_t st) {
    const size_t total = (size_t)ts * ts * n_tiles;
    const uint32_t blocks = static_cast<uint32_t>((total + kBlockThreads - 1) / kBlockThreads);
    if (blocks) {
        hipLaunchKernelGGL(unpack_kernel, dim3(blocks), dim3(kBlockThreads), 0, st, packed, tiles,
                           n_tiles, ts, tiles_x, W, H, img);
    }
    return hipGetLastError();
}

}  // namespace rtamd
