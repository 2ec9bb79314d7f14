// rt_walk.h — the per-lane octree walk and its helpers, shared by the frame
// kernels (rt_kernels.hip) and the ray-query kernels (rt_query.hip,
// rt_multihit.hip, rt_gbuffer.hip).  Device
// code only; included inside a HIP translation unit.
#pragma once
#include <hip/hip_runtime.h>

#include "rt_params.h"

namespace rtamd {

#ifdef RT_BLOCK_STATS
// Diagnostic build: the first active lane counts one execution of block i by
// the wave, and the active lanes (BlockStat, rt_params.h).
__device__ __forceinline__ void bs_count(uint32_t* bs, uint32_t i) {
    const uint64_t m = __ballot(1);
    if (__lane_id() == static_cast<uint32_t>(__builtin_ctzll(m))) {
        bs[2 * i] += 1u;
        bs[2 * i + 1] += static_cast<uint32_t>(__popcll(m));
    }
}
#define RT_BS(i) bs_count(bs, (i))
#else
#define RT_BS(i) ((void)0)
#endif

// Nearest root with the perpendicular-distance discriminant, explicit FMAs
// (13 VALU to the h < 0 test); accepted iff tmin < t < tmax.  Same operations
// as oracle.c:isect.  isect_oc takes o - c already formed (in the same f32
// operations: the camera-relative records hold it), isect forms it.
__device__ __forceinline__ bool isect_oc(float ocx, float ocy, float ocz, float d0, float d1,
                                         float d2, float r, float tmin, float tmax, float& tout,
                                         uint32_t* bs = nullptr) {
    const float b = fmaf(ocz, d2, fmaf(ocy, d1, ocx * d0));
    const float qx = fmaf(-b, d0, ocx);
    const float qy = fmaf(-b, d1, ocy);
    const float qz = fmaf(-b, d2, ocz);
    const float qq = fmaf(qz, qz, fmaf(qy, qy, qx * qx));
    const float h = fmaf(r, r, -qq);
    if (h < 0.0f) return false;
    RT_BS(kBsSqrt);
    const float sq = sqrtf(h);
    float t = -b - sq;
    if (!(t > tmin)) t = -b + sq;
    if (!(t > tmin) || !(t < tmax)) return false;
    tout = t;
    return true;
}
__device__ __forceinline__ bool isect(float o0, float o1, float o2, float d0, float d1, float d2,
                                      float4 sp, float tmin, float tmax, float& tout,
                                      uint32_t* bs = nullptr) {
    const float ocx = o0 - sp.x;
    const float ocy = o1 - sp.y;
    const float ocz = o2 - sp.z;
    return isect_oc(ocx, ocy, ocz, d0, d1, d2, sp.w, tmin, tmax, tout, bs);
}

// v_readlane of a float's bits (the builtin is int-typed: a float argument
// would be converted to an integer value)
__device__ __forceinline__ float readlane_f(float x, uint32_t lane) {
    return __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(x), lane));
}

// isect's discriminant h alone (same operations): h < 0 <=> isect rejects
// the sphere before its square root.
__device__ __forceinline__ float isect_h_oc(float ocx, float ocy, float ocz, float d0, float d1,
                                            float d2, float r) {
    const float b = fmaf(ocz, d2, fmaf(ocy, d1, ocx * d0));
    const float qx = fmaf(-b, d0, ocx);
    const float qy = fmaf(-b, d1, ocy);
    const float qz = fmaf(-b, d2, ocz);
    const float qq = fmaf(qz, qz, fmaf(qy, qy, qx * qx));
    return fmaf(r, r, -qq);
}
__device__ __forceinline__ float isect_h(float o0, float o1, float o2, float d0, float d1,
                                         float d2, float4 sp) {
    const float ocx = o0 - sp.x;
    const float ocy = o1 - sp.y;
    const float ocz = o2 - sp.z;
    return isect_h_oc(ocx, ocy, ocz, d0, d1, d2, sp.w);
}

// The kernel's FrameArgs as memory (the kernarg segment, scalar-cached),
// behind an opaque pointer: a field read through it is a fresh s_load at that
// point instead of a value kept live in an SGPR across the walk (the register
// allocator would spill it into VGPR lanes: v_writelane / v_readlane, VALU
// work per pixel).  Used for the per-sample camera, shading and output fields.
typedef __attribute__((address_space(4))) const FrameArgs KernArgs;
__device__ __forceinline__ KernArgs* kernargs() {
    KernArgs* p = (KernArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return p;
}

// An incomplete frame (FrameArgs::qerr): this frame's id into the renderer's
// pinned host word, a plain system-scope store (no atomic over the host
// link), visible to the host without a copy.  Called by a wave's lead lane.
__device__ __forceinline__ void frame_failed() {
    KernArgs* ka = kernargs();
    __hip_atomic_store(ka->qerr, ka->frame_id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// rank of this lane among the lanes set in m
__device__ __forceinline__ uint32_t lane_rank(uint64_t m) {
    return __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(m >> 32),
                                     __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(m), 0u));
}

// LDS leaf staging: a per-wave buffer of kLeafBuf spheres
// after the rest of the workgroup's LDS (pixel sums and stacks, or the sorted
// path's stacks and per-wave regions).  Used by the nearest walks that screen
// 16-byte camera-relative records: the block-tile queue (variants 7 and 10)
// and progressive frames below 8 spp.
// Leaves of fewer spheres read them directly: staging adds an LDS round trip
// to the first chunk, which a leaf of one or two chunks does not win back.
// Measured (profiles/r05/ldsmin_ab.log, 3 alternating rounds, against no
// staging): from 1 / 4 / 6 / 8 spheres C3 +1.0 / -0.7 / -1.7 / +0.2%, C5
// -6.9 / -7.8 / -7.8 / -5.3%, C5d +4.0 / +2.5 / +2.3 / +2.5%.  Round 6, with
// shadow walks no longer staging, against 6: from 2 / 3 / 4 / 5 spheres C3
// +0.2 / -0.4 / -0.5 / -1.0%, C5 -0.8 / -1.1 / -1.2 / -1.3%, C5d +1.0 / +0.5
// / +0.3 / +0.1%, 8: C3 +3.5%, C5 +4.6%
// (profiles/r06/ab_r6_lmin2_lmin3_lmin4_lmin5.log, ab_r6_lmin4_lmin8.log).
constexpr uint32_t kLdsLeafMin = 5;

// Ancestor-stack levels per thread (rt_sched.h) of a scene
__host__ __device__ inline uint32_t stack_levels(const SceneArgs& S, bool no_stack = false) {
    return stack_levels(S.tab_k, S.stack_depth, no_stack);
}

// First float4 of this wave's LDS leaf buffer: FrameLds::leaf_buf / 16
// (rt_sched.h, the layout's one statement) plus the wave's part, written in
// float4 units here because computed from FrameLds' byte offsets the kernels
// get other scalar instructions than the ones measured (profiles/r13).
__device__ __forceinline__ uint32_t leaf_buf_base(const SceneArgs& S, bool sorted) {
    const uint32_t wave = threadIdx.x >> 6;
    const uint32_t head = sorted ? (stack_levels(S, true) * kBlockThreads * 8u +
                                    (kBlockThreads / 64u) * kSortWaveBytes) / 16u
                                 : kBlockThreads + stack_levels(S) * kBlockThreads / 2u;
    return head + wave * kLeafBuf;
}

// One lane's K nearest hits of a multi-hit walk (rt_multihit.hip, DESIGN.md
// 5.9): {t, leaf reference}, sorted by (t, then the caller's sphere index), a
// free slot {the ray's tmax, kNoHit} (isect accepts t < tmax only, so a free
// slot sorts after every hit and t[K - 1] is the walk's bound either way).
// Every index below is a compile-time constant once the loops are unrolled:
// the arrays are registers, never scratch.
template <int K>
struct MultiHits {
    float t[K > 0 ? K : 1];
    uint32_t ref[K > 0 ? K : 1];
    __device__ __forceinline__ void clear(float tmax) {
#pragma unroll
        for (int i = 0; i < K; ++i) {
            t[i] = tmax;
            ref[i] = kNoHit;
        }
    }
    // An accepted sphere.  It enters iff it sorts before the K-th entry and is
    // not held already.  A sphere met again in a later leaf has the same t
    // bits, so the sphere indices are loaded only when an entry's t equals th
    // exactly (the nearest walk's tie load); a sphere evicted earlier sorts
    // after the K-th entry and is rejected by the same comparison.
    __device__ __forceinline__ void offer(const uint32_t* __restrict__ prim_idx, float th, uint32_t r) {
        if (!(th <= t[K - 1])) return;
        uint32_t pos = 0;  // entries that sort before the candidate
        bool tie = false;
#pragma unroll
        for (int i = 0; i < K; ++i) {
            pos += t[i] < th ? 1u : 0u;
            tie |= t[i] == th;
        }
        bool held = false;
        if (tie) {
            // (an entry whose t equals th is a hit, never a free slot: th <
            // tmax, so ref[i] below is a leaf reference)
            const uint32_t ci = prim_idx[r];
#pragma unroll
            for (int i = 0; i < K; ++i)
                if (t[i] == th) {
                    const uint32_t ei = prim_idx[ref[i]];
                    held |= ei == ci;
                    pos += ei < ci ? 1u : 0u;
                }
        }
        if (held || pos >= static_cast<uint32_t>(K)) return;
#pragma unroll
        for (int i = K - 1; i >= 0; --i) {
            const bool below = static_cast<uint32_t>(i) > pos;  // shifts down one slot
            const bool here = static_cast<uint32_t>(i) == pos;
            const int up = i > 0 ? i - 1 : 0;  // (slot 0 never shifts: pos >= 0)
            t[i] = here ? th : below ? t[up] : t[i];
            ref[i] = here ? r : below ? ref[up] : ref[i];
        }
    }
};

// Grid-space octree walk (DESIGN.md "Octree walk"): mirrored origin so every
// direction component is >= 0 (the Revelles entry step of hit_sphere,
// src/renderer.cu:23-43), cell planes at integer grid coordinates, descend by
// mid-plane tests at the current t, leave a cell through its exit planes, and
// pop to the common ancestor found from the highest flipped coordinate bit.
// The per-thread ancestor stack lives in LDS, [depth-1][thread] (conflict-free).
// kAnyHit: compile-time any-hit; with kDynAny the mode comes from `any_rt`
// instead, so ONE inlined walk serves both the primary and the shadow ray.
// kShadowL: this walk's any-hit rays are the frame's shadow rays, whose
// direction is FrameArgs::L in every lane: only then may it use
// the light-plane screen and keep its reciprocals wave-uniform.  Any other
// any-hit walk (a per-lane direction: ambient occlusion, area lights) keeps
// the full discriminant screen.
// kGeneric: a caller's ray (rt_query.hip), any origin and direction per lane,
// in a kernel that renders no frame: no camera-relative or image-plane screen
// (the origin is not the camera), no light-plane screen, no LDS leaf staging
// (the lanes are incoherent), and NO read through kernargs(): every such read
// below sits behind a condition that is false at compile time in this mode.
// Both kinds return the hit's leaf REFERENCE in `iout` (an any-hit walk of a
// frame sets `tout` only); the caller maps it through prim_idx, or shades by
// reference (prim_sp[ref], SceneArgs::prim_al[ref]: against the sphere index
// and the by-index arrays C3 -0.7%, C5 -0.5%, L2 misses C3 -7.5%, C5d -11.5%,
// profiles/r06/ab_ref_shade.log).
// lb_u: the wave's LDS leaf buffer (scene_body's leaf_buf_base), read only by
// a walk that stages leaves: a frame's nearest walk without kCam8.  The other
// walks pass none.
// kMulti > 0: a multi-hit walk (rt_multihit.hip), a generic
// nearest walk that keeps the kMulti smallest (t, sphere index) in *mh (which
// the caller cleared to the ray's tmax) instead of one best hit: every
// accepted sphere is offered to mh, and mh's last t takes best_t's place in
// the stop rule.  isect keeps the ray's own tmax, so a sphere tied with the
// last entry at a lower index is still seen.  Returns whether mh holds a hit;
// tout and iout are left alone.
//
// Leaf spheres are read kLeafChunk = 2 at a time, in every walk: one dwordx4
// of 8-byte screen records a chunk.  (4 a chunk in the shadow walks: 4 spills
// of 48-100 B, C3 +6%, C5 +8%, C5d +5%, profiles/r06/ab_shd_chunk4.log.)
constexpr int kLeafChunk = 2;

// The switches of a walk, by name; the kinds of walk that exist follow.
struct WalkKind {
    static constexpr bool any_hit = false;   // kAnyHitT: compile-time any-hit
    static constexpr bool dyn_any = false;   // kDynAny: any-hit or nearest by `any_rt`
    static constexpr bool stats = false;     // counts node visits and sphere tests
    static constexpr bool no_stack = false;  // kNoStack: no ancestor stack where there is a table
    static constexpr bool shadow_l = false;  // kShadowL: any-hit rays along the frame's L
    static constexpr bool cam8 = false;      // kCam8: 8-byte image-plane screen, no staging
    static constexpr bool generic = false;   // kGeneric: a caller's ray, no frame
    static constexpr int multi = 0;          // kMulti: keeps the k nearest hits
};
// a frame's primary walk (staged 16-byte screen, or kCam8: the image-plane
// screen) and its shadow walk along L
template <bool kStats, bool kCam8>
struct FramePrimary : WalkKind { static constexpr bool stats = kStats, cam8 = kCam8; };
template <bool kStats>
struct FrameShadow : WalkKind { static constexpr bool any_hit = true, stats = kStats, shadow_l = true; };
// the sorted path's primary and shadow walks: stackless, any-hit or nearest
// at run time (kDynAny), as measured
template <bool kStats>
struct SortedPrimary : WalkKind { static constexpr bool dyn_any = true, stats = kStats, no_stack = true, cam8 = true; };
template <bool kStats>
struct SortedShadow : WalkKind { static constexpr bool dyn_any = true, stats = kStats, no_stack = true, shadow_l = true; };
// the occluder lists' fallback: a shadow walk of a plain frame
template <bool kNoStack>
struct OccFallback : WalkKind { static constexpr bool any_hit = true, no_stack = kNoStack, shadow_l = true; };
// a caller's ray, any-hit or nearest (rt_query.hip, rt_gbuffer.hip), or
// keeping its K nearest hits (rt_multihit.hip)
template <bool kAny, bool kStats>
struct GenericRay : WalkKind { static constexpr bool any_hit = kAny, stats = kStats, generic = true; };
template <int K, bool kStats>
struct MultiHitRay : GenericRay<false, kStats> { static constexpr int multi = K; };

template <class Kind>
__device__ __forceinline__ bool walk(const SceneArgs& S, float o0, float o1, float o2, float d0,
                                     float d1, float d2, float tmin, float tmax, float& tout,
                                     uint32_t& iout, uint32_t& n_nodes, uint32_t& n_prims,
                                     uint2* __restrict__ stk, bool any_rt = false,
                                     uint32_t* bs = nullptr, uint32_t lb_u = ~0u,
                                     MultiHits<Kind::multi>* mh = nullptr) {
    constexpr bool kAnyHitT = Kind::any_hit, kDynAny = Kind::dyn_any, kStats = Kind::stats,
                   kNoStack = Kind::no_stack, kShadowL = Kind::shadow_l, kCam8 = Kind::cam8,
                   kGeneric = Kind::generic;
    constexpr int kChunk = kLeafChunk, kMulti = Kind::multi;
    static_assert(!kShadowL || kAnyHitT || kDynAny, "a shadow walk along L is an any-hit walk");
    static_assert(!kGeneric || (!kShadowL && !kCam8), "a generic ray has no frame to screen against");
    static_assert(kMulti == 0 || (kGeneric && !kAnyHitT && !kDynAny),
                  "a multi-hit walk is a generic nearest walk");
    const bool kAnyHit = kDynAny ? any_rt : kAnyHitT;
    const uint32_t D = S.max_depth;
    const uint32_t G = 1u << D;
    // Camera-relative screen: a nearest-hit walk is a primary
    // ray, whose origin is the frame's camera origin, so its screen reads the
    // per-frame records {o - c, C'} and tests fma(b, b, -C') >= 0 (4 VALU a
    // sphere) instead of the full discriminant (13 VALU); the exact tests of a
    // chunk that passes load the chunk's own sphere records (through a fresh
    // kernel-argument read: no second array pointer lives in the walk).
    // Shadow (any-hit) walks start at hit points and keep the full screen.
    // (Exact records {o - c, r} instead, the discriminant from the stored
    // o - c with no slack and no reload, gained less: C3 -1.7% against -2.9%,
    // profiles/r05/screen_ab.log.)
    const bool cam = !kGeneric && !kAnyHit;
    // Image-plane screen in 8 bytes (kCam8; SceneArgs::prim_cam8, DESIGN.md
    // 5.1 round 6): the wave-queue walks, sorted and not, screen a chunk's two
    // spheres from ONE dwordx4 instead of two 16-byte camera-relative records
    // and stage no leaves in LDS: C3 -2.9%, C5 -2.4%, C5d -2.1%, C2 -1.9%
    // (profiles/r06/ab_cam8_sorted.log).  The lane's point s = (Bd).xy /
    // (Bd).z, once per walk
    const bool cam8 = kCam8 && cam;
    float s8x = 0.0f, s8y = 0.0f;
    if (cam8) {
        KernArgs* kb = kernargs();
        const float px = fmaf(kb->cam8_B[2], d2, fmaf(kb->cam8_B[1], d1, kb->cam8_B[0] * d0));
        const float py = fmaf(kb->cam8_B[5], d2, fmaf(kb->cam8_B[4], d1, kb->cam8_B[3] * d0));
        const float pz = fmaf(kb->cam8_B[8], d2, fmaf(kb->cam8_B[7], d1, kb->cam8_B[6] * d0));
        const float iz = __builtin_amdgcn_rcpf(pz);
        s8x = px * iz;
        s8y = py * iz;
    }
    // Light-plane screen: a shadow walk's direction is the
    // frame's L in every lane, so a sphere is near the ray iff its centre is
    // near the ray's origin in the plane perpendicular to L.  The records
    // hold each centre's {u, v} there and a radius grown by the rounding
    // bound, the lane its origin's {up, vp}: 5 VALU a sphere instead of 13.
    // The records are 8 bytes (SceneArgs::prim_shd8), a chunk's two spheres
    // in ONE dwordx4 (the texture path charges a load by instruction, not by
    // bytes), screened against the scene's largest radius term shd_rr: C3
    // -2.0%, C5 -2.4%, C2 -2.8%, C5d -0.1% against 16-byte records with each
    // sphere's own (profiles/r06/ab_shd8.log).  Each sphere's own as bf16 in
    // the records' low bytes: C3 +0.5%, C5 +0.3%, C5d +0.1%
    // (profiles/r06/ab_shd8_per_sphere.log).
    const bool shd = kShadowL && kAnyHit;  // a shadow ray along L (the caller says so)
    float up = 0.0f, vp = 0.0f;
    const float2* __restrict__ shd8_base = shd ? S.prim_shd8 : nullptr;
    const float2* __restrict__ cam8_base = cam8 ? kernargs()->sc.prim_cam8 : nullptr;
    const float shd_rr = shd ? kernargs()->shd_rr : 0.0f;
    if (shd) {
        KernArgs* ke = kernargs();
        up = fmaf(o2, ke->shd_e[2], fmaf(o1, ke->shd_e[1], o0 * ke->shd_e[0]));
        vp = fmaf(o2, ke->shd_e[5], fmaf(o1, ke->shd_e[4], o0 * ke->shd_e[3]));
    }
    const float4* __restrict__ prim_sp = cam ? S.prim_cam : S.prim_sp;
    const uint2* __restrict__ nodes = S.nodes;
    const float o[3] = {o0, o1, o2};
    const float d[3] = {d0, d1, d2};
    float inv[3], nog[3];
    // Mirror mask packed in the cell table's index layout: field i (K bits,
    // 1 without a table) is all ones iff axis i is mirrored, so a table
    // index is the packed l >> (D - K) XOR mt (top - c == c ^ top for c <=
    // top), and the descent's child mirror bits are each field's low bit.
    const uint32_t kf = S.tab_k ? S.tab_k : 1u;
    const uint32_t ftop = (1u << kf) - 1u;
    uint32_t mt = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float g = (o[i] - S.rmin[i]) * S.scale[i];
        const bool neg = d[i] < 0.0f;
        float a = fabsf(d[i]);
        if (a < 1e-20f) a = 1e-20f;
        const float og = neg ? S.G - g : g;
        inv[i] = 1.0f / (a * S.scale[i]);
        // a shadow walk's direction is the frame's light direction, the same
        // in every lane (sample_color_unified): its reciprocals live in SGPRs
        if (kShadowL && kAnyHitT && !kDynAny)
            inv[i] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(
                                                   __builtin_bit_cast(uint32_t, inv[i])));
        nog[i] = -(og * inv[i]);
        mt |= neg ? ftop << (i * kf) : 0u;
    }
    // t of the grid plane at (mirrored) integer k: one FMA (oracle.c:plane)
    auto plane = [&](int i, uint32_t k) { return fmaf(static_cast<float>(k), inv[i], nog[i]); };
    float t0 = plane(0, 0), t1 = plane(0, G);
#pragma unroll
    for (int i = 1; i < 3; ++i) {
        const float a0 = plane(i, 0), a1 = plane(i, G);
        if (a0 > t0) t0 = a0;
        if (a1 < t1) t1 = a1;
    }
    if (t0 < tmin) t0 = tmin;
    if (t1 > tmax) t1 = tmax;
    if (!(t0 < t1)) return false;
    RT_BS(kBsWalk);

    float best_t = tmax;
    if (kStats) n_nodes += 1;

    // Nearest keeps the best leaf *reference*; the sphere index is loaded only
    // for an exact t tie (rare) and once at the end, so no dependent load sits
    // in the hot loop.  Same result as the oracle's (min t, then min index).
    uint32_t best_ref = kNoHit;
    auto test = [&](const float4& sp, uint32_t ref) -> bool {
        if (kStats) n_prims += 1;
        RT_BS(kBsTest);
        if (kAnyHit) RT_BS(kBsTestShadow);
        float th;
        if (isect(o0, o1, o2, d0, d1, d2, sp, tmin, tmax, th, bs)) {
            RT_BS(kBsAccept);
            if (kAnyHit) {
                tout = th;
                if (kGeneric) iout = ref;
                return true;
            }
            if constexpr (kMulti > 0) {
                mh->offer(S.prim_idx, th, ref);
                return false;
            }
            if (th < best_t) {
                best_t = th;
                best_ref = ref;
            } else if (th == best_t) {
                RT_BS(kBsTieLoad);
                if (S.prim_idx[ref] < S.prim_idx[best_ref]) best_ref = ref;
            }
        }
        return false;
    };
    // Leaf spheres in list order (same order, hence same counters, as the
    // oracle): each lane loads its own, kChunk loads in flight.
    // The chunk loop over one leaf's spheres (offset off, count cnt), each
    // read as load(k), k counted from the leaf's first reference.
    auto chunks = [&](auto&& load, uint32_t off, uint32_t cnt) -> bool {
        // cnt >= 1 (a leaf is a non-empty cell; the root leaf is guarded by
        // its caller): a do-while skips the loop-entry test and its branch
        uint32_t j = 0;
        // Slot q of a chunk holds one of the leaf's spheres iff j + q < cnt.
        // Slot 0 always does (j < cnt inside the do-while), and for q >= 1
        // the test is j < cnt - q against a per-leaf bound: no per-chunk
        // m = cnt - j, no second loop counter and no mask for slot 0.
        const auto in_leaf = [&](int q) -> bool {
            return q == 0 || static_cast<int>(j) < static_cast<int>(cnt) - q;
        };
        do {
            RT_BS(kBsLeafChunk);
            if (kAnyHit) RT_BS(kBsChunkShadow);
            // kChunk unconditional dwordx4 loads in flight at fixed offsets; a
            // slot past the leaf's end reads the next leaf or the array's
            // kPrimPad tail (in bounds) and is never tested
            // (fetching slot q >= 1 only when some lane's leaf still holds
            // it, a wave-uniform branch: C3 +8.0%, C5 +7.3%, C5d +7.5%,
            // profiles/r05/lds_pastend_ab.log)
            float4 sv[kChunk];
            if (shd || cam8) {
                // two slots' 8-byte records per dwordx4 (8-byte aligned:
                // global loads need dword alignment only).  Staged in LDS
                // instead, pairs per float4, from 8 / 5 / 3 spheres: C3 +1.2 /
                // +1.3 / +3.4% (profiles/r06/ab_cam8_staging.log)
                static_assert(!(kCam8 || kShadowL) || kChunk % 2 == 0, "two 8-byte records per load");
#pragma unroll
                for (int h = 0; h < kChunk / 2; ++h) {
                    const float4 pr = *reinterpret_cast<const float4*>((cam8 ? cam8_base : shd8_base) +
                                                                       (off + j + 2u * h));
                    sv[2 * h] = make_float4(pr.x, pr.y, 0.0f, 0.0f);
                    sv[2 * h + 1] = make_float4(pr.z, pr.w, 0.0f, 0.0f);
                }
            } else
#pragma unroll
            for (int q = 0; q < kChunk; ++q) {
                sv[q] = load(j + q);
                // issue in list order, so the first test waits for its own
                // sphere only (vmcnt(kChunk-1)), not for the whole chunk
                __builtin_amdgcn_sched_barrier(0);
            }
            // Uniform screen: every lane's discriminants first, with no branch;
            // only when some lane's h is >= 0 (or NaN) does the wave run the
            // exact per-lane tests (which recompute them), one branch for the
            // chunk instead of a divergent branch per test.  h < 0 is exactly
            // where isect returns false, so the same spheres are accepted.
            bool maybe = false;
#pragma unroll
            for (int q = 0; q < kChunk; ++q) {
                // unconditional and unmasked: a slot past the leaf's end holds
                // a real sphere record too, and if it passes the screen the
                // exact tests below still skip it (in_leaf), so it can only
                // send the chunk down the exact path for nothing
                bool pos;
                if (cam8) {
                    // the lane's image-plane distance from the centre's
                    // projection against rho^2 (bf16 in the records' low bytes)
                    const float rho2 = __uint_as_float(__builtin_amdgcn_perm(
                        __float_as_uint(sv[q].x), __float_as_uint(sv[q].y), 0x04000C0Cu));
                    const float dx = s8x - sv[q].x, dy = s8y - sv[q].y;
                    pos = !(fmaf(dy, dy, dx * dx) > rho2);
                } else if (cam) {
                    // b exactly as isect computes it ({x,y,z} = o - c in the
                    // same f32 operations); C' undercuts |o-c|^2 - r^2 by the
                    // rounding bound, so every sphere isect accepts passes
                    const float b = fmaf(sv[q].z, d2, fmaf(sv[q].y, d1, sv[q].x * d0));
                    pos = !(fmaf(b, b, -sv[q].w) < 0.0f);
                } else if (shd) {
                    // the centre's light-plane distance from the origin; rr'
                    // covers the rounding, so every sphere isect accepts passes
                    const float du = up - sv[q].x, dv = vp - sv[q].y;
                    pos = !(fmaf(dv, dv, du * du) > shd_rr);
                } else {
                    pos = !(isect_h(o0, o1, o2, d0, d1, d2, sv[q]) < 0.0f);
                }
                maybe |= pos;
            }
            // marked unlikely (it is: most chunks pass no lane): the exact
            // tests are laid out off the fall-through path (C3 -0.6%, C5
            // -0.7%, profiles/r02/branch_hint_ab.log)
#ifdef RT_BLOCK_STATS
            if (j + 1u >= cnt) RT_BS(kBsPastEnd);
#endif
            if (__builtin_expect(__any(maybe), 0)) {
                if (cam || shd) {  // the exact tests need the spheres themselves (cam8 too)
                    RT_BS(kBsExactLoad);
                    const float4* __restrict__ ex = kernargs()->sc.prim_sp + off;
#pragma unroll
                    for (int q = 0; q < kChunk; ++q) sv[q] = ex[j + q];
                }
#pragma unroll
                for (int q = 0; q < kChunk; ++q)
                    if (in_leaf(q) && test(sv[q], off + j + q)) return true;
            } else if (kStats) {
                n_prims += min(cnt - j, static_cast<uint32_t>(kChunk));
            }
            j += kChunk;
        } while (j < cnt);
        return false;
    };
    auto leaf = [&](uint32_t off, uint32_t cnt) -> bool {
        static_assert(kChunk <= kPrimPad + 1, "leaf loads may run kChunk-1 spheres past a leaf");
        RT_BS(kBsLeaf);
        // A leaf the whole wave is at (the common case: one pixel's samples
        // walk together): its spheres cross the texture path ONCE, each
        // active lane fetching one into the wave's LDS leaf buffer, and the
        // chunks read them back by LDS broadcast (every lane the same
        // address): one dwordx4 texture instruction per leaf visit instead
        // of two per chunk (DESIGN.md 5.1 "LDS leaf staging").  The buffer
        // is a typed LDS array, never a generic pointer (round 3's flat
        // loads).  A slot past the leaf's end holds a stale sphere, which
        // the exact tests skip as before.
        // Only nearest-hit walks stage: a shadow ray may stop at a leaf's
        // first chunk, after a staging load fetched all of the leaf's lines.
        // Against staging shadow leaves too: C5d -1.3%, C5 -0.5%, C3 -0.1%
        // (profiles/r06/ab_ctr3_noshst_sbo.log).
        // The fill goes through registers (a ds_write per record).  gfx950's
        // direct global -> LDS load instead, one global_load_lds_dwordx4 for a
        // run of active lanes: C3 +0.9%, C5 +1.3%, C5d +0.1%
        // (profiles/r06/ab_ctr2_glds_pack.log); its first build faulted a GPU
        // (a sign-extended address half, pack_ab_glds_fault.log).
        const uint32_t off_u = __builtin_amdgcn_readfirstlane(off);
        const uint32_t cnt_u = __builtin_amdgcn_readfirstlane(cnt);
        if (!kGeneric && !kAnyHit && !cam8 && cnt_u >= kLdsLeafMin && cnt_u < kernargs()->sc.lds_max &&
            __all(off == off_u)) {
            RT_BS(kBsLdsLeaf);
            extern __shared__ __attribute__((aligned(16))) float4 lds_leaf[];
            // lb_u is scene_body's wave-uniform copy (an SGPR) in every frame
            // kernel, so the test below never fails.  It stays because the
            // block-tile-queue kernels are scheduled around it: with lb_u used
            // as it is, variant 10 runs C3 +0.7 / +1.3% and variant 7 +1.2 /
            // -0.1% (profiles/r08/ab_block_tile_queue_split.log), and this
            // way their machine code is the one measured so far
            const uint32_t lb = lb_u != ~0u ? lb_u : leaf_buf_base(S, kNoStack);
            const float4* __restrict__ pu = prim_sp + off_u;
            const uint64_t act = __ballot(1);
            const uint32_t na = static_cast<uint32_t>(__popcll(act));
            for (uint32_t k = lane_rank(act); k < cnt_u; k += na) lds_leaf[lb + k] = pu[k];
            // (a wave's LDS operations complete in order: the reads below see
            // the writes, and the compiler keeps them in order: same array)
            return chunks([&](uint32_t k) { return lds_leaf[lb + k]; }, off_u, cnt_u);
        }
        const float4* __restrict__ ps = prim_sp + off;
        return chunks([&](uint32_t k) { return ps[k]; }, off, cnt);
    };

    if (S.root_is_leaf) {
        if (S.root.y && leaf(S.root.x, S.root.y)) return true;  // an empty scene's root holds 0
    } else {
        uint2 node = S.root;
        // Cell = (depth, lower corner l* in finest-grid units, size = G >> depth):
        // mid plane = l + size/2, exit plane = l + size: the same integers (hence
        // the same plane values) as the oracle's c * size forms, 3 VALU a plane.
        uint32_t depth = 0, l0 = 0, l1 = 0, l2 = 0, size = G;
        float t = t0;
        // Cell table: the walk enters at depth K through one
        // table load, and a step whose common ancestor lies above depth K
        // jumps the same way instead of re-reading the records down to K.
        const uint2* __restrict__ tab = S.tab;
        const uint32_t K = S.tab_k;
        bool jump = tab != nullptr;
        uint32_t from = 0;  // depth the oracle re-descends from (stats)
        // with a table, only depths >= K are ever on the stack (stack_levels);
        // the stackless walk (kNoStack) keeps one only without a table
        const uint32_t sb = K ? K - 1u : 0u;
        // Hard cap (never reached by a correct walk: a ray crosses < 3*G cells
        // and each crossing costs at most one descent): no input can hang the GPU.
        // One exit per trip (`stop`): the any-hit, nearest-done, ray-left and
        // root-left conditions are OR-ed into one flag, so the wave's exec
        // bookkeeping is one loop-exit mask update per trip (the scalar pipe is
        // this kernel's busiest unit, profiles/r02/pmc_sq_screen.json).
        // (The trip counter as a lane value, so that the cap test is a VALU
        // compare: SALU -4.0% as predicted, time C3 -0.6 / 0.0%, C5d +0.7%:
        // the scalar pipe does not bind.  profiles/r06/capv_ab.log)
        bool any_hit = false;
        for (uint32_t it = 0, cap = 8u * G + 64u;; ++it) {
            RT_BS(kBsIter);
            if (kAnyHit) RT_BS(kBsIterShadow);
            uint2 rec = make_uint2(0u, 0u);
            bool have = false;   // rec is a leaf record (else the cell is empty)
            bool inner = false;  // stepped into an internal node: descend next trip
            if (jump) {
                RT_BS(kBsJump);
                jump = false;
                // mid-plane tests at t from `depth` down to K (no loads: the
                // descent's child choices), then the cell's table entry
                while (depth < K) {
                    RT_BS(kBsJumpDescend);
                    if (kAnyHit) RT_BS(kBsJumpDescendShadow);
                    const uint32_t half = size >> 1;
                    l0 += plane(0, l0 + half) <= t ? half : 0u;
                    l1 += plane(1, l1 + half) <= t ? half : 0u;
                    l2 += plane(2, l2 + half) <= t ? half : 0u;
                    size = half;
                    depth += 1;
                }
                const uint32_t sh = D - K;
                // real cell coordinates: mirrored axes count from the far side
                // (the XOR with mt flips every mirrored field at once)
                const uint32_t c = ((((l2 >> sh) << K) | (l1 >> sh)) << K | (l0 >> sh)) ^ mt;
                const uint2 e = tab[c];
                const uint32_t kind = e.y >> kCellKindShift;
                depth = (e.y >> kCellDepthShift) & 31u;
                size = G >> depth;
                l0 &= ~(size - 1u);
                l1 &= ~(size - 1u);
                l2 &= ~(size - 1u);
                rec = make_uint2(e.x, e.y & kCellRecMask);
                // the oracle reads one record per level from `from` down to
                // the covering node (an empty child's own level reads none)
                // (a re-entry below K re-reads levels the oracle pops: none counted)
                if (kStats) {
                    const uint32_t cd = kind == kCellEmpty ? depth - 1u : depth;
                    n_nodes += cd > from ? cd - from : 0u;
                }
                inner = kind == kCellInternal;
                have = kind == kCellLeaf;
            } else {
                RT_BS(kBsDescend);
                const uint32_t half = size >> 1;
                const bool b0 = plane(0, l0 + half) <= t;
                const bool b1 = plane(1, l1 + half) <= t;
                const bool b2 = plane(2, l2 + half) <= t;
                const uint32_t bits = (b0 ? 1u : 0u) | (b1 ? 2u : 0u) | (b2 ? 4u : 0u);
                const uint32_t mbits = (mt & 1u) | ((mt >> (kf - 1u)) & 2u) |
                                       ((mt >> (2u * kf - 2u)) & 4u);
                const uint32_t child = bits ^ mbits;
                l0 += b0 ? half : 0u;
                l1 += b1 ? half : 0u;
                l2 += b2 ? half : 0u;
                size = half;
                depth += 1;
                const uint32_t valid = node.y & 0xFFu;
                have = (valid & (1u << child)) != 0;
                if (have) {
                    const uint32_t slot = node.x + __builtin_popcount(valid & ((1u << child) - 1u));
                    rec = nodes[slot];
#ifdef RT_BLOCK_STATS
                    if (depth > from) RT_BS(kBsNodeRead);
                    else RT_BS(kBsNodeReread);
#endif
                    // records down to a re-entered ancestor are the oracle's
                    // stack pops, not reads
                    if (kStats && depth > from) n_nodes += 1;
                    inner = !((node.y >> 8) & (1u << child));
                    have = !inner;
                }
            }
            // An internal node: descend next trip.  No `continue` and no break
            // inside the step: the rest of the trip is the else branch, and the
            // loop's one exit is `stop` at the end of the trip (a stopped lane's
            // step state is garbage it never uses; its pop is masked off), so
            // the structurizer keeps no exit-code variable: C3 -3.3%, C5 -3.3%,
            // C5d -3.8% (profiles/r02/inner_else_ab.log).
            bool stop = false;
            if (inner) {
                RT_BS(kBsInternal);
                node = rec;
                if (!kNoStack || !tab) stk[(depth - 1 - sb) * kBlockThreads] = rec;
            } else {
                if (have) any_hit = leaf(rec.x, rec.y);
                RT_BS(kBsExit);
                const float e0 = plane(0, l0 + size);
                const float e1 = plane(1, l1 + size);
                const float e2 = plane(2, l2 + size);
                // one v_min3_f32 (the oracle's ternaries can differ only in the sign
                // of a zero, and texit is only ever compared: identical walks)
                const float texit = fminf(fminf(e0, e1), e2);
                // step every axis whose exit plane is texit; the flipped bits give the
                // common ancestor (oracle.c: diff of the cell coordinates)
                const uint32_t n0 = e0 == texit ? l0 + size : l0;
                const uint32_t n1 = e1 == texit ? l1 + size : l1;
                const uint32_t n2 = e2 == texit ? l2 + size : l2;
                // leave on an any-hit, a nearest hit before this cell's exit, or
                // the ray's end.  The oracle's root-boundary test (a stepped
                // coordinate reaching G) needs no term of its own: an axis that
                // steps to G exits through plane(i, G), the very value t1 is
                // the minimum of, so texit >= t1 already holds there.
                // (a multi-hit walk: all kMulti entries before this cell's exit)
                float near_t = best_t;
                if constexpr (kMulti > 0) near_t = mh->t[kMulti - 1];
                stop = any_hit | (!kAnyHit & (near_t < texit)) | (texit >= t1);
                const uint32_t diff = (l0 ^ n0) | (l1 ^ n1) | (l2 ^ n2);
                const uint32_t top = 31u - __builtin_clz(diff);  // highest flipped bit
                t = texit;
                // The common ancestor: size 2^(top+1), depth D - (top+1).  With a
                // table the walk re-enters through it unless the ancestor is the
                // node it iterates (m == 1): above depth K, or (no ancestor stack)
                // two or more levels up.  A cell at depth >= K indexes the table
                // straight from the neighbour's corner (`keep`) and re-descends
                // by records; a shallower one resolves down to K from the
                // ancestor's cell.  Without a table it pops to the ancestor.
                // Selects, not branches: every lane ends the trip with the same
                // instructions (the scalar pipe carries the branches' exec-mask
                // updates, and it is the kernel's busiest unit).
                const uint32_t adepth = D - (top + 1u);
                const uint32_t m = depth - adepth;  // levels up to the ancestor
                const bool above = adepth < K || (kNoStack && K != 0u && m > 1u);
                const bool keep = above && depth >= K;
                const uint32_t asize = 2u << top;
                const uint32_t am = keep ? 0xFFFFFFFFu : ~(asize - 1u);
                l0 = n0 & am;
                l1 = n1 & am;
                l2 = n2 & am;
                size = keep ? size : asize;
                depth = keep ? depth : adepth;
                if (kStats && above) from = adepth;
                jump = above;
                // m == 1: the ancestor is the node we are iterating (still in `node`)
                if (!stop && !above && m > 1) {  // (the stackless walk: only without a table)
                    RT_BS(kBsPop);
                    node = depth ? stk[(depth - 1 - sb) * kBlockThreads] : S.root;
                }
            }
            // the safety cap shares the one exit (C3 -0.3%, profiles/r02/cap_exit_ab.log)
            if (stop || it + 1u >= cap) break;
        }
        if (any_hit) return true;
    }
    if constexpr (kMulti > 0) return mh->ref[0] != kNoHit;
    if (!kAnyHit && best_ref != kNoHit) {
        tout = best_t;
        iout = best_ref;
        return true;
    }
    return false;
}

// The octree walk of the shadow rays whose sphere has no occluder list (a
// "walk" header).  Inlined: out of line the callee is allocated without the
// kernel's 64-VGPR budget and the kernel inherits its count (5 waves per SIMD).
template <bool kNoStack>
__device__ __forceinline__ bool shadow_walk_fallback(const SceneArgs& S, float o0, float o1, float o2,
                                                  uint2* __restrict__ stk) {
    KernArgs* kl = kernargs();
    float ts;
    uint32_t is, nn = 0, np = 0;
    return walk<OccFallback<kNoStack>>(
        S, o0, o1, o2, kl->L[0], kl->L[1], kl->L[2], 0.0f, INFINITY, ts, is, nn, np, stk, true);
}

// A frame's shadow ray from a hit on the sphere of leaf reference `ref`,
// answered from that sphere's occluder list (SceneArgs::prim_occ / occ_sp,
// DESIGN.md 5.1 round 7): the list holds every sphere isect can accept from
// an origin made on that sphere, so the OR of isect over it (the walk's own
// exact test, same operands) is the walk's answer.  `hdr` = prim_occ[ref],
// loaded by the caller; lanes whose header says "walk" walk the octree.
template <bool kNoStack>
__device__ __forceinline__ bool shadow_occluded(const SceneArgs& S, uint2 hdr, bool active, float o0,
                                                float o1, float o2, uint2* __restrict__ stk) {
    KernArgs* kl = kernargs();
    const float l0 = kl->L[0], l1 = kl->L[1], l2 = kl->L[2];
    const bool walks = active && hdr.y == kOccWalk;
    const uint32_t cnt = active && !walks ? hdr.y : 0u;
    const float4* __restrict__ lst = kl->sc.occ_sp + hdr.x;
    bool occ = false;
    // (candidate k + 1 loaded before candidate k's test, four more VGPRs: C3
    // +1.4%, round 19, not kept)
    for (uint32_t k = 0; k < cnt && !occ; ++k) {
        const float4 sp = lst[k];
        float th;
        occ = isect(o0, o1, o2, l0, l1, l2, sp, 0.0f, INFINITY, th);
    }
    if (__any(walks)) {
        if (walks) occ = shadow_walk_fallback<kNoStack>(S, o0, o1, o2, stk);
    }
    return occ;
}

}  // namespace rtamd
