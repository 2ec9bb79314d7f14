// rt_kernels.hip — the scene kernels, hand-written HIP for gfx950 (MI355X,
// CDNA4): the build-defined octree path (DESIGN.md "Scene mode") that stands
// where the reference has its single CUDA kernel `raytracing`
// (src/renderer.cu:57-82) and its <<<1,1>>> setup kernels (src/renderer.cu:84-109).
//   * scene_body   : its two schedulers (block-tile queue, two-level wave
//                    queue); what a wave does per tile is in rt_shade.h and
//                    rt_sorted.h.
//   * scene_kernel, scene_kernel_w8 : the entry points, and the table of the
//                    instances that exist (launch_flags).
//   * launch_scene : the launch of a planned frame (FramePlan, rt_sched.h).
// Nothing else: the byte-exact restatement of `raytracing` and the tile unpack
// are rt_compat.hip, the per-reference record kernels rt_records.hip.
// Compiled with -ffp-contract=off: every f32/f64 expression is evaluated in
// source order with IEEE division/sqrt, exactly like oracle/oracle.c.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "rt_params.h"
#include "rt_shade.h"   // scene mode: a sample's colour, a wave tile's pixels (and the walk, the bins)
#include "rt_sorted.h"  // scene mode: quadrant-sorted rounds

namespace rtamd {

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

// Work scheduling (persistent workgroups: grid = resident workgroups):
//
// C::waveq = false: workgroups pull bts x bts block tiles from ONE device-wide
//   queue head (a returning atomic per tile); the tile's wave tiles are dealt
//   to the 4 waves round-robin, and the workgroup syncs per tile.
// C::waveq = true: every WAVE pulls tickets of 1-4 wave tiles on its own.  The
//   wave tiles are numbered in 8x8 blocks (spatially coherent) of 8x8-block
//   superblocks; whole superblocks go to XCD groups (blockIdx % 8: blocks are
//   dealt round-robin over the 8 XCDs, MI355X_MICROARCH.md "Workgroup
//   dispatch") in claim order, and each XCD has its own ticket head on its
//   own cache line (one head saturates near 88 dequeues/us) over the
//   superblocks it claimed: the two-level queue below.  No workgroup barrier;
//   the tail is one ticket.
//
// C::min_waves = minimum waves per SIMD requested from the register allocator.
// C::prog: progressive frame (a.accum set); compiled separately so plain frames
// keep their register budget.
// Residency of the wave-queue builds is set by SGPRs, not VGPRs: at 60-65
// VGPRs and 94 SGPRs (112 allocated) a SIMD holds 7 waves.  The 8-wave build
// caps its SGPRs at 80 (the rest spill into VGPR lanes, no scratch), and 8
// waves fit: C3 -1.9%, its tile path -3.3%, C5 -2.4% (84: 8 do not fit; 76
// and 72: the extra spills cost more; profiles/r02/sgpr_ab.log).
// scene_kernel_w8 below is that build of the timed default.
// C: the instance's switches by name (Frame<>, rt_sched.h, which also rules
// out the combinations no frame runs).
template <class C>
__device__ __forceinline__ void scene_body(FrameArgs a) {
    constexpr bool kTiles = C::tiles, kStats = C::stats, kWaveQ = C::waveq, kSort = C::sorted;
    extern __shared__ __attribute__((aligned(16))) float4 lds[];
    float4* acc = lds;  // [256] running pixel sums (leader lanes' slots)
    const uint32_t wave = threadIdx.x >> 6;
    // FrameLds (rt_sched.h) is this layout's statement: stk = its `stacks`,
    // wl = its `sort_waves` plus the wave's region.  Sorted rounds: no
    // per-thread pixel sums; stacks first, then each wave's colours and
    // tracing order.  (Written in elements, not from FrameLds' byte offsets:
    // those gave 21 kernels other code than the one measured, profiles/r13)
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
    // what every pixel of the frame needs of its bins beside its own bin (the
    // fallback flag, the wide list's length, the logarithms of the wave tile's
    // sides), read once per wave into one SGPR (round 19): each pixel read
    // them again through bin_info, two scalar waits at the head of its chain
    // and two dependent loads behind its entries
    uint32_t binc = 0;
    if constexpr (C::bin && !kSort)
        binc = bin_frame_consts(static_cast<uint32_t>(__builtin_ctz(a.tw)), static_cast<uint32_t>(__builtin_ctz(a.th)));
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
        // wave-tile grid of the frame, or of one packed tile: WaveGrid
        // (rt_sched.h) is its statement, and the host's; built from a WaveGrid
        // here, kernels get other code than the one measured (profiles/r13)
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
                if constexpr (C::pair) {
                    // this pixel and the next of its ticket in one pass (pair_starts,
                    // rt_sched.h); a pair that cannot be (shade_pixel_pair) is two
                    // tiles of the one-pixel path below, the only call of it
                    if (pair_starts(cur, w0, chunk) &&
                        shade_pixel_pair<C>(ox, oy, n_primary, n_shadow, binc)) {
                        ++cur;
                        continue;
                    }
                }
                if (kSort)
                    shade_pixel_sorted<C>(a, wl, stk, ox, oy, obase, n_primary, n_shadow, n_nodes,
                                          n_prims, bs);
                else
                    shade_wave_tile<C>(a, acc, stk, ox, oy, obase, n_primary, n_shadow, n_nodes,
                                       n_prims, bs, lbs, binc);
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
                shade_wave_tile<C>(a, acc, stk, ox + wox, oy + woy, obase, n_primary, n_shadow,
                                   n_nodes, n_prims, bs, lbs);
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

template <class C>
__global__ void __launch_bounds__(kBlockThreads, C::min_waves) scene_kernel(FrameArgs a) {
    static_assert(C::min_waves != 8, "the 8-wave build is scene_kernel_w8");
    scene_body<C>(a);
}

// The timed default for spp >= 8 (variant 13, plain frames): 8 waves per SIMD,
// SGPRs capped so that they fit (see above).
// C::occ: shadow rays answered from the occluder lists (a scene that has them)
// C::bin: primary rays answered from the frame's screen-space bins (a frame that built them)
template <class C>
__global__ void __launch_bounds__(kBlockThreads, 8) __attribute__((amdgpu_num_sgpr(80)))
    scene_kernel_w8(FrameArgs a) {
    static_assert(C::min_waves == 8, "plain frames of the wave queue");
    scene_body<C>(a);
}

// ---------------------------------------------------------------------------
// launch_scene (called from rt_frame.cpp): the frame's plan (FramePlan,
// rt_sched.h) and the device's occupancy numbers size the launch
// ---------------------------------------------------------------------------

// What a device holds: its CUs and, per (kernel, LDS bytes), the resident
// workgroups.  The queries are host calls: cached per device, so the launch
// path stays a single hipLaunchKernelGGL.
struct Occupancy {
    uint32_t resident, cus;
};
static Occupancy occupancy(const void* kernel, size_t lds) {
    struct Kernel {
        const void* k;
        size_t lds;
        uint32_t resident;
    };
    struct Device {
        int dev;
        uint32_t cus;
        std::vector<Kernel> kernels;
    };
    static std::mutex mu;
    static std::vector<Device> devices;
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> g(mu);
    auto d = std::find_if(devices.begin(), devices.end(), [dev](const Device& e) { return e.dev == dev; });
    if (d == devices.end()) {
        hipDeviceProp_t prop;
        const uint32_t cus = hipGetDeviceProperties(&prop, dev) == hipSuccess ? prop.multiProcessorCount : 256;
        d = devices.insert(d, Device{dev, cus, {}});
    }
    for (const Kernel& e : d->kernels)
        if (e.k == kernel && e.lds == lds) return {e.resident, d->cus};
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, kBlockThreads, lds) != hipSuccess ||
        per_cu <= 0)
        per_cu = 4;
    d->kernels.push_back({kernel, lds, d->cus * static_cast<uint32_t>(per_cu)});
    return {d->kernels.back().resident, d->cus};
}

// One instance: the 8-wave build for plain wave-queue frames, scene_kernel
// for the rest; each queue has its sizing (rt_sched.h).
template <class C>
static auto instance_kernel() {
    if constexpr (C::min_waves == 8)
        return scene_kernel_w8<C>;
    else
        return scene_kernel<C>;
}
template <class C>
static void launch_instance(FrameArgs a, const FramePlan& p, hipStream_t st) {
    const auto kernel = instance_kernel<C>();
    const size_t lds = C::waveq ? p.lds_bytes : block_tile_lds(p.lds_bytes, p.spw, a.sc.opt);
    const Occupancy o = occupancy(reinterpret_cast<const void*>(kernel), lds);
    uint32_t grid;
    if constexpr (C::waveq) {
        const WaveQueueLaunch s =
            size_wave_queue(p.grid.units(), o.resident, o.cus, C::min_waves, p.ticket, p.ticket_forced);
        a.wq_chunk = s.ticket;
        grid = s.grid;
    } else {
        const BlockTileLaunch s =
            size_block_tiles(a.W, a.H, a.tiles ? a.n_tiles : 0u, a.tile_size, p.grid.tw, p.grid.th,
                             o.resident, (a.sc.opt >> kOptBtsShift) & 7u);
        a.bts = s.side;
        grid = s.grid;
    }
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlockThreads), lds, st, a);
}

// SceneInstance -> compiled instance: the 26 that exist, each for the frame
// (kT = 0) and for a packed tile list (kT = kFTiles).  Written out, because a
// generic flag-by-flag dispatch would instantiate combinations no frame runs.
// (And the pair instance, which only frames run.)
template <uint32_t kT>
static bool launch_flags(uint32_t flags, const FrameArgs& a, const FramePlan& p, hipStream_t st) {
    switch (flags) {
#define RT_INSTANCE(f) \
    case (f): launch_instance<Frame<(f) | kT>>(a, p, st); return true;
#define RT_INSTANCE_FRAME(f) \
    case (f): if constexpr (kT == 0u) { launch_instance<Frame<(f)>>(a, p, st); return true; } else return false;
#define RT_INSTANCE_OCC(f) RT_INSTANCE(f) RT_INSTANCE((f) | kFOcc)
#define RT_INSTANCE_OCC_BIN(f) RT_INSTANCE_OCC(f) RT_INSTANCE_OCC((f) | kFBin)
        // stats frames: they walk and count (7 waves per SIMD: the counters
        // need the registers; C3 -2.8%, C5 -5.4% against 6, profiles/r01/occupancy_ab.log)
        RT_INSTANCE(kFStats)
        RT_INSTANCE(kFStats | kFProg)
        RT_INSTANCE(kFStats | kFWaveQ)
        RT_INSTANCE(kFStats | kFWaveQ | kFProg)
        RT_INSTANCE(kFStats | kFWaveQ | kFSorted)
        RT_INSTANCE(kFStats | kFWaveQ | kFSorted | kFProg)
        // plain frames of the block-tile queue
        RT_INSTANCE_OCC(0u)
        RT_INSTANCE_OCC(kFProg)
        // plain frames of the wave queue, the timed defaults (scene_kernel_w8).
        // Below 8 spp too (round 4): the block-tile queue's waves idled 28% of
        // the C2 launch at the barrier per tile; C2 0.155 -> 0.107 ms, and
        // without that queue's 3-workgroups-per-CU cap (0.152 ms with it;
        // profiles/r04/c2_timeline.log, c2_waveq_ab.log)
        RT_INSTANCE_OCC_BIN(kFWaveQ)
        RT_INSTANCE_OCC_BIN(kFWaveQ | kFProg)
        RT_INSTANCE_OCC_BIN(kFWaveQ | kFSorted)
        RT_INSTANCE_OCC_BIN(kFWaveQ | kFSorted | kFProg)
        // a binned plain frame of one-pixel wave tiles in one round (33 .. 64
        // spp): two pixels a wave pass (round 26)
        // (the frame only: launch_scene)
        RT_INSTANCE_FRAME(kFWaveQ | kFOcc | kFBin | kFPair)
#undef RT_INSTANCE_FRAME
#undef RT_INSTANCE_OCC_BIN
#undef RT_INSTANCE_OCC
#undef RT_INSTANCE
    }
    return false;
}

// Variants compiled into this build (rt_create refuses the others).
bool variant_available(uint32_t v) {
    return pick_scene_instance(v, 1, false, false, false, false, false, 0, 1).valid;
}

// p: the frame's plan (do_render made it; the frame's occluder lists and
// bins, which the steps since filled in, finish its instance)
hipError_t launch_scene(const FrameArgs& a_in, const FramePlan& p, hipStream_t st, uint32_t* instance) {
    FrameArgs a = a_in;
    // (bins: set only for a frame whose instance reads them, bins_gate)
    SceneInstance inst =
        p.inst.with(a.sc.prim_occ && a.sc.occ_sp && a.shadows, a.bin_hdr && a.bin_ent && a.bin_info);
    // packed tiles keep the one-pixel path: with pairs the tile instance needs 64
    // bytes of scratch, and a 1/8 C3 share measured +1.2% (round 26)
    if (a.tiles) inst.pair = false;
    a.spw = p.spw, a.g = p.g, a.ppw = p.ppw, a.rounds = p.rounds;
    a.tw = p.grid.tw, a.th = p.grid.th;
    a.wq_chunk = p.ticket;  // (the wave queue's launch may cap it)
    *instance = inst.flags() | (a.tiles ? kFTiles : 0u);
    // (an instance outside the table: a bug in pick_scene_instance, a failed frame)
    const bool known = inst.valid && (a.tiles ? launch_flags<kFTiles>(inst.flags(), a, p, st)
                                              : launch_flags<0u>(inst.flags(), a, p, st));
    return known ? hipGetLastError() : hipErrorInvalidDeviceFunction;
}

}  // namespace rtamd
