// rt_sched.h — how a scene frame is scheduled, stated once: which kernel
// instance runs it (SceneInstance, Frame<>), its wave-tile grid (WaveGrid), its
// workgroup's LDS layout (FrameLds), all of these as the one plan the host
// makes per frame (FramePlan), and how large the launch is (size_wave_queue,
// size_block_tiles).  Scalars only and no HIP types, so it compiles with g++
// too (tests/native/sched_dump.cpp); rt_params.h includes it.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define RT_HD __host__ __device__
#else
#define RT_HD
#endif

namespace rtamd {

constexpr int kBlockThreads = 256;  // 4 waves of 64
constexpr uint32_t kTileSide = 16;  // scene kernel: largest block tile (16x16 pixels per workgroup)

// The A/B toggles that size a launch (rt_config.flags bits 21..27, SceneArgs::opt
// bits 1..7; bit 0 is rt_params.h's), results identical either way
constexpr uint32_t kOptBtsShift = 1;       // bits 1..3: force the block-tile side (A/B):
                                           // 0 auto, 1 = 16, 2 = 8, 3 = 4, 4 = 2 pixels
constexpr uint32_t kOptNoWgCap = 1u << 7; // bit 7: 1-spp frames without the 3-workgroups-per-CU cap
constexpr uint32_t kOptChunkShift = 4;     // bits 4..6: wave-queue tiles per ticket: 0 auto
                                           // (4 / rounds, at least 1), k = 1..4 -> 1 << (k - 1);
                                           // 5..7 are refused (a ticket must not span half
                                           // a slot: the two-level queue's claim rule)
constexpr uint32_t kOptChunkMax = 4;
constexpr uint32_t kOptNoPairs = 1u << 8;  // bit 8 (RT_FLAG_NO_PAIRS: the eight rt_config bits are
                                           // taken): no pixel pairs (kFPair), every wave tile
                                           // takes the one-pixel path

// scene kernel variants (rt_config.flags bits 16..19, RT_FLAG_VARIANT_SHIFT);
// 0 picks 13 for spp >= 8, else 4 (default_variant).  Numbers of the variants
// measured and removed are not reused.
constexpr uint32_t kVariantLaneUnified = 7;   // one walk instance for primary + shadow, 2 in flight
constexpr uint32_t kVariantLaneUnified2NoStats = 10; // 7 with counters only in stats frames
constexpr uint32_t kVariantWaveQ = 13;     // unified walk scheduled per wave over per-XCD queues
                                           // (default for spp >= 8)
constexpr uint32_t kVariantWaveQLow = 4;   // the per-wave queue for spp < 8 too (no workgroup
                                           // barrier per block tile; the spp < 8 default
                                           // since round 4)
RT_HD inline uint32_t default_variant(uint32_t spp) { return spp >= 8u ? kVariantWaveQ : kVariantWaveQLow; }

// Spheres per wave in the LDS leaf buffer (a leaf of >= kLeafBuf uses global loads)
constexpr uint32_t kLeafBuf = 32;
constexpr size_t kLeafBufBytes = (kBlockThreads / 64u) * kLeafBuf * 16u;  // float4 records

// Sorted rounds (rt_sorted.h): up to 256 samples of one pixel per wave
constexpr uint32_t kSortMaxRounds = 4;
constexpr uint32_t kSortMax = 64u * kSortMaxRounds;
// per wave: per sample a slot {t, sphere} -> {lam | miss g, albedo | miss b}
// and a kind byte; the tracing order and the list of lit samples (u8 each)
constexpr uint32_t kSortCellBits = 3;  // jitter cells per axis: 2^3 (8 x 8, Morton order)
constexpr uint32_t kSortCells = 1u << (2u * kSortCellBits);
constexpr uint32_t kSortWaveBytes = kSortMax * 8u + 3u * kSortMax + kSortCells * 4u;
static_assert(kSortWaveBytes % 16u == 0u, "per-wave regions stay float4-aligned");

// Per-thread ancestor-stack levels.  Internal nodes sit at depths <
// stack_depth (the deepest leaf), and with a cell table only depths >= K are
// pushed: K .. stack_depth - 1 (C5: its tree stops at depth 8 under a
// depth-12 grid, so 2 levels, not 6).  The stackless walk (no_stack, sorted
// pixels) keeps none when there is a table: an ancestor that is not the
// current node re-enters through the table.
RT_HD inline uint32_t stack_levels(uint32_t tab_k, uint32_t stack_depth, bool no_stack = false) {
    if (no_stack && tab_k) return 0u;
    const uint32_t sb = tab_k ? tab_k - 1u : 0u;
    return stack_depth > 1u + sb ? stack_depth - 1u - sb : 1u;
}

// The workgroup's dynamic LDS, as byte offsets.  Block tiles and the plain
// wave queue: the 256 pixel sums (float4, the leader lanes' slots), the
// ancestor stacks [level][thread] (uint2), the per-wave leaf buffers.  Sorted
// rounds: no per-thread pixel sums; the stacks first (the stackless walk's),
// then each wave's colours and tracing order (kSortWaveBytes), then the leaf
// buffers.
struct FrameLds {
    uint32_t sums, stacks, sort_waves, leaf_buf, bytes;  // (a region the layout lacks: empty)
    RT_HD FrameLds(bool sorted, uint32_t tab_k, uint32_t stack_depth) {
        sums = 0u;
        stacks = sorted ? 0u : kBlockThreads * 16u;
        sort_waves = stacks + stack_levels(tab_k, stack_depth, sorted) * kBlockThreads * 8u;
        leaf_buf = sort_waves + (sorted ? (kBlockThreads / 64u) * kSortWaveBytes : 0u);
        bytes = leaf_buf + static_cast<uint32_t>(kLeafBufBytes);
    }
};

// Wave mapping of the scene kernel: spw = min(spp, 64) samples of a pixel on
// g = pow2ceil(spw) lanes, ppw = 64 / g pixels per wave as a tw x th tile.
RT_HD inline void wave_tile_shape(uint32_t spp, uint32_t& spw, uint32_t& g, uint32_t& ppw,
                                  uint32_t& tw, uint32_t& th) {
    spw = spp >= 64u ? 64u : (spp ? spp : 1u);
    g = 1;
    while (g < spw) g *= 2u;
    ppw = 64u / g;
    uint32_t lg = 0;
    while ((1u << lg) < ppw) ++lg;
    tw = 1u << ((lg + 1) / 2);
    th = 1u << (lg / 2);
}

// The wave queue's level-1 unit (scene_body): superblocks when there are
// enough of them that one superblock is a small part of an XCD's share
// (>= 192: C3 full frame (510), block slots cost it 0.6-3.4%; C4 8-way share
// (255), equal within noise) and they are mostly wave
// tiles (a packed 64x64 tile below 64 spp fills 1/4 of one or less), else
// 8x8 blocks (1/8 and 1/4 C3 tile shares, 64 and 128: -4% and -2%,
// profiles/r02/slot_size_ab.log).
#ifndef RT_SLOT_SB_MIN
#define RT_SLOT_SB_MIN 192u
#endif
RT_HD inline uint32_t wave_queue_slot_shift(uint32_t superblocks, uint32_t blocks) {
    return superblocks >= RT_SLOT_SB_MIN && 4ull * blocks >= 3ull * 64u * superblocks ? 12u : 6u;
}

// The wave-tile grid of a scene frame, or of each of n_tiles packed tiles
// (n_tiles = 0: the frame): gw x gh wave tiles of tw x th pixels, numbered in
// 8x8 blocks (nbx x nby, those that hold at least one wave tile) of 8x8-block
// superblocks (nsx x nsy; one 64x64 tile at 64 spp).
struct WaveGrid {
    uint32_t tw, th, gw, gh, nbx, nby, nsx, nsy, grids;
    RT_HD WaveGrid(uint32_t W, uint32_t H, uint32_t spp, uint32_t n_tiles, uint32_t tile_size) {
        uint32_t spw, g, ppw;
        wave_tile_shape(spp, spw, g, ppw, tw, th);
        gw = n_tiles ? tile_size / tw : (W + tw - 1) / tw;
        gh = n_tiles ? tile_size / th : (H + th - 1) / th;
        nbx = (gw + 7u) / 8u, nby = (gh + 7u) / 8u;
        nsx = (nbx + 7u) / 8u, nsy = (nby + 7u) / 8u;
        grids = n_tiles ? n_tiles : 1u;
    }
    RT_HD uint64_t units() const { return static_cast<uint64_t>(grids) * gw * gh; }  // wave tiles
    RT_HD uint32_t blocks() const { return grids * nbx * nby; }
    RT_HD uint32_t superblocks() const { return grids * nsx * nsy; }
    RT_HD uint32_t slot_shift() const { return wave_queue_slot_shift(superblocks(), blocks()); }
    // words of one XCD's slot table: a slot per level-1 unit, the claim past
    // the last one (kSlotNone) and the slot claimed half a slot early
    RT_HD uint32_t slot_stride() const { return (slot_shift() == 12u ? superblocks() : blocks()) + 2u; }
};

// ---------------------------------------------------------------------------
// The scene-kernel instance a frame runs
// ---------------------------------------------------------------------------

// A compiled instance's switches, as one word: Frame<kFWaveQ | kFOcc | kFBin>.
enum FrameFlag : uint32_t {
    kFTiles = 1u << 0,   // renders a packed tile list, not the frame
    kFStats = 1u << 1,   // counts rays, node visits and sphere tests
    kFProg = 1u << 2,    // progressive: adds onto FrameArgs::accum
    kFWaveQ = 1u << 3,   // the per-wave two-level queue (else the block-tile queue)
    kFSorted = 1u << 4,  // quadrant-sorted rounds, one pixel per wave
    kFOcc = 1u << 5,     // shadow rays answered from the occluder lists
    kFBin = 1u << 6,     // primary rays answered from the frame's screen-space bins
    kFPair = 1u << 7,    // one-pixel wave tiles shaded two to a wave pass (shade_pixel_pair)
};

template <uint32_t kF>
struct Frame {
    static constexpr bool tiles = kF & kFTiles, stats = kF & kFStats, prog = kF & kFProg,
                          waveq = kF & kFWaveQ, sorted = kF & kFSorted, occ = kF & kFOcc,
                          bin = kF & kFBin, pair = kF & kFPair;
    // waves per SIMD asked of the register allocator: plain wave-queue frames
    // are the 8-wave build (scene_kernel_w8), stats frames keep 7
    static constexpr int min_waves = waveq ? (stats ? 7 : 8) : 1;
    // unsorted wave-queue walks screen by the 8-byte image-plane records and
    // stage no leaves; the block-tile queue keeps the staged 16-byte screen
    static constexpr bool cam8 = waveq && !sorted;
    static_assert(!sorted || waveq, "sorted rounds: a wave-queue frame");
    static_assert(!occ || !stats, "stats frames walk: their counters are the oracle's");
    static_assert(!bin || (!stats && waveq), "bins: plain frames of the wave queue");
    static_assert(!pair || (bin && occ && !sorted && !prog && !tiles),
                  "pairs: binned plain frames with occluder lists, not packed tiles");
};

struct SceneInstance {
    bool valid;  // false: a variant this build does not have
    bool waveq, stats, prog, sorted, occ, bin;
    // pair_shape: the frame's wave tile is one pixel in one round and pairs are
    // not switched off (plan_scene_frame); pair: such a frame of an instance
    // that has the pair path (with())
    bool pair_shape, pair;
    RT_HD uint32_t flags() const {  // without kFTiles: the launcher's
        return (stats ? kFStats : 0u) | (prog ? kFProg : 0u) | (waveq ? kFWaveQ : 0u) |
               (sorted ? kFSorted : 0u) | (occ ? kFOcc : 0u) | (bin ? kFBin : 0u) | (pair ? kFPair : 0u);
    }
    RT_HD uint32_t min_waves() const { return waveq ? (stats ? 7u : 8u) : 1u; }
    RT_HD bool w8() const { return waveq && !stats; }  // scene_kernel_w8: the instances that read bins
    // this instance once the frame's occluder lists and bins are known
    RT_HD SceneInstance with(bool have_occ, bool have_bins) const {
        SceneInstance s = *this;
        s.occ = !stats && have_occ;
        s.bin = !stats && waveq && have_bins;
        s.pair = pair_shape && s.bin && s.occ && !sorted && !prog;
        return s;
    }
};

// The instance of a frame.  count_work: a stats frame; sort_on: false only
// under the test hook RT_SORT=0; have_occ: the scene has occluder lists, the
// frame casts shadows and its camera is inside their gate; have_bins: the
// frame built bins.  Sorted rounds: a wave-queue frame of one pixel per wave
// and 2..4 rounds, wherever the per-wave LDS still lets 8 workgroups share a
// CU.  Progressive frames run the unified walk whatever the variant: the wave
// queue from 8 spp, like variant 13.
RT_HD inline SceneInstance pick_scene_instance(uint32_t variant, uint32_t spp, bool progressive,
                                               bool count_work, bool sort_on, bool have_occ,
                                               bool have_bins, uint32_t tab_k, uint32_t stack_depth) {
    if (!variant) variant = default_variant(spp);
    SceneInstance s = {true, false, count_work, progressive, false, false, false, false, false};
    const uint32_t rounds = (spp + 63u) / 64u;
    s.sorted = sort_on && spp >= 64u && rounds >= 2u && rounds <= kSortMaxRounds &&
               FrameLds(true, tab_k, stack_depth).bytes * 8u <= 160u * 1024u &&
               (progressive || variant == kVariantWaveQ);
    if (s.sorted)
        s.waveq = true;
    else if (progressive)
        s.waveq = spp >= 8u;
    else if (variant == kVariantWaveQ || variant == kVariantWaveQLow)
        s.waveq = true;
    else if (variant == kVariantLaneUnified)
        s.stats = true;  // block-tile queue, counting in every frame
    else if (variant != kVariantLaneUnified2NoStats)
        s.valid = false;
    return s.with(have_occ, have_bins);
}

// ---------------------------------------------------------------------------
// The plan of a scene frame, made once by the host (do_render)
// ---------------------------------------------------------------------------

struct FramePlan {
    SceneInstance inst;  // before the occluder lists and the bins are known: inst.with()
    WaveGrid grid;
    // wave mapping: spw samples x ppw pixels per wave (see rt_shade.h), g =
    // pow2ceil(spw) lanes per pixel, rounds of spw samples per pixel
    uint32_t spw, g, ppw, rounds;
    uint32_t slot_shift, slot_stride;  // the wave queue's slot size and per-XCD slot-table length
    uint32_t lds_bytes;                // FrameLds of the instance
    uint32_t ticket;                   // wave tiles per ticket, before the launch's cap (size_wave_queue)
    bool ticket_forced;                // by kOptChunkShift: no cap
};

// n_tiles = 0: the frame; opt: SceneArgs::opt.
RT_HD inline FramePlan plan_scene_frame(uint32_t variant, uint32_t spp, bool progressive, bool count_work,
                                        bool sort_on, uint32_t tab_k, uint32_t stack_depth, uint32_t W,
                                        uint32_t H, uint32_t n_tiles, uint32_t tile_size, uint32_t opt) {
    FramePlan p = {pick_scene_instance(variant, spp, progressive, count_work, sort_on, false, false, tab_k,
                                       stack_depth),
                   WaveGrid(W, H, spp, n_tiles, tile_size)};
    uint32_t tw, th;
    wave_tile_shape(spp, p.spw, p.g, p.ppw, tw, th);
    p.rounds = (spp + p.spw - 1) / p.spw;
    // pixel pairs (kFPair): a wave tile is one pixel, shaded in one round (33 .. 64 spp)
    p.inst.pair_shape = p.ppw == 1u && p.rounds == 1u && !(opt & kOptNoPairs);
    p.slot_shift = p.grid.slot_shift();
    p.slot_stride = p.grid.slot_stride();
    p.lds_bytes = FrameLds(p.inst.sorted, tab_k, stack_depth).bytes;
    // wave-queue ticket size: adjacent wave tiles back to back on one wave
    // reuse its CU's L1; a ticket of about four rounds of work balances that
    // against the queue tail (C3, 1 round: 4 per ticket -4.1%; C5, 4 rounds:
    // 1 per ticket, more is slower; profiles/r01/chunk_ab.log)
    const uint32_t ck = (opt >> kOptChunkShift) & 7u;
    p.ticket = ck ? 1u << (ck - 1u) : 4u / (p.rounds < 1u ? 1u : p.rounds > 4u ? 4u : p.rounds);
    p.ticket_forced = ck != 0u;
    return p;
}

// Pixel pairs (kFPair, rt_shade.h shade_pixel_pair): inside a ticket's wave
// tiles [w0, w0 + chunk) of a slot, tile cur starts a pair with cur + 1 when it
// is even and cur + 1 belongs to the ticket.  A slot's tiles are numbered row
// by row in 8-wide blocks (scene_body), so the two are the pixels (x, y) and
// (x + 1, y), x even, of one block row: one 8x8 bin.  A tile that starts no
// pair and is not the second of one is shaded alone.
RT_HD inline bool pair_starts(uint32_t cur, uint32_t w0, uint32_t chunk) {
    return (cur & 1u) == 0u && cur + 1u < w0 + chunk;
}

// ---------------------------------------------------------------------------
// The size of a launch, from the plan and the device's occupancy numbers
// (resident: workgroups of the kernel the device holds at its LDS size)
// ---------------------------------------------------------------------------

struct WaveQueueLaunch {
    uint32_t grid, ticket;  // workgroups; wave tiles per ticket (FrameArgs::wq_chunk)
};
struct BlockTileLaunch {
    uint32_t grid, side;  // workgroups; the block-tile side in pixels (FrameArgs::bts)
};

// Per-wave queue launch: grid = resident workgroups, capped by the work.
// per_simd: the build's waves per SIMD (0: no cap); cus: the device's CUs.
RT_HD inline WaveQueueLaunch size_wave_queue(uint64_t units, uint32_t resident, uint32_t cus, uint32_t per_simd,
                                        uint32_t ticket, bool ticket_forced) {
    // (the grid only sizes the launch; padding units of edge blocks are skipped)
    const uint64_t want = (units + kBlockThreads / 64 - 1) / (kBlockThreads / 64);
    // The occupancy query counts 8 workgroups per CU for the 7-wave builds
    // (60-65 VGPRs), but their 94 SGPRs leave room for 7: the 8th per CU
    // only starts when another exits, finds nothing and adds 8 queue atomics
    // to the tail (profiles/r02/timeline_hwid.log).  Capped at the build's
    // waves per SIMD: C3 -0.8%, 1/8 share -5% (profiles/r02/steal_ab.log,
    // measured with the static per-XCD ranges that preceded the two-level queue)
    const uint64_t cap = per_simd ? static_cast<uint64_t>(cus) * per_simd : resident;
    uint64_t grid = resident < cap ? resident : cap;
    if (want < grid) grid = want;
    if (grid < 1u) grid = 1u;
    WaveQueueLaunch s = {static_cast<uint32_t>(grid), ticket};
    if (!ticket_forced) {
        // auto ticket size, second half: a small launch (a multi-GPU share)
        // has few units per wave, and big tickets lengthen its tail. N-way
        // C3 shares: 4 per ticket best at 1/2 and 1/4, 2 at 1/8 (36 units a
        // wave; profiles/r01/shard_chunk.log)
        const uint64_t per_wave = units / (grid * (kBlockThreads / 64));
        const uint32_t most = per_wave >= 64 ? 4u : per_wave >= 16 ? 2u : 1u;
        if (most < s.ticket) s.ticket = most;
    }
    return s;
}

// Block tiles in the frame (or in the packed tile list) for block-tile side b.
RT_HD inline uint32_t count_block_tiles(uint32_t W, uint32_t H, uint32_t n_tiles, uint32_t tile_size,
                                        uint32_t b) {
    if (n_tiles) return n_tiles * (tile_size / b) * (tile_size / b);
    return ((W + b - 1) / b) * ((H + b - 1) / b);
}

// Persistent launch: grid = resident workgroups; the block-tile side shrinks
// (16 -> 8 -> 4 pixels, never below two wave tiles) until the tile queue holds
// >= 8 tiles per resident workgroup, so the dynamic queue can even out costly
// image regions to the end (A/B, profiles/r01/bts_ab.log: 1080p 64 spp picks
// 8x8 tiles, -6.4% vs 16x16; a 1/4 or 1/8 multi-GPU share picks 4x4).
// force: kOptBtsShift's field (0: auto; a side below two wave tiles is not forced).
RT_HD inline BlockTileLaunch size_block_tiles(uint32_t W, uint32_t H, uint32_t n_tiles, uint32_t tile_size,
                                              uint32_t tw, uint32_t th, uint32_t resident, uint32_t force) {
    const uint32_t min_side = 2u * (tw > th ? tw : th);
    uint32_t bts = kTileSide;
    if (force && (kTileSide >> (force - 1u)) >= min_side)
        bts = kTileSide >> (force - 1u);
    else
        while (bts / 2u >= min_side && count_block_tiles(W, H, n_tiles, tile_size, bts) < 8u * resident)
            bts /= 2u;
    const uint32_t tiles = count_block_tiles(W, H, n_tiles, tile_size, bts);
    return {tiles < resident ? tiles : resident, bts};
}

// The block-tile queue's dynamic LDS.  1 spp: a wave's 64 lanes are 64
// different pixels, whose walks thrash the L1 when 5 workgroups share a CU;
// the dynamic LDS is padded so that at most 3 are resident (C2: 0.358 ->
// 0.274 ms; 2 or 4 per CU slower, 4 spp unchanged; profiles/r01/c2_wg_cap_ab.log)
constexpr uint32_t kOneSppLds = (160u * 1024u / 3u) & ~15u;  // 3 workgroups per CU
RT_HD inline uint32_t block_tile_lds(uint32_t lds_bytes, uint32_t spw, uint32_t opt) {
    return spw == 1u && !(opt & kOptNoWgCap) && lds_bytes < kOneSppLds ? kOneSppLds : lds_bytes;
}

}  // namespace rtamd
