// rt_frame.cpp — what a renderer queues per call: a frame's preparation and
// launch (do_render and its steps), tile frames, ray queries, the G-buffer.
// The arithmetic the images depend on is rt_frame_math.h's.
#include "rt_bins_math.h"
#include "rt_frame_math.h"
#include "rt_host.h"

using namespace rtamd;

namespace rtamd {

void fill_frame_args(rt_renderer* r, FrameArgs& a) {
    memset(&a, 0, sizeof(a));
    fill_camera(r, a.cam);
    a.sc = r->sc;
    a.W = r->W;
    a.H = r->H;
    a.spp = r->cfg.spp ? r->cfg.spp : 1;
    a.seedmix = mix32(r->cfg.seed ^ 0x9E3779B9u);
    bool jitter = a.spp > 1;
    if (r->cfg.flags & RT_FLAG_JITTER) jitter = true;
    if (r->cfg.flags & RT_FLAG_NO_JITTER) jitter = false;
    a.jitter = jitter ? 1u : 0u;
    a.shadows = (r->cfg.flags & RT_FLAG_NO_SHADOWS) ? 0u : 1u;
    a.contract = (r->cfg.flags & RT_FLAG_COMPAT_FMA) ? 1u : 0u;
    const float* ld = r->cfg.light_dir;
    const float ll = sqrtf(ld[0] * ld[0] + ld[1] * ld[1] + ld[2] * ld[2]);
    a.L[0] = -(ld[0] / ll);
    a.L[1] = -(ld[1] / ll);
    a.L[2] = -(ld[2] / ll);
    a.ambient = r->cfg.ambient;
    a.inv_spp = 1.0f / static_cast<float>(a.spp);
    if ((r->cfg.flags & RT_FLAG_PROGRESSIVE) && r->cfg.mode == RT_MODE_SCENE) {
        // frame k traces samples [k*spp, (k+1)*spp) and adds them onto the
        // stored sums: after K frames the image is the mean of K*spp samples
        // (identical to one K*spp frame when spp is a multiple of 64)
        if (uint64_t(r->frames_accum + 1) * a.spp >= (1ull << 31)) r->frames_accum = 0;
        a.accum = r->accum.p;
        a.s_base = r->frames_accum * a.spp;
        a.accum_in = r->frames_accum ? 1u : 0u;
        a.inv_spp = 1.0f / static_cast<float>((r->frames_accum + 1) * a.spp);
    }
    a.counters = r->counters.p;
    a.sc.opt = (r->cfg.flags >> RT_FLAG_OPT_SHIFT) & 0xFFu;
    a.wq_claim_delay = r->test_claim_delay;
    a.qerr = r->qerr_dev;
    if (++r->frame_seq == 0) r->frame_seq = 1;
    a.frame_id = r->frame_seq;
    const uint32_t v = (r->cfg.flags >> RT_FLAG_VARIANT_SHIFT) & 0xFu;
    // default: multi-sample frames are scheduled per wave over per-XCD queues
    // (variant 13: C5 -15%, equal on C3, better on multi-GPU shares); 1-spp
    // frames (8x8-pixel wave tiles) keep the block-tile queue (tools/variants.py A/B,
    // profiles/r01/wave_queue_ab.log)
    // spp < 8: the block-tile queue with counters only in stats frames (C2
    // 0.185 -> 0.168 ms against the always-counting build 7,
    // profiles/r02/c2_variant_ab.log)
    // round 4: spp < 8 frames take the per-wave queue too (variant 4, no
    // workgroup barrier per block tile: C2 0.155 -> 0.107 ms,
    // profiles/r04/c2_waveq_ab.log)
    a.variant = v ? v : default_variant(a.spp);
}

int check_tiles(rt_renderer* r, const uint32_t* ids, uint32_t n_tiles, uint32_t ts,
                bool allow_skip) {
    if (ts == 0 || ts % 64 != 0 || ts > 4096)
        return fail(r, RT_E_INVALID, "tile_size must be a multiple of 64 in [64, 4096]");
    const uint32_t tx = (r->W + ts - 1) / ts, ty = (r->H + ts - 1) / ts;
    for (uint32_t i = 0; i < n_tiles; ++i)
        if (ids[i] >= tx * ty && !(allow_skip && ids[i] == RT_TILE_SKIP))
            return fail(r, RT_E_INVALID, "tile id out of range");
    return RT_OK;
}

// Device copy of a tile list: found in the cache when the same list was used
// recently (steady-state frames never copy or synchronise), else uploaded
// asynchronously into the least recently used slot.
constexpr size_t kTileListSlots = 16;

int tile_list(rt_renderer* r, const uint32_t* ids, uint32_t n, hipStream_t s, const uint32_t** out) {
    rt_renderer::TileList* hit = nullptr;
    for (auto& e : r->tile_lists)
        if (e.host.size() == n && e.dev.p && memcmp(e.host.data(), ids, n * sizeof(uint32_t)) == 0) {
            hit = &e;
            break;
        }
    if (!hit) {
        if (r->tile_lists.size() < kTileListSlots) {
            r->tile_lists.emplace_back();
            hit = &r->tile_lists.back();
        } else {
            hit = &r->tile_lists[0];
            for (auto& e : r->tile_lists)
                if (e.used < hit->used) hit = &e;
            // its previous upload may still be in flight on some stream
            RT_HIP(r, hipDeviceSynchronize());
        }
        int st;
        if ((st = ensure(r, hit->dev, n))) return st;
        hit->host.assign(ids, ids + n);
        RT_HIP(r, hipMemcpyAsync(hit->dev.p, hit->host.data(), n * sizeof(uint32_t),
                                 hipMemcpyHostToDevice, s));
    }
    hit->used = ++r->tile_clock;
    *out = hit->dev.p;
    return RT_OK;
}

// Progressive sums belong to one pixel set: the full frame (sig 1) or one
// tile list; rendering another set starts the accumulation over.
void accum_pixels(rt_renderer* r, const uint32_t* ids, uint32_t n, uint32_t ts) {
    const uint64_t sig = pixel_set_signature(ids, n, ts);
    if (sig != r->accum_sig) r->frames_accum = 0;
    r->accum_sig = sig;
}

// SceneArgs::prim_al, the albedo of every leaf reference: made once per scene
// on `st`, by the first frame or G-buffer call that shades from it.
int ensure_prim_al(rt_renderer* r, SceneArgs& sc, hipStream_t st) {
    bool stale;
    if (const int ost = r->prim_al.query(r, r->prim_slots + kPrimPad, r->scene_gen, nullptr, 0, &stale))
        return ost;
    if (stale) {
        hipError_t e = launch_albedo_refs(sc.prim_idx, sc.albedo, r->prim_slots, r->n_spheres,
                                          r->prim_al.buf.p, st);
        if (e != hipSuccess) return hip_fail(r, e, "albedo by leaf reference");
        r->prim_al.commit(r->scene_gen, nullptr, 0);
    }
    sc.prim_al = r->prim_al.buf.p;
    return RT_OK;
}

}  // namespace rtamd

namespace {

// RT_FLAG_TEST_POISON: the frame's outputs filled with a sentinel first
// (rt.h), so a pixel no kernel writes shows in the readback.
int poison_outputs(rt_renderer* r, const FrameArgs& a, hipStream_t st) {
    if (!(r->cfg.flags & RT_FLAG_TEST_POISON)) return RT_OK;
    const size_t px = a.tiles ? (size_t)a.n_tiles * a.tile_size * a.tile_size : (size_t)a.W * a.H;
    RT_HIP(r, hipMemsetAsync(a.out8, 0xAB, px * 4, st));
    // (the compat kernel writes RGBA8 only: no radiance to check there)
    if (a.out32 && r->cfg.mode == RT_MODE_SCENE)
        RT_HIP(r, hipMemsetAsync(a.out32, 0xFF, (size_t)a.W * a.H * 16, st));
    if (a.accum && !a.accum_in) RT_HIP(r, hipMemsetAsync(a.accum, 0xFF, (size_t)a.W * a.H * 16, st));
    return RT_OK;
}

// The work counters of a stats launch: {primary, shadow, nodes, prims} per XCD
// group, one line each (kStatLineBase), summed into c.
constexpr size_t kStatLineWords = 8 * kStatLineStride;
void sum_stat_lines(const unsigned long long* lines, unsigned long long c[4]) {
    for (uint32_t i = 0; i < 4; ++i) c[i] = 0;
    for (uint32_t q = 0; q < 8; ++q)
        for (uint32_t i = 0; i < 4; ++i) c[i] += lines[q * kStatLineStride + i];
}

// ---- do_render's steps, in its order: each queues on `st` and fills its part of `a` ----

// Step 1: this frame's counter set (RendererState::ctr_set) and, for the wave
// queue, its per-XCD slot table (8 x (superblocks + 2) words after the
// counters), zero when the kernel starts; the other set is the one the kernel
// zeroes for the next frame.  counters_after_launch is the other half.
int frame_counters(rt_renderer* r, FrameArgs& a, hipStream_t st) {
    const bool scene = r->cfg.mode == RT_MODE_SCENE;
    size_t words = kCounterWords;  // one set
    a.wq_slots = nullptr;
    a.wq_slot_stride = 0;
    if (scene) {
        const WaveGrid grid(a.W, a.H, a.spp, a.tiles ? a.n_tiles : 0u, a.tile_size);
        a.wq_slot_shift = grid.slot_shift();
        a.wq_slot_stride = (a.wq_slot_shift == 12u ? grid.superblocks() : grid.blocks()) + 2u;
        words += (8u * static_cast<size_t>(a.wq_slot_stride) + 1u) / 2u;
    }
    if (r->ctr_stride < words) {  // (re)allocate both sets and zero them
        if (const int ost = ensure(r, r->counters, 2 * words)) return ost;
        r->ctr_stride = r->counters.n / 2;
        RT_HIP(r, hipMemsetAsync(r->counters.p, 0, r->counters.n * sizeof(unsigned long long), st));
        r->ctr_zero[0] = r->ctr_zero[1] = r->ctr_stride;
    }
    const uint32_t cs = r->ctr_set;
    a.counters = r->counters.p + cs * r->ctr_stride;
    if (r->ctr_zero[cs] < words)  // (after a failed launch, or a frame needing more words)
        RT_HIP(r, hipMemsetAsync(a.counters, 0, words * sizeof(unsigned long long), st));
    if (a.wq_slot_stride) a.wq_slots = reinterpret_cast<uint32_t*>(a.counters + kCounterWords);
    a.ctr_next = scene ? r->counters.p + (1u - cs) * r->ctr_stride : nullptr;
    a.ctr_next_words = scene ? static_cast<uint32_t>(words) : 0u;
    return RT_OK;
}

// ... after the launch: a scene frame dirtied its set and zeroed the other
// one, which the next frame takes; after a failed launch neither set is
// known to be zero.
void counters_after_launch(rt_renderer* r, const FrameArgs& a, bool launched) {
    const uint32_t cs = r->ctr_set;
    if (!launched) {
        r->ctr_zero[0] = r->ctr_zero[1] = 0;
    } else if (a.ctr_next) {
        r->ctr_zero[cs] = 0;
        r->ctr_zero[1u - cs] = a.ctr_next_words;
        r->ctr_set = 1u - cs;
    }
}

// Step 2: the superblock claim order of a full frame (RT_SB_ORDER=1, a test
// hook), uploaded when the superblock grid changes.
int superblock_order(rt_renderer* r, FrameArgs& a, hipStream_t) {
    a.sb_order = nullptr;
    if (r->cfg.mode != RT_MODE_SCENE || a.tiles || a.wq_slot_shift != 12u || !r->sb_hilbert) return RT_OK;
    const WaveGrid grid(a.W, a.H, a.spp, 0u, 0u);
    const uint32_t nx = grid.nsx, ny = grid.nsy;  // the superblock grid of this frame
    if (r->sb_nx != nx || r->sb_ny != ny || !r->sb_order.p) {
        const std::vector<uint32_t> ord = hilbert_order(nx, ny);
        if (const int ost = ensure(r, r->sb_order, ord.size())) return ost;
        RT_HIP(r, hipMemcpy(r->sb_order.p, ord.data(), ord.size() * sizeof(uint32_t),
                            hipMemcpyHostToDevice));
        r->sb_nx = nx;
        r->sb_ny = ny;
    }
    a.sb_order = r->sb_order.p;
    return RT_OK;
}

// Step 3a: the records of this frame's camera: the
// camera-relative ones (key: the origin) and the image-plane ones (origin,
// basis, check), remade on this stream, after the renderer's earlier frames
// (order_after_last), when their key or the scene changed.
int camera_records(rt_renderer* r, FrameArgs& a, hipStream_t st) {
    const uint32_t nr = r->prim_slots + kPrimPad;
    bool stale;
    int ost;
    if ((ost = r->prim_cam.query(r, nr, r->scene_gen, a.cam.o, 3, &stale))) return ost;
    if (stale) {
        hipError_t e = launch_cam_screen(a.sc.prim_sp, nr, a.cam.o, r->prim_cam.buf.p, st);
        if (e != hipSuccess) return hip_fail(r, e, "camera-relative screen records");
        r->prim_cam.commit(r->scene_gen, a.cam.o, 3);
    }
    a.sc.prim_cam = r->prim_cam.buf.p;
    const uint32_t ok = cam8_basis(a.cam.K, a.cam.R, a.W, a.H, a.cam8_B);
    float key[13];
    memcpy(key, a.cam.o, sizeof(a.cam.o));
    memcpy(key + 3, a.cam8_B, sizeof(a.cam8_B));
    key[12] = ok ? 1.0f : 0.0f;
    if ((ost = r->prim_cam8.query(r, nr, r->scene_gen, key, 13, &stale))) return ost;
    if (stale) {
        hipError_t e = launch_cam8_screen(a.sc.prim_sp, nr, a.cam.o, a.cam8_B, ok, r->prim_cam8.buf.p, st);
        if (e != hipSuccess) return hip_fail(r, e, "image-plane screen records");
        r->prim_cam8.commit(r->scene_gen, key, 13);
    }
    a.sc.prim_cam8 = r->prim_cam8.buf.p;
    return RT_OK;
}

// Step 4 (called from 3b): the occluder lists of this scene and light
// (DESIGN.md 5.1 round 7), around the ONE wait of a light-plane refresh: the
// counting passes and their totals ride on it with the radius term's copy
// (light_records), the fill is queued after it.
int occluder_lists(rt_renderer* r, const FrameArgs& a, double delta, double M, hipStream_t st) {
    const bool want_occ = !(r->cfg.flags & RT_FLAG_NO_OCCLUDERS) && a.shadows;
    r->occ.off();
    r->occ_timed = false;
    r->info.occluder_build_ms = 0.0;
    r->info.occluder_entries = 0;
    r->info.occluder_lists_on = 0;
    if (want_occ) {
        RT_HIP(r, hipEventRecord(r->occ_e0, st));
        hipError_t e = r->occ.count(r->d_spheres.p, r->n_spheres, a.L, a.shd_e, delta, M, r->occ_cap, st);
        if (e != hipSuccess) {
            // count()'s own copies may be queued into its state: wait before leaving
            (void)hipStreamSynchronize(st);
            return hip_fail(r, e, "occluder lists (count)");
        }
        r->occ_M = M;
    }
    RT_HIP(r, hipStreamSynchronize(st));
    if (want_occ) {
        hipError_t e = r->occ.fill(a.sc.prim_idx, r->prim_slots, r->occ_mean_max, st);
        if (e != hipSuccess) return hip_fail(r, e, "occluder lists (fill)");
        RT_HIP(r, hipEventRecord(r->occ_e1, st));
        r->occ_timed = true;
        r->info.occluder_lists_on = r->occ.on() ? 1u : 0u;
        r->info.occluder_entries = r->occ.on() ? r->occ.totals().entries : 0u;
    }
    return RT_OK;
}

// Step 3b: the light-plane screen: the basis of the plane perpendicular to
// the shadow direction a.L, the records of the centres in it and their radius
// term, remade with the occluder lists when the scene or the basis changes
// (once per scene and light, a sync).
int light_records(rt_renderer* r, FrameArgs& a, hipStream_t st) {
    const uint32_t nr = r->prim_slots + kPrimPad;
    light_plane_basis(a.L, a.shd_e);
    bool stale;
    int ost;
    if ((ost = r->prim_shd8.query(r, nr, r->scene_gen, a.shd_e, 6, &stale))) return ost;
    const uint32_t nbk = (nr + kBlockThreads - 1u) / kBlockThreads;  // shd_screen_kernel's blocks
    if ((ost = ensure(r, r->d_shd_rr, nbk + 1u))) return ost;
    if (stale) {
        const double M = root_reach(r->info.root_min, r->info.root_max) + 1e-4;
        const double delta = kShadowSlackM / 16777216.0 * M;
        RT_HIP(r, hipMemsetAsync(r->d_shd_rr.p, 0, (nbk + 1u) * sizeof(uint32_t), st));
        hipError_t e = launch_shd_screen(a.sc.prim_sp, nr, a.shd_e, delta, r->prim_shd8.buf.p,
                                         r->d_shd_rr.p, st);
        if (e != hipSuccess) return hip_fail(r, e, "light-plane screen records");
        // the radius term lands in the renderer, which outlives every early
        // return below; it counts once the wait in occluder_lists is over
        RT_HIP(r, hipMemcpyAsync(&r->shd_rr_bits, r->d_shd_rr.p + nbk, sizeof(r->shd_rr_bits),
                                 hipMemcpyDeviceToHost, st));
        if ((ost = occluder_lists(r, a, delta, M, st))) return ost;
        memcpy(&r->shd_rr, &r->shd_rr_bits, sizeof(r->shd_rr));
        r->prim_shd8.commit(r->scene_gen, a.shd_e, 6);
    }
    a.sc.prim_shd8 = r->prim_shd8.buf.p;
    a.shd_rr = r->shd_rr;
    return RT_OK;
}

// The far-camera gate: whether this frame's camera is within the distance the
// occluder lists were derived for (occ_camera_in_gate); a frame from farther
// away walks: the kOcc = false instances.
bool camera_in_occluder_gate(const rt_renderer* r, const FrameArgs& a) {
    return occ_camera_in_gate(a.cam.o, r->info.root_min, r->info.root_max, kOccCamGate * r->occ_M);
}

// Step 4b: this frame's screen-space bins (screen_bins.hip, DESIGN.md 5.1
// round 10), queued on `st` ahead of the frame kernel: built by every plain
// frame whose kernel reads them, never keyed on the pose (the Displayer's
// camera moves every frame), with no wait and no readback.  The buffer sizes
// are fixed here; a frame whose entries do not fit sets its device flag and
// walks, the flag lands in the renderer's pinned words, and the next frame
// that sees it grows the buffer.
int screen_bins(rt_renderer* r, FrameArgs& a, hipStream_t st) {
    a.bin_hdr = nullptr;
    a.bin_ent = nullptr;
    a.bin_nb = 0;
    a.bin_wide = nullptr;
    a.bin_info = nullptr;
    a.bin_nbx = 0;
    r->bin_timed = false;
    if (r->cfg.flags & RT_FLAG_NO_BINS) return r->bin_last_reason = RT_BINS_OFF_FLAG, RT_OK;
    if (a.count_work || !frame_reads_bins(a, r->sort_rounds) ||
        static_cast<uint64_t>(a.W) * a.H * a.spp < r->bin_min_samples)
        return r->bin_last_reason = RT_BINS_OFF_KERNEL, RT_OK;
    float B[9];
    if (!bins_camera_ok(a.cam.K, a.cam.R, a.cam.o) || !cam8_basis(a.cam.K, a.cam.R, a.W, a.H, B))
        return r->bin_last_reason = RT_BINS_OFF_CAMERA, RT_OK;
    // a scene the device rule found too dense: probe once in kBinDenseSkip + 1 frames
    if (r->bin_skip_gen != r->scene_gen) r->bin_dense_skip = 0, r->bin_skip_gen = r->scene_gen;
    if (!r->bin_dense_skip && r->bin_last_frame && r->bin_mirror[kBinInfoFrame] == r->bin_last_frame &&
        r->bin_mirror[kBinInfoFlag] == kBinFlagDense) {
        // (this frame is the first of the kBinDenseSkip skipped ones: the block below counts it)
        r->bin_dense_skip = kBinDenseSkip;
        r->bin_last_frame = 0;  // (this observation is used up: the probe makes the next one)
    }
    if (r->bin_dense_skip) {
        --r->bin_dense_skip;
        return r->bin_last_reason = RT_BINS_OFF_DENSE, RT_OK;
    }
    int ost;
    bool stale;
    if ((ost = r->bin_first_ref.query(r, std::max(1u, r->n_spheres), r->scene_gen, nullptr, 0, &stale))) return ost;
    if (stale) {
        hipError_t e = launch_first_refs(a.sc.prim_sp, a.sc.prim_idx, r->prim_slots, r->d_spheres.p,
                                         r->n_spheres, r->bin_first_ref.buf.p, st);
        if (e != hipSuccess) return hip_fail(r, e, "screen bins (first references)");
        r->bin_first_ref.commit(r->scene_gen, nullptr, 0);
    }
    const uint32_t nbx = (a.W + kBinSide - 1u) / kBinSide, nby = (a.H + kBinSide - 1u) / kBinSide;
    const uint32_t nb = nbx * nby;
    // the entry buffer: 6 per sphere to start with (C3 needs 3.1, C5 2.0), grown
    // when the last frame that built bins reported that it did not fit
    // (RT_TEST_BIN_CAPACITY: a tiny first buffer, so the first frame overflows)
    size_t want = r->bin_capacity_test ? r->bin_capacity_test : 6ull * r->n_spheres + 65536ull;
    if (r->bin_last_frame && r->bin_mirror[kBinInfoFrame] == r->bin_last_frame &&
        (r->bin_mirror[kBinInfoFlag] & kBinFlagCapacity))
        want = std::max<size_t>(want, size_t(r->bin_mirror[kBinInfoEntries]) + r->bin_mirror[kBinInfoEntries] / 4u);
    want = std::min<size_t>(std::max<size_t>(want, r->bin_ent.n / 2), 0x7FFFFFFFull / 4u);
    if (r->bin_ent.n < 2 * want) {
        // (the buffer may still be read by a frame in flight on another stream)
        if (r->bin_ent.p) RT_HIP(r, hipDeviceSynchronize());
        if ((ost = ensure(r, r->bin_ent, 2 * want))) return ost;
    }
    if ((ost = ensure(r, r->bin_rects, std::max(1u, r->n_spheres))) ||
        (ost = ensure(r, r->bin_cnt, 2ull * nb + 1ull)) || (ost = ensure(r, r->bin_offs, nb + 1ull)) ||
        (ost = ensure(r, r->bin_hdr, size_t(nb) * (1u + kBinCap))) ||  // (and the tile words)
        (ost = ensure(r, r->bin_wide, 2ull * kBinWideCap)) ||
        (ost = ensure(r, r->bin_info, kBinInfoWords)))
        return ost;
    if (r->bin_temp_items < nb + 1u || !r->bin_temp.p) {
        const size_t bytes = bins_scan_temp_bytes(nb + 1u);
        if (!bytes) return fail(r, RT_E_HIP, "screen bins: scan scratch size");
        if ((ost = ensure(r, r->bin_temp, bytes))) return ost;
        r->bin_temp_items = nb + 1u;
    }
    BinBuild b{};
    b.spheres = r->d_spheres.p;
    b.first_ref = r->bin_first_ref.buf.p;
    b.n_spheres = r->n_spheres;
    memcpy(b.K, a.cam.K, sizeof(b.K));
    memcpy(b.R, a.cam.R, sizeof(b.R));
    memcpy(b.o, a.cam.o, sizeof(b.o));
    b.W = a.W;
    b.H = a.H;
    b.nbx = nbx;
    b.nby = nby;
    {  // the wave tile launch_scene gives this frame's kernel
        const WaveGrid grid(a.W, a.H, a.spp, a.tiles ? a.n_tiles : 0u, a.tile_size);
        b.tw = grid.tw;
        b.th = grid.th;
    }
    b.shrink = r->bin_shrink;
    b.capacity = static_cast<uint32_t>(r->bin_ent.n / 2);
    b.cap = r->bin_cap;
    b.mean_max = r->bin_mean_max;
    b.frame_id = a.frame_id;
    b.rects = r->bin_rects.p;
    b.counts = r->bin_cnt.p;
    b.cursor = r->bin_cnt.p + nb + 1u;
    b.offs = r->bin_offs.p;
    b.hdr = r->bin_hdr.p;
    b.ent = r->bin_ent.p;
    b.tiles = reinterpret_cast<unsigned long long*>(r->bin_hdr.p + nb);
    b.wide = r->bin_wide.p;
    b.info = r->bin_info.p;
    b.mirror = r->bin_mirror_dev;
    b.temp = r->bin_temp.p;
    b.temp_bytes = r->bin_temp.n;
    if (r->bin_timing) RT_HIP(r, hipEventRecord(r->bin_e0, st));
    hipError_t e = launch_screen_bins(b, st);
    if (e != hipSuccess) return hip_fail(r, e, "screen bins");
    if (r->bin_timing) {
        RT_HIP(r, hipEventRecord(r->bin_e1, st));
        r->bin_timed = true;
    }
    r->bin_last_reason = RT_BINS_ON;  // (the device flag may still send the frame walking: rt_get_bin_info)
    r->bin_last_frame = a.frame_id;
    r->bin_last_capacity = b.capacity;
    r->bin_nbx = nbx;
    r->bin_nby = nby;
    r->bin_tw = b.tw;
    r->bin_th = b.th;
    a.bin_hdr = r->bin_hdr.p;
    a.bin_ent = r->bin_ent.p;
    a.bin_nb = nb;
    a.bin_wide = r->bin_wide.p;
    a.bin_info = r->bin_info.p;
    a.bin_nbx = nbx;
    return RT_OK;
}

// The two diagnostic builds, each a begin / end pair around the launch (empty in the product).
#ifdef RT_TIMELINE
// tools/timeline.sh: every frame appends its per-wave timeline to $RT_TIMELINE_FILE
unsigned long long* g_timeline = nullptr;
constexpr size_t kTlWaves = 1u << 16;
constexpr size_t kTlWords = kTlWaves * 4 + (3u << 22) + kTlWaves * 2;  // per wave, per unit, phases
int timeline_begin(rt_renderer* r, FrameArgs& a, hipStream_t st) {
    if (!getenv("RT_TIMELINE_FILE")) return RT_OK;
    if (!g_timeline) RT_HIP(r, hipMalloc(reinterpret_cast<void**>(&g_timeline), kTlWords * 8));
    RT_HIP(r, hipMemsetAsync(g_timeline, 0, kTlWords * 8, st));
    a.timeline = g_timeline;
    return RT_OK;
}
int timeline_end(rt_renderer* r, const FrameArgs& a, hipStream_t st) {
    if (!a.timeline) return RT_OK;
    std::vector<unsigned long long> h(kTlWords);
    RT_HIP(r, hipStreamSynchronize(st));
    RT_HIP(r, hipMemcpy(h.data(), g_timeline, kTlWords * 8, hipMemcpyDeviceToHost));
    if (FILE* f = fopen(getenv("RT_TIMELINE_FILE"), "ab")) {
        fwrite(h.data(), 8, h.size(), f);
        fclose(f);
    }
    return RT_OK;
}
#else
inline int timeline_begin(rt_renderer*, FrameArgs&, hipStream_t) { return RT_OK; }
inline int timeline_end(rt_renderer*, const FrameArgs&, hipStream_t) { return RT_OK; }
#endif
#ifdef RT_BLOCK_STATS
// tools/block_stats.py: stats frames count the wave executions of every walk
// block and append them to $RT_BLOCK_STATS_FILE
unsigned long long* g_bstats = nullptr;
int block_stats_begin(rt_renderer* r, FrameArgs& a, hipStream_t st) {
    a.bstats = nullptr;
    if (!a.count_work || !getenv("RT_BLOCK_STATS_FILE")) return RT_OK;
    if (!g_bstats) RT_HIP(r, hipMalloc(reinterpret_cast<void**>(&g_bstats), 2 * kBlockStats * 8));
    RT_HIP(r, hipMemsetAsync(g_bstats, 0, 2 * kBlockStats * 8, st));
    a.bstats = g_bstats;
    return RT_OK;
}
int block_stats_end(rt_renderer* r, const FrameArgs& a, hipStream_t st) {
    if (!a.bstats) return RT_OK;
    unsigned long long h[2 * kBlockStats];
    RT_HIP(r, hipStreamSynchronize(st));
    RT_HIP(r, hipMemcpy(h, g_bstats, sizeof(h), hipMemcpyDeviceToHost));
    if (FILE* f = fopen(getenv("RT_BLOCK_STATS_FILE"), "a")) {
        fprintf(f, "{\"W\": %u, \"H\": %u, \"spp\": %u, \"counts\": [", a.W, a.H, a.spp);
        for (uint32_t i = 0; i < 2 * kBlockStats; ++i) fprintf(f, "%s%llu", i ? ", " : "", h[i]);
        fprintf(f, "]}\n");
        fclose(f);
    }
    return RT_OK;
}
#else
inline int block_stats_begin(rt_renderer*, FrameArgs&, hipStream_t) { return RT_OK; }
inline int block_stats_end(rt_renderer*, const FrameArgs&, hipStream_t) { return RT_OK; }
#endif

// Step 5: poison (test only), launch, and the renderer's bookkeeping of a queued frame.
int launch_frame(rt_renderer* r, FrameArgs& a, hipStream_t st) {
    int ost;
    if ((ost = timeline_begin(r, a, st)) || (ost = block_stats_begin(r, a, st))) return ost;
    hipError_t e = r->cfg.mode == RT_MODE_SCENE ? launch_scene(a, r->sort_rounds, st) : launch_compat(a, st);
    counters_after_launch(r, a, e == hipSuccess);
    if (e != hipSuccess) return hip_fail(r, e, "kernel launch");
    if ((ost = block_stats_end(r, a, st)) || (ost = mark_queued(r, st))) return ost;
    if ((ost = timeline_end(r, a, st))) return ost;
    if (a.accum) ++r->frames_accum;
    return RT_OK;
}

// Step 6: a stats frame waits for its kernel (events ev0 .. ev1) and reads the counters.
int frame_stats(rt_renderer* r, const FrameArgs& a, hipStream_t st, rt_stats* stats) {
    RT_HIP(r, hipEventRecord(r->ev1, st));
    RT_HIP(r, hipEventSynchronize(r->ev1));
    occ_collect_time(r);
    unsigned long long lines[kStatLineWords], c[4];
    RT_HIP(r, hipMemcpy(lines, a.counters + kStatLineBase, sizeof(lines), hipMemcpyDeviceToHost));
    sum_stat_lines(lines, c);
    float ms = 0.f;
    RT_HIP(r, hipEventElapsedTime(&ms, r->ev0, r->ev1));
    memset(stats, 0, sizeof(*stats));
    const uint64_t px = a.tiles ? 0 : (uint64_t)a.W * a.H;
    stats->primary_rays = r->cfg.mode == RT_MODE_SCENE ? c[0] : px;
    stats->shadow_rays = c[1];
    stats->nodes_visited = c[2];
    stats->prims_tested = c[3];
    stats->ms = ms;
    stats->samples_per_pixel = r->cfg.mode != RT_MODE_SCENE ? 1u
                               : a.accum ? a.spp * r->frames_accum : a.spp;
    return queue_report(r);
}

}  // namespace

int rtamd::do_render(rt_renderer* r, FrameArgs& a, void* stream, rt_stats* stats) {
    hipStream_t st = stream ? static_cast<hipStream_t>(stream) : r->stream;
    const bool scene = r->cfg.mode == RT_MODE_SCENE;
    if (scene && !r->has_scene)
        return fail(r, RT_E_NOSCENE, "RT_MODE_SCENE render without rt_set_scene");
    int ost;
    if ((ost = order_after_last(r, st))) return ost;
    if ((ost = frame_counters(r, a, st))) return ost;
    if ((ost = superblock_order(r, a, st))) return ost;
    if (scene) {
        if ((ost = camera_records(r, a, st))) return ost;
        if ((ost = light_records(r, a, st))) return ost;  // (and the occluder lists)
        a.sc.prim_occ = r->occ.prim_occ();
        a.sc.occ_sp = r->occ.occ_sp();
        if (a.sc.prim_occ && !camera_in_occluder_gate(r, a)) a.sc.prim_occ = nullptr, a.sc.occ_sp = nullptr;
        if ((ost = ensure_prim_al(r, a.sc, st))) return ost;
    }
    if ((ost = poison_outputs(r, a, st))) return ost;
    a.count_work = stats ? 1u : 0u;
    if (scene) {
        if ((ost = screen_bins(r, a, st))) return ost;
    } else {
        r->bin_last_reason = RT_BINS_OFF_KERNEL;
    }
    a.test_fault_queue = r->test_fault_queue && !stats ? 1u : 0u;
    if (stats) RT_HIP(r, hipEventRecord(r->ev0, st));
    if ((ost = launch_frame(r, a, st))) return ost;
    return stats ? frame_stats(r, a, st, stats) : RT_OK;
}

int rtamd::render_tiles_one(rt_renderer* r, const uint32_t* tile_ids, uint32_t n_tiles, uint32_t ts,
                            void* dev_packed, void* stream, rt_stats* stats) {
    if (n_tiles && (!tile_ids || !dev_packed))
        return fail(r, RT_E_INVALID, "rt_render_tiles: null argument");
    int st;
    if ((st = check_tiles(r, tile_ids, n_tiles, ts))) return st;
    const uint32_t tx = (r->W + ts - 1) / ts;
    if ((st = set_device(r))) return st;
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : r->stream;
    if (n_tiles == 0) {
        if (stats) memset(stats, 0, sizeof(*stats));
        return RT_OK;
    }
    const uint32_t* dev_ids = nullptr;
    if ((st = order_after_last(r, s))) return st;
    if ((st = tile_list(r, tile_ids, n_tiles, s, &dev_ids))) return st;
    accum_pixels(r, tile_ids, n_tiles, ts);
    FrameArgs a;
    fill_frame_args(r, a);
    a.out8 = static_cast<uint32_t*>(dev_packed);
    a.out32 = nullptr;
    a.tiles = dev_ids;
    a.n_tiles = n_tiles;
    a.tile_size = ts;
    a.tiles_x = tx;
    st = do_render(r, a, s, stats);
    if (!st && stats && r->cfg.mode != RT_MODE_SCENE) {
        uint64_t px = 0;
        for (uint32_t i = 0; i < n_tiles; ++i) {
            const uint32_t x0 = (tile_ids[i] % tx) * ts, y0 = (tile_ids[i] / tx) * ts;
            const uint64_t w = std::min<uint64_t>(ts, r->W - x0), h = std::min<uint64_t>(ts, r->H - y0);
            px += w * h;
        }
        stats->primary_rays = px;
    }
    return st;
}

int rtamd::unpack_tiles_one(rt_renderer* r, const void* dev_packed, const uint32_t* tile_ids,
                            uint32_t n_tiles, uint32_t ts, void* dev_rgba8, void* stream) {
    if (n_tiles && (!tile_ids || !dev_packed)) return fail(r, RT_E_INVALID, "rt_unpack_tiles: null argument");
    int st;
    if ((st = check_tiles(r, tile_ids, n_tiles, ts, /*allow_skip=*/true))) return st;
    if (n_tiles == 0) return RT_OK;
    const uint32_t tx = (r->W + ts - 1) / ts;
    if ((st = set_device(r))) return st;
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : r->stream;
    const uint32_t* dev_ids = nullptr;
    if ((st = order_after_last(r, s))) return st;
    if ((st = tile_list(r, tile_ids, n_tiles, s, &dev_ids))) return st;
    hipError_t e = launch_unpack(static_cast<const uint32_t*>(dev_packed), dev_ids, n_tiles, ts, tx,
                                 r->W, r->H, dev_rgba8 ? static_cast<uint32_t*>(dev_rgba8) : r->fb.p, s);
    if (e != hipSuccess) return hip_fail(r, e, "rt_unpack_tiles");
    return mark_queued(r, s);
}

namespace {

// The query path's own stat lines (rt_trace_rays, rt_render_gbuffer: a stats
// launch never touches the frames' counter sets): zeroed on `hs` with the
// start event behind them; after the launch and the end event, read back into
// `stats` (nodes, tests and ms; the caller adds its ray count).
int query_stats_begin(rt_renderer* r, hipStream_t hs, unsigned long long*& ctr) {
    int st;
    if ((st = ensure(r, r->q_counters, kStatLineWords))) return st;
    ctr = r->q_counters.p;
    RT_HIP(r, hipMemsetAsync(ctr, 0, kStatLineWords * sizeof(unsigned long long), hs));
    RT_HIP(r, hipEventRecord(r->ev0, hs));
    return RT_OK;
}
int query_stats_read(rt_renderer* r, const unsigned long long* ctr, rt_stats* stats) {
    RT_HIP(r, hipEventSynchronize(r->ev1));
    unsigned long long lines[kStatLineWords], c[4];
    RT_HIP(r, hipMemcpy(lines, ctr, sizeof(lines), hipMemcpyDeviceToHost));
    sum_stat_lines(lines, c);
    float ms = 0.f;
    RT_HIP(r, hipEventElapsedTime(&ms, r->ev0, r->ev1));
    memset(stats, 0, sizeof(*stats));
    stats->nodes_visited = c[2];
    stats->prims_tested = c[3];
    stats->ms = ms;
    return RT_OK;
}

// rt_pick's ray through image coordinates (u, v): tmin = 0, tmax = +inf.
void pick_ray(const rt_renderer* r, float u, float v, float4 ray[2]) {
    // Camera::getRay (include/camera.h:24-41) in source order on the host (built
    // with -ffp-contract=off, IEEE division and sqrt): the same bits as the CPU oracle's getRay
    const float* K = r->K;
    const float* P = r->pose;
    const float dx = (u - K[2]) / K[0];
    const float dy = (v - K[5]) / K[4];
    const float dz = 1.0f;
    float wx = P[0] * dx + P[4] * dy + P[8] * dz;
    float wy = P[1] * dx + P[5] * dy + P[9] * dz;
    float wz = P[2] * dx + P[6] * dy + P[10] * dz;
    const float len = sqrtf(wx * wx + wy * wy + wz * wz);
    wx /= len;
    wy /= len;
    wz /= len;
    ray[0] = make_float4(P[12], P[13], P[14], 0.0f);
    ray[1] = make_float4(wx, wy, wz, INFINITY);
}

}  // namespace

extern "C" {

int rt_get_bin_info(rt_renderer* r, rt_bin_info* info) {
    if (!r || !info) return fail(r, RT_E_INVALID, "rt_get_bin_info: null argument");
    if (const int st = rt_synchronize(r)) return st;
    memset(info, 0, sizeof(*info));
    info->bin_size = kBinSide;
    info->reason = r->bin_last_reason;
    if (r->bin_last_reason == RT_BINS_ON) {
        const uint32_t* m = r->bin_mirror;
        if (m[kBinInfoFrame] != r->bin_last_frame)
            return fail(r, RT_E_STATE, "rt_get_bin_info: the last frame's bin words never arrived");
        const uint32_t flag = m[kBinInfoFlag];
        info->reason = flag & kBinFlagCapacity ? RT_BINS_OFF_CAPACITY
                       : flag & kBinFlagWide   ? RT_BINS_OFF_WIDE
                       : flag & kBinFlagDense  ? RT_BINS_OFF_DENSE
                                               : RT_BINS_ON;
        info->bins = r->bin_nbx * r->bin_nby;
        info->entries = m[kBinInfoEntries];
        info->capacity = r->bin_last_capacity;
        info->non_empty_bins = m[kBinInfoNonEmpty];
        info->longest = m[kBinInfoLongest];
        info->overflowed_bins = m[kBinInfoOver];
        info->wide = m[kBinInfoWide];
        if (r->bin_timed) (void)hipEventElapsedTime(&info->bin_build_ms, r->bin_e0, r->bin_e1);
    }
    info->enabled = info->reason == RT_BINS_ON ? 1u : 0u;
    r->bin_timing = true;  // frames record the build's events from now on
    return RT_OK;
}

int rt_export_bins(rt_renderer* r, uint32_t* headers_out, uint32_t* indices_out, uint32_t* wide_out) {
    rt_bin_info bi;
    if (const int st = rt_get_bin_info(r, &bi)) return st;
    if (!bi.enabled) return fail(r, RT_E_STATE, "rt_export_bins: the last frame built no lists");
    if (headers_out && bi.bins)
        RT_HIP(r, hipMemcpy(headers_out, r->bin_hdr.p, bi.bins * sizeof(uint2), hipMemcpyDeviceToHost));
    std::vector<BinEntry> ent(std::max(bi.entries, bi.wide));
    if (indices_out && bi.entries) {
        RT_HIP(r, hipMemcpy(ent.data(), r->bin_ent.p, bi.entries * sizeof(BinEntry), hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < bi.entries; ++i) indices_out[i] = ent[i].idx;
    }
    if (wide_out && bi.wide) {
        RT_HIP(r, hipMemcpy(ent.data(), r->bin_wide.p, bi.wide * sizeof(BinEntry), hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < bi.wide; ++i) wide_out[i] = ent[i].idx;
    }
    return RT_OK;
}

int rt_export_bin_tiles(rt_renderer* r, uint32_t* tw, uint32_t* th, uint32_t* tiles_per_bin,
                        uint64_t* words_out) {
    rt_bin_info bi;
    if (const int st = rt_get_bin_info(r, &bi)) return st;
    if (!bi.enabled) return fail(r, RT_E_STATE, "rt_export_bin_tiles: the last frame built no lists");
    const uint32_t tpb = bin_tiles_per_bin(r->bin_tw, r->bin_th);
    if (tw) *tw = r->bin_tw;
    if (th) *th = r->bin_th;
    if (tiles_per_bin) *tiles_per_bin = tpb;
    if (words_out && bi.bins) {
        const size_t n = size_t(bi.bins) * tpb;
        RT_HIP(r, hipMemcpy(words_out, r->bin_hdr.p + bi.bins, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
        // the builder writes the words of the bins whose lists the kernel reads
        std::vector<uint2> hdr(bi.bins);
        RT_HIP(r, hipMemcpy(hdr.data(), r->bin_hdr.p, bi.bins * sizeof(uint2), hipMemcpyDeviceToHost));
        for (uint32_t b = 0; b < bi.bins; ++b)
            if (hdr[b].y == 0u || hdr[b].y == kBinWalk)
                for (uint32_t t = 0; t < tpb; ++t) words_out[size_t(b) * tpb + t] = 0;
    }
    return RT_OK;
}

int rt_render_tiles(rt_renderer* r, const uint32_t* tile_ids, uint32_t n_tiles, uint32_t ts,
                    void* dev_packed, void* stream, rt_stats* stats) {
    if (!r) return fail(r, RT_E_INVALID, "rt_render_tiles: null handle");
    if (r->multi)
        return fail(r, RT_E_STATE, "rt_render_tiles: a multi-device handle renders whole frames");
    return render_tiles_one(r, tile_ids, n_tiles, ts, dev_packed, stream, stats);
}

int rt_unpack_tiles(rt_renderer* r, const void* dev_packed, const uint32_t* tile_ids,
                    uint32_t n_tiles, uint32_t ts, void* dev_rgba8, void* stream) {
    if (!r) return fail(r, RT_E_INVALID, "rt_unpack_tiles: null handle");
    if (r->multi)
        return fail(r, RT_E_STATE, "rt_unpack_tiles: a multi-device handle renders whole frames");
    return unpack_tiles_one(r, dev_packed, tile_ids, n_tiles, ts, dev_rgba8, stream);
}

// Ray queries (the reference has none: Octree::traverse is a stub,
// include/octree.h:19-21).  A query reads scene state only: it takes no frame
// id, leaves the progressive sums, the frames' counter sets and the qerr word
// alone, and is ordered after the handle's earlier work like every launch.
int rt_trace_rays(rt_renderer* r, const void* dev_rays, uint32_t n, uint32_t kind, void* dev_hits,
                  void* stream, rt_stats* stats) {
    if (!r) return fail(r, RT_E_INVALID, "rt_trace_rays: null handle");
    if (kind != RT_QUERY_NEAREST && kind != RT_QUERY_ANY)
        return fail(r, RT_E_INVALID, "rt_trace_rays: unknown query kind");
    if (!r->has_scene) return fail(r, RT_E_NOSCENE, "rt_trace_rays: no scene (rt_set_scene first)");
    if (n == 0) {
        if (stats) memset(stats, 0, sizeof(*stats));
        return RT_OK;
    }
    if (!dev_rays || !dev_hits) return fail(r, RT_E_INVALID, "rt_trace_rays: null buffer");
    int st;
    if ((st = set_device(r))) return st;
    hipStream_t hs = stream ? static_cast<hipStream_t>(stream) : own_stream(r);
    if ((st = order_after_last(r, hs))) return st;
    // the kernel's leading argument is a FrameArgs (rt_query.hip): the scene, the rest zero
    FrameArgs a;
    memset(&a, 0, sizeof(a));
    a.sc = r->sc;
    unsigned long long* ctr = nullptr;
    if (stats && (st = query_stats_begin(r, hs, ctr))) return st;
    hipError_t e = launch_query(a, dev_rays, dev_hits, n, kind == RT_QUERY_ANY, ctr, hs);
    if (e != hipSuccess) return hip_fail(r, e, "rt_trace_rays: kernel launch");
    if (stats) RT_HIP(r, hipEventRecord(r->ev1, hs));
    if ((st = mark_queued(r, hs))) return st;
    if (stats) {
        if ((st = query_stats_read(r, ctr, stats))) return st;
        (kind == RT_QUERY_ANY ? stats->shadow_rays : stats->primary_rays) = n;
    }
    return RT_OK;
}

int rt_pick(rt_renderer* r, float u, float v, rt_hit* hit_out, float point_out[3]) {
    if (!r || !hit_out) return fail(r, RT_E_INVALID, "rt_pick: null argument");
    if (!r->has_scene) return fail(r, RT_E_NOSCENE, "rt_pick: no scene (rt_set_scene first)");
    float4 ray[2];
    pick_ray(r, u, v, ray);
    int st;
    if ((st = set_device(r))) return st;
    if ((st = ensure(r, r->q_ray, 2)) || (st = ensure(r, r->q_hit, 1))) return st;
    hipStream_t hs = own_stream(r);
    if ((st = order_after_last(r, hs))) return st;
    RT_HIP(r, hipMemcpyAsync(r->q_ray.p, ray, sizeof(ray), hipMemcpyHostToDevice, hs));
    if ((st = rt_trace_rays(r, r->q_ray.p, 1, RT_QUERY_NEAREST, r->q_hit.p, hs, nullptr))) return st;
    uint2 h;
    RT_HIP(r, hipMemcpyAsync(&h, r->q_hit.p, sizeof(h), hipMemcpyDeviceToHost, hs));
    RT_HIP(r, hipStreamSynchronize(hs));
    memcpy(&hit_out->t, &h.x, sizeof(float));
    hit_out->sphere = h.y;
    if (point_out) {
        const float o[3] = {ray[0].x, ray[0].y, ray[0].z}, d[3] = {ray[1].x, ray[1].y, ray[1].z};
        for (int i = 0; i < 3; ++i) point_out[i] = o[i] + hit_out->t * d[i];
    }
    return RT_OK;
}

// Ordered multi-hit queries: the k nearest spheres of each ray
// by (t, sphere index).  A query like rt_trace_rays: scene state only, the
// query path's own stat lines, the same stream ordering.
int rt_trace_rays_multi(rt_renderer* r, const void* dev_rays, uint32_t n, uint32_t k, void* dev_hits,
                        void* dev_counts, void* stream, rt_stats* stats) {
    if (!r) return fail(r, RT_E_INVALID, "rt_trace_rays_multi: null handle");
    if (k == 0 || k > RT_MULTIHIT_MAX)
        return fail(r, RT_E_INVALID, "rt_trace_rays_multi: k must be 1 .. RT_MULTIHIT_MAX");
    if (!r->has_scene)
        return fail(r, RT_E_NOSCENE, "rt_trace_rays_multi: no scene (rt_set_scene first)");
    if (n == 0) {
        if (stats) memset(stats, 0, sizeof(*stats));
        return RT_OK;
    }
    if (!dev_rays || !dev_hits) return fail(r, RT_E_INVALID, "rt_trace_rays_multi: null buffer");
    int st;
    if ((st = set_device(r))) return st;
    hipStream_t hs = stream ? static_cast<hipStream_t>(stream) : own_stream(r);
    if ((st = order_after_last(r, hs))) return st;
    // the kernel's leading argument is a FrameArgs (rt_multihit.hip): the scene, the rest zero
    FrameArgs a;
    memset(&a, 0, sizeof(a));
    a.sc = r->sc;
    unsigned long long* ctr = nullptr;
    if (stats && (st = query_stats_begin(r, hs, ctr))) return st;
    hipError_t e = launch_multihit(a, dev_rays, dev_hits, dev_counts, n, k, ctr, hs);
    if (e != hipSuccess) return hip_fail(r, e, "rt_trace_rays_multi: kernel launch");
    if (stats) RT_HIP(r, hipEventRecord(r->ev1, hs));
    if ((st = mark_queued(r, hs))) return st;
    if (stats) {
        if ((st = query_stats_read(r, ctr, stats))) return st;
        stats->primary_rays = n;
    }
    return RT_OK;
}

int rt_pick_multi(rt_renderer* r, float u, float v, uint32_t k, rt_hit* hits_out, uint32_t* count_out) {
    if (!r || !hits_out) return fail(r, RT_E_INVALID, "rt_pick_multi: null argument");
    if (k == 0 || k > RT_MULTIHIT_MAX)
        return fail(r, RT_E_INVALID, "rt_pick_multi: k must be 1 .. RT_MULTIHIT_MAX");
    if (!r->has_scene) return fail(r, RT_E_NOSCENE, "rt_pick_multi: no scene (rt_set_scene first)");
    float4 ray[2];
    pick_ray(r, u, v, ray);
    int st;
    if ((st = set_device(r))) return st;
    if ((st = ensure(r, r->q_ray, 2)) || (st = ensure(r, r->q_multi_hits, RT_MULTIHIT_MAX)) ||
        (st = ensure(r, r->q_multi_count, 1)))
        return st;
    hipStream_t hs = own_stream(r);
    if ((st = order_after_last(r, hs))) return st;
    RT_HIP(r, hipMemcpyAsync(r->q_ray.p, ray, sizeof(ray), hipMemcpyHostToDevice, hs));
    if ((st = rt_trace_rays_multi(r, r->q_ray.p, 1, k, r->q_multi_hits.p, r->q_multi_count.p, hs, nullptr)))
        return st;
    uint2 h[RT_MULTIHIT_MAX];
    uint32_t count = 0;
    RT_HIP(r, hipMemcpyAsync(h, r->q_multi_hits.p, k * sizeof(uint2), hipMemcpyDeviceToHost, hs));
    RT_HIP(r, hipMemcpyAsync(&count, r->q_multi_count.p, sizeof(count), hipMemcpyDeviceToHost, hs));
    RT_HIP(r, hipStreamSynchronize(hs));
    for (uint32_t s = 0; s < k; ++s) {
        memcpy(&hits_out[s].t, &h[s].x, sizeof(float));
        hits_out[s].sphere = h[s].y;
    }
    if (count_out) *count_out = count;
    return RT_OK;
}

// Sphere-overlap queries: the scene spheres each probe sphere
// touches, the k smallest indices.  A query like rt_trace_rays: scene state
// only, the query path's own stat lines, the same stream ordering.
int rt_query_overlaps(rt_renderer* r, const void* dev_probes, uint32_t n, uint32_t k, uint32_t flags,
                      void* dev_indices, void* dev_counts, void* stream, rt_stats* stats) {
    if (!r) return fail(r, RT_E_INVALID, "rt_query_overlaps: null handle");
    if (k == 0 || k > RT_OVERLAP_MAX)
        return fail(r, RT_E_INVALID, "rt_query_overlaps: k must be 1 .. RT_OVERLAP_MAX");
    if (flags & ~static_cast<uint32_t>(RT_OVERLAP_SKIP_SELF))
        return fail(r, RT_E_INVALID, "rt_query_overlaps: unknown flag bits");
    if (n > 0 && (!dev_probes || !dev_indices))
        return fail(r, RT_E_INVALID, "rt_query_overlaps: null buffer");
    if (!r->has_scene) return fail(r, RT_E_NOSCENE, "rt_query_overlaps: no scene (rt_set_scene first)");
    if (n == 0) {
        if (stats) memset(stats, 0, sizeof(*stats));
        return RT_OK;
    }
    int st;
    if ((st = set_device(r))) return st;
    hipStream_t hs = stream ? static_cast<hipStream_t>(stream) : own_stream(r);
    if ((st = order_after_last(r, hs))) return st;
    // the kernel's leading argument is a FrameArgs (rt_overlap.hip): the scene, the rest zero
    FrameArgs a;
    memset(&a, 0, sizeof(a));
    a.sc = r->sc;
    const float slack_m = overlap_slack_m(r->info.root_min, r->info.root_max);
    unsigned long long* ctr = nullptr;
    if (stats && (st = query_stats_begin(r, hs, ctr))) return st;
    hipError_t e = launch_overlap(a, dev_probes, dev_indices, dev_counts, n, k,
                                  (flags & RT_OVERLAP_SKIP_SELF) != 0, slack_m, ctr, hs);
    if (e != hipSuccess) return hip_fail(r, e, "rt_query_overlaps: kernel launch");
    if (stats) RT_HIP(r, hipEventRecord(r->ev1, hs));
    if ((st = mark_queued(r, hs))) return st;
    if (stats && (st = query_stats_read(r, ctr, stats))) return st;  // (no rays: both ray counts 0)
    return RT_OK;
}

int rt_overlaps_at(rt_renderer* r, const float center[3], float radius, uint32_t k,
                   uint32_t* indices_out, uint32_t* count_out) {
    if (!r || !center || !indices_out) return fail(r, RT_E_INVALID, "rt_overlaps_at: null argument");
    if (k == 0 || k > RT_OVERLAP_MAX)
        return fail(r, RT_E_INVALID, "rt_overlaps_at: k must be 1 .. RT_OVERLAP_MAX");
    if (!r->has_scene) return fail(r, RT_E_NOSCENE, "rt_overlaps_at: no scene (rt_set_scene first)");
    const float4 probe = make_float4(center[0], center[1], center[2], radius);
    int st;
    if ((st = set_device(r))) return st;
    if ((st = ensure(r, r->q_probe, 1)) || (st = ensure(r, r->q_overlap_idx, RT_OVERLAP_MAX)) ||
        (st = ensure(r, r->q_overlap_count, 1)))
        return st;
    hipStream_t hs = own_stream(r);
    if ((st = order_after_last(r, hs))) return st;
    RT_HIP(r, hipMemcpyAsync(r->q_probe.p, &probe, sizeof(probe), hipMemcpyHostToDevice, hs));
    if ((st = rt_query_overlaps(r, r->q_probe.p, 1, k, 0, r->q_overlap_idx.p, r->q_overlap_count.p, hs,
                                nullptr)))
        return st;
    uint32_t idx[RT_OVERLAP_MAX], count = 0;
    RT_HIP(r, hipMemcpyAsync(idx, r->q_overlap_idx.p, k * sizeof(uint32_t), hipMemcpyDeviceToHost, hs));
    RT_HIP(r, hipMemcpyAsync(&count, r->q_overlap_count.p, sizeof(count), hipMemcpyDeviceToHost, hs));
    RT_HIP(r, hipStreamSynchronize(hs));
    memcpy(indices_out, idx, k * sizeof(uint32_t));
    if (count_out) *count_out = count;
    return RT_OK;
}

// First-hit G-buffer (the reference writes one colour per pixel,
// src/renderer.cu:57-82).  Like a query it reads scene and camera state only:
// no frame id, no fill_frame_args (which advances both), the query path's own
// stat lines, nothing of the frames' counter sets, sums or framebuffer.
int rt_render_gbuffer(rt_renderer* r, const rt_gbuffer* out, void* stream, rt_stats* stats) {
    if (!r) return fail(r, RT_E_INVALID, "rt_render_gbuffer: null handle");
    if (!out || (!out->dev_hits && !out->dev_normals && !out->dev_albedo))
        return fail(r, RT_E_INVALID, "rt_render_gbuffer: no output buffer");
    if (!r->has_scene) return fail(r, RT_E_NOSCENE, "rt_render_gbuffer: no scene (rt_set_scene first)");
    int st;
    if ((st = set_device(r))) return st;
    hipStream_t hs = stream ? static_cast<hipStream_t>(stream) : own_stream(r);
    if ((st = order_after_last(r, hs))) return st;
    // the kernel's leading argument is a FrameArgs (rt_gbuffer.hip): camera,
    // scene and size, the rest zero
    FrameArgs a;
    memset(&a, 0, sizeof(a));
    fill_camera(r, a.cam);
    a.sc = r->sc;
    a.W = r->W;
    a.H = r->H;
    // the frames' own table: whichever of the two runs first makes it
    if (out->dev_albedo && (st = ensure_prim_al(r, a.sc, hs))) return st;
    unsigned long long* ctr = nullptr;
    if (stats && (st = query_stats_begin(r, hs, ctr))) return st;
    hipError_t e = launch_gbuffer(a, out->dev_hits, out->dev_normals, out->dev_albedo, ctr, hs);
    if (e != hipSuccess) return hip_fail(r, e, "rt_render_gbuffer: kernel launch");
    if (stats) RT_HIP(r, hipEventRecord(r->ev1, hs));
    if ((st = mark_queued(r, hs))) return st;
    if (stats) {
        if ((st = query_stats_read(r, ctr, stats))) return st;
        stats->primary_rays = static_cast<uint64_t>(r->W) * r->H;
    }
    return RT_OK;
}

}  // extern "C"
