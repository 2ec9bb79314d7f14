// rt_frame.cpp — what a renderer queues per frame: its preparation and launch
// (do_render and its steps; the screen-bin step is rt_bins_host.cpp's) and
// tile frames.  The arithmetic the images depend on is rt_frame_math.h's.
#include "rt_frame_math.h"
#include "rt_host.h"

using namespace rtamd;

namespace rtamd {

// The handle's shading as a kernel reads it (the frames, and the one-bounce layer
// that shades its hits like them): the unit vector toward the light, the ambient
// term and whether lit hits cast a shadow ray.
void fill_shading(const rt_renderer* r, FrameArgs& a) {
    a.shadows = (r->cfg.flags & RT_FLAG_NO_SHADOWS) ? 0u : 1u;
    const float* ld = r->cfg.light_dir;
    const float ll = sqrtf(ld[0] * ld[0] + ld[1] * ld[1] + ld[2] * ld[2]);
    a.L[0] = -(ld[0] / ll);
    a.L[1] = -(ld[1] / ll);
    a.L[2] = -(ld[2] / ll);
    a.ambient = r->cfg.ambient;
}

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
    a.contract = (r->cfg.flags & RT_FLAG_COMPAT_FMA) ? 1u : 0u;
    fill_shading(r, a);
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
    a.sc.opt = ((r->cfg.flags >> RT_FLAG_OPT_SHIFT) & 0xFFu) | ((r->cfg.flags & RT_FLAG_NO_PAIRS) ? kOptNoPairs : 0u);
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

// ---- do_render's steps, in its order: each queues on `st` and fills its part of `a` ----

// Step 1: this frame's counter set (RendererState::ctr_set) and, for the wave
// queue, its per-XCD slot table (8 x plan->slot_stride words after the
// counters), zero when the kernel starts; the other set is the one the kernel
// zeroes for the next frame.  counters_after_launch is the other half.
// plan: a scene frame's, null for a compat frame.
int frame_counters(rt_renderer* r, FrameArgs& a, const FramePlan* plan, hipStream_t st) {
    const bool scene = plan != nullptr;
    size_t words = kCounterWords;  // one set
    a.wq_slots = nullptr;
    a.wq_slot_stride = 0;
    if (scene) {
        a.wq_slot_shift = plan->slot_shift;
        a.wq_slot_stride = plan->slot_stride;
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
int superblock_order(rt_renderer* r, FrameArgs& a, const FramePlan* plan, hipStream_t) {
    a.sb_order = nullptr;
    if (!plan || a.tiles || plan->slot_shift != 12u || !r->sb_hilbert) return RT_OK;
    const uint32_t nx = plan->grid.nsx, ny = plan->grid.nsy;  // the superblock grid of this frame
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
int launch_frame(rt_renderer* r, FrameArgs& a, const FramePlan* plan, hipStream_t st) {
    int ost;
    if ((ost = timeline_begin(r, a, st)) || (ost = block_stats_begin(r, a, st))) return ost;
    hipError_t e = plan ? launch_scene(a, *plan, st, &r->last_instance) : launch_compat(a, st);
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
    a.count_work = stats ? 1u : 0u;
    // a scene frame's plan, made once: its kernel instance, wave-tile grid,
    // slot table, LDS bytes and ticket size (rt_sched.h); the steps read it
    const FramePlan planned = plan_scene_frame(a.variant, a.spp, a.accum != nullptr, stats != nullptr,
                                               r->sort_rounds, a.sc.tab_k, a.sc.stack_depth, a.W, a.H,
                                               a.tiles ? a.n_tiles : 0u, a.tile_size, a.sc.opt);
    const FramePlan* plan = scene ? &planned : nullptr;
    int ost;
    if ((ost = order_after_last(r, st))) return ost;
    if ((ost = frame_counters(r, a, plan, st))) return ost;
    if ((ost = superblock_order(r, a, plan, st))) return ost;
    if (scene) {
        if ((ost = camera_records(r, a, st))) return ost;
        if ((ost = light_records(r, a, st))) return ost;  // (and the occluder lists)
        a.sc.prim_occ = r->occ.prim_occ();
        a.sc.occ_sp = r->occ.occ_sp();
        if (a.sc.prim_occ && !camera_in_occluder_gate(r, a)) a.sc.prim_occ = nullptr, a.sc.occ_sp = nullptr;
        if ((ost = ensure_prim_al(r, a.sc, st))) return ost;
    }
    if ((ost = poison_outputs(r, a, st))) return ost;
    if (scene) {
        if ((ost = screen_bins(r, a, *plan, st))) return ost;  // (step 4b: rt_bins_host.cpp)
    } else {
        r->bins.last_reason = RT_BINS_OFF_KERNEL;
    }
    a.test_fault_queue = r->test_fault_queue && !stats ? 1u : 0u;
    if (stats) RT_HIP(r, hipEventRecord(r->ev0, st));
    if ((ost = launch_frame(r, a, plan, st))) return ost;
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

extern "C" {

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

}  // extern "C"
