// rt_bins_host.cpp — the host side of the screen-space bins (screen_bins.hip,
// DESIGN.md 5.1 round 10): do_render's step that builds a frame's bins, and
// the calls that report and export them.  When a frame builds and how large
// its entry buffer is are rt_bins_math.h's policy functions.
#include "rt_frame_math.h"
#include "rt_host.h"

using namespace rtamd;

namespace {

// Whether this frame builds bins; bins.last_reason says why not.
bool bins_gate(rt_renderer* r, const FrameArgs& a, const FramePlan& plan) {
    ScreenBinState& s = r->bins;
    if (r->cfg.flags & RT_FLAG_NO_BINS) return s.last_reason = RT_BINS_OFF_FLAG, false;
    // (the scene_kernel_w8 instances read bins: plain frames of the wave queue)
    if (a.count_work || !plan.inst.w8() ||
        static_cast<uint64_t>(a.W) * a.H * a.spp < s.min_samples)
        return s.last_reason = RT_BINS_OFF_KERNEL, false;
    float B[9];
    if (!bins_camera_ok(a.cam.K, a.cam.R, a.cam.o) || !cam8_basis(a.cam.K, a.cam.R, a.W, a.H, B))
        return s.last_reason = RT_BINS_OFF_CAMERA, false;
    // a scene the device rule found too dense: probe once in kBinDenseSkip + 1 frames
    if (bin_dense_skip_step(s.cadence, r->scene_gen, s.mirror[kBinInfoFrame], s.mirror[kBinInfoFlag]))
        return s.last_reason = RT_BINS_OFF_DENSE, false;
    return true;
}

// The per-scene first references and every buffer of an nbx x nby build.  The
// sizes are fixed here; a frame whose entries do not fit sets its device flag
// and walks, the flag lands in the pinned words, and the next frame that sees
// it grows the entry buffer.
int bins_buffers(rt_renderer* r, const FrameArgs& a, uint32_t nb, hipStream_t st) {
    ScreenBinState& s = r->bins;
    int ost;
    bool stale;
    if ((ost = s.first_ref.query(r, std::max(1u, r->n_spheres), r->scene_gen, nullptr, 0, &stale))) return ost;
    if (stale) {
        hipError_t e = launch_first_refs(a.sc.prim_sp, a.sc.prim_idx, r->prim_slots, r->d_spheres.p,
                                         r->n_spheres, s.first_ref.buf.p, st);
        if (e != hipSuccess) return hip_fail(r, e, "screen bins (first references)");
        s.first_ref.commit(r->scene_gen, nullptr, 0);
    }
    const size_t want = bin_entries_wanted(s.capacity_test, r->n_spheres, s.mirror[kBinInfoFrame],
                                           s.mirror[kBinInfoFlag], s.mirror[kBinInfoEntries],
                                           s.cadence.last_frame, s.ent.n);
    if (s.ent.n < 2 * want) {
        // (the buffer may still be read by a frame in flight on another stream)
        if (s.ent.p) RT_HIP(r, hipDeviceSynchronize());
        if ((ost = ensure(r, s.ent, 2 * want))) return ost;
    }
    if ((ost = ensure(r, s.rects, std::max(1u, r->n_spheres))) ||
        (ost = ensure(r, s.cnt, bin_zeroed_words(nb))) || (ost = ensure(r, s.offs, nb + 1ull)) ||
        (ost = ensure(r, s.hdr, size_t(nb) * (1u + kBinCap))) ||  // (and the tile words)
        (ost = ensure(r, s.wide, 2ull * kBinWideCap)))
        return ost;
    if (s.temp_items < nb + 1u || !s.temp.p) {
        const size_t bytes = bins_scan_temp_bytes(nb + 1u);
        if (!bytes) return fail(r, RT_E_HIP, "screen bins: scan scratch size");
        if ((ost = ensure(r, s.temp, bytes))) return ost;
        s.temp_items = nb + 1u;
    }
    return RT_OK;
}

// The build's arguments: the scene, the frame's camera and wave tile, the buffers.
BinBuild bins_build_args(const rt_renderer* r, const FrameArgs& a, const FramePlan& plan, uint32_t nbx,
                         uint32_t nby) {
    const ScreenBinState& s = r->bins;
    const uint32_t nb = nbx * nby;
    BinBuild b{};
    b.spheres = r->d_spheres.p;
    b.first_ref = s.first_ref.buf.p;
    b.n_spheres = r->n_spheres;
    memcpy(b.K, a.cam.K, sizeof(b.K));
    memcpy(b.R, a.cam.R, sizeof(b.R));
    memcpy(b.o, a.cam.o, sizeof(b.o));
    b.W = a.W;
    b.H = a.H;
    b.nbx = nbx;
    b.nby = nby;
    b.tw = plan.grid.tw;
    b.th = plan.grid.th;
    b.shrink = s.shrink;
    b.capacity = static_cast<uint32_t>(s.ent.n / 2);
    b.cap = s.cap;
    b.mean_max = s.mean_max;
    b.frame_id = a.frame_id;
    b.rects = s.rects.p;
    b.counts = s.cnt.p;
    b.cursor = s.cnt.p + bin_cursor_at(nb);
    b.decide = s.cnt.p + bin_decide_at(nb);
    b.info = s.cnt.p + bin_info_at(nb);
    b.offs = s.offs.p;
    b.hdr = s.hdr.p;
    b.ent = s.ent.p;
    b.tiles = reinterpret_cast<unsigned long long*>(s.hdr.p + nb);
    b.wide = s.wide.p;
    b.mirror = s.mirror_dev;
    b.temp = s.temp.p;
    b.temp_bytes = s.temp.n;
    return b;
}

// The build on `st` between its timing events, what the renderer remembers of
// it, and the frame kernel's view of the result.
int bins_launch(rt_renderer* r, FrameArgs& a, const BinBuild& b, hipStream_t st) {
    ScreenBinState& s = r->bins;
    if (s.timing) RT_HIP(r, hipEventRecord(s.e0, st));
    hipError_t e = launch_screen_bins(b, st);
    if (e != hipSuccess) return hip_fail(r, e, "screen bins");
    if (s.timing) {
        RT_HIP(r, hipEventRecord(s.e1, st));
        s.timed = true;
    }
    s.last_reason = RT_BINS_ON;  // (the device flag may still send the frame walking: rt_get_bin_info)
    s.cadence.last_frame = a.frame_id;
    s.last_capacity = b.capacity;
    s.nbx = b.nbx;
    s.nby = b.nby;
    s.tw = b.tw;
    s.th = b.th;
    a.bin_hdr = s.hdr.p;
    a.bin_ent = s.ent.p;
    a.bin_nb = b.nbx * b.nby;
    a.bin_wide = s.wide.p;
    a.bin_info = b.info;
    a.bin_nbx = b.nbx;
    return RT_OK;
}

}  // namespace

// do_render's step 4b: this frame's screen-space bins, queued on `st` ahead of
// the frame kernel: built by every plain frame whose kernel reads them, never
// keyed on the pose (the Displayer's camera moves every frame), with no wait
// and no readback.
int rtamd::screen_bins(rt_renderer* r, FrameArgs& a, const FramePlan& plan, hipStream_t st) {
    a.bin_hdr = nullptr;
    a.bin_ent = nullptr;
    a.bin_nb = 0;
    a.bin_wide = nullptr;
    a.bin_info = nullptr;
    a.bin_nbx = 0;
    r->bins.timed = false;
    if (!bins_gate(r, a, plan)) return RT_OK;
    const uint32_t nbx = (a.W + kBinSide - 1u) / kBinSide, nby = (a.H + kBinSide - 1u) / kBinSide;
    if (const int ost = bins_buffers(r, a, nbx * nby, st)) return ost;
    return bins_launch(r, a, bins_build_args(r, a, plan, nbx, nby), st);
}

extern "C" {

int rt_get_bin_info(rt_renderer* r, rt_bin_info* info) {
    if (!r || !info) return fail(r, RT_E_INVALID, "rt_get_bin_info: null argument");
    if (const int st = rt_synchronize(r)) return st;
    const ScreenBinState& s = r->bins;
    memset(info, 0, sizeof(*info));
    info->bin_size = kBinSide;
    info->reason = s.last_reason;
    if (s.last_reason == RT_BINS_ON) {
        const uint32_t* m = s.mirror;
        if (m[kBinInfoFrame] != s.cadence.last_frame)
            return fail(r, RT_E_STATE, "rt_get_bin_info: the last frame's bin words never arrived");
        const uint32_t flag = m[kBinInfoFlag];
        info->reason = flag & kBinFlagCapacity ? RT_BINS_OFF_CAPACITY
                       : flag & kBinFlagWide   ? RT_BINS_OFF_WIDE
                       : flag & kBinFlagDense  ? RT_BINS_OFF_DENSE
                                               : RT_BINS_ON;
        info->bins = s.nbx * s.nby;
        info->entries = m[kBinInfoEntries];
        info->capacity = s.last_capacity;
        info->non_empty_bins = m[kBinInfoNonEmpty];
        info->longest = m[kBinInfoLongest];
        info->overflowed_bins = m[kBinInfoOver];
        info->wide = m[kBinInfoWide];
        if (s.timed) (void)hipEventElapsedTime(&info->bin_build_ms, s.e0, s.e1);
    }
    info->enabled = info->reason == RT_BINS_ON ? 1u : 0u;
    r->bins.timing = true;  // frames record the build's events from now on
    return RT_OK;
}

int rt_export_bins(rt_renderer* r, uint32_t* headers_out, uint32_t* indices_out, uint32_t* wide_out) {
    rt_bin_info bi;
    if (const int st = rt_get_bin_info(r, &bi)) return st;
    if (!bi.enabled) return fail(r, RT_E_STATE, "rt_export_bins: the last frame built no lists");
    if (headers_out && bi.bins)
        RT_HIP(r, hipMemcpy(headers_out, r->bins.hdr.p, bi.bins * sizeof(uint2), hipMemcpyDeviceToHost));
    std::vector<BinEntry> ent(std::max(bi.entries, bi.wide));
    if (indices_out && bi.entries) {
        RT_HIP(r, hipMemcpy(ent.data(), r->bins.ent.p, bi.entries * sizeof(BinEntry), hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < bi.entries; ++i) indices_out[i] = ent[i].idx;
    }
    if (wide_out && bi.wide) {
        RT_HIP(r, hipMemcpy(ent.data(), r->bins.wide.p, bi.wide * sizeof(BinEntry), hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < bi.wide; ++i) wide_out[i] = ent[i].idx;
    }
    return RT_OK;
}

int rt_export_bin_tiles(rt_renderer* r, uint32_t* tw, uint32_t* th, uint32_t* tiles_per_bin,
                        uint64_t* words_out) {
    rt_bin_info bi;
    if (const int st = rt_get_bin_info(r, &bi)) return st;
    if (!bi.enabled) return fail(r, RT_E_STATE, "rt_export_bin_tiles: the last frame built no lists");
    const ScreenBinState& s = r->bins;
    const uint32_t tpb = bin_tiles_per_bin(s.tw, s.th);
    if (tw) *tw = s.tw;
    if (th) *th = s.th;
    if (tiles_per_bin) *tiles_per_bin = tpb;
    if (words_out && bi.bins) {
        const size_t n = size_t(bi.bins) * tpb;
        RT_HIP(r, hipMemcpy(words_out, s.hdr.p + bi.bins, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
        // the builder writes the words of the bins whose lists the kernel reads
        std::vector<uint2> hdr(bi.bins);
        RT_HIP(r, hipMemcpy(hdr.data(), s.hdr.p, bi.bins * sizeof(uint2), hipMemcpyDeviceToHost));
        for (uint32_t b = 0; b < bi.bins; ++b)
            if (hdr[b].y == 0u || hdr[b].y == kBinWalk)
                for (uint32_t t = 0; t < tpb; ++t) words_out[size_t(b) * tpb + t] = 0;
    }
    return RT_OK;
}

}  // extern "C"
