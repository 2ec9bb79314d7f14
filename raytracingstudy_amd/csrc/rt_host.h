// rt_host.h — what the host units of the C-ABI share (internal, never
// installed): the renderer's state, the error and allocation helpers, the
// stream-ordering helpers, and the functions the units call across.
//   rt_capi.cpp   handle lifetime, camera, rt_render and the display binding
//   rt_scene.cpp  scene upload, octree build, exports
//   rt_frame.cpp  per-frame preparation and launch (do_render's steps: it plans a
//                 scene frame once, FramePlan, and hands the plan to them), tiles
//   rt_bins_host.cpp  do_render's screen-bin step, the bin exports
//   rt_queries.cpp    ray, multi-hit, overlap, closest-sphere and swept-sphere queries, picking, the G-buffer,
//                     the AO layer, the one-bounce layer, the layer filter, the layer multiply, the layer add and
//                     the layer reprojection
//   rt_multi.cpp  the multi-device handle and its RCCL loader
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <vector>

#include "../../include/rt.h"
#include "octree_gpu.h"
#include "rt_bins_math.h"
#include "rt_closest_math.h"
#include "rt_overlap_math.h"
#include "rt_params.h"
#include "rt_reproject_math.h"
#include "rt_sweep_math.h"
#include "scene_build.h"

struct ncclComm;  // <rccl/rccl.h>'s ncclComm_t is a pointer to it; only rt_multi.cpp includes that

namespace rtamd {

// the kernels' launchers
// rt_kernels.hip: a scene frame as do_render planned it (plan_scene_frame, rt_sched.h)
// (instance: the launched instance's Frame<> switches, rt_last_instance)
hipError_t launch_scene(const FrameArgs& a, const FramePlan& plan, hipStream_t st, uint32_t* instance);
bool variant_available(uint32_t v);
// rt_compat.hip: the reference's frame restated; packed tiles scattered into the frame
hipError_t launch_compat(const FrameArgs& a, hipStream_t st);
hipError_t launch_unpack(const uint32_t* packed, const uint32_t* tiles, uint32_t n_tiles,
                         uint32_t ts, uint32_t tiles_x, uint32_t W, uint32_t H, uint32_t* img,
                         hipStream_t st);
// rt_records.hip: the per-reference records
hipError_t launch_cam_screen(const float4* prim_sp, uint32_t n, const float o[3], float4* out,
                             hipStream_t st);
hipError_t launch_shd_screen(const float4* prim_sp, uint32_t n, const float e[6], double delta,
                             float2* out8, uint32_t* rr_max, hipStream_t st);
hipError_t launch_albedo_refs(const uint32_t* prim_idx, const uint32_t* albedo, uint32_t n,
                              uint32_t n_spheres, uint32_t* out, hipStream_t st);
hipError_t launch_cam8_screen(const float4* prim_sp, uint32_t n, const float o[3], const float B[9],
                              uint32_t ok, float2* out, hipStream_t st);
// rt_query.hip: n rays (rt_ray) -> n hits (rt_hit) against a.sc; counters != null: a stats launch
hipError_t launch_query(const FrameArgs& a, const void* rays, void* hits, uint32_t n, bool any,
                        unsigned long long* counters, hipStream_t st);
// rt_multihit.hip: n rays -> n x k hits (ray-major, the k nearest by (t, sphere index)) and n
// counts (may be null) against a.sc; 1 <= k <= RT_MULTIHIT_MAX; counters != null: a stats launch
hipError_t launch_multihit(const FrameArgs& a, const void* rays, void* hits, void* counts, uint32_t n,
                           uint32_t k, unsigned long long* counters, hipStream_t st);
// rt_overlap.hip: n probes (rt_probe) -> n x k sphere indices (probe-major, the k smallest of each
// probe's accepted set, ascending) and n count words (may be null) against a.sc; 1 <= k <=
// RT_OVERLAP_MAX; slack_m: overlap_slack_m of the root box; counters != null: a stats launch
hipError_t launch_overlap(const FrameArgs& a, const void* probes, void* indices, void* counts,
                          uint32_t n, uint32_t k, bool skip_self, float slack_m,
                          unsigned long long* counters, hipStream_t st);
// rt_closest.hip: n probes (rt_probe: a point and its search radius) -> n x k rt_near (probe-major,
// the k nearest of each probe's accepted set by (key, sphere index)) and n counts (may be null)
// against a.sc; 1 <= k <= RT_CLOSEST_MAX; slack_m: closest_slack_m of the root box; counters !=
// null: a stats launch
hipError_t launch_closest(const FrameArgs& a, const void* probes, void* near, void* counts, uint32_t n,
                          uint32_t k, bool skip_self, float slack_m, unsigned long long* counters,
                          hipStream_t st);
// rt_sweep.hip: n casts (rt_ray, with radii[i] or, radii null, `radius`) -> n rt_hit: the first sphere
// each moving ball touches by (t, sphere index) against a.sc; slack_m: sweep_slack_m of the root box;
// counters != null: a stats launch
hipError_t launch_sweep(const FrameArgs& a, const void* rays, const void* radii, float radius, void* hits,
                        uint32_t n, bool entry_only, bool skip_self, float slack_m,
                        unsigned long long* counters, hipStream_t st);
// rt_gbuffer.hip: the first-hit G-buffer of a.cam at a.W x a.H against a.sc; null buffers are skipped
hipError_t launch_gbuffer(const FrameArgs& a, void* hits, void* normals, void* albedo,
                          unsigned long long* counters, hipStream_t st);
// rt_ao.hip: the ambient-occlusion layer of a.cam at a.W x a.H against a.sc: `rays` (1, 2, .. 64) any-hit rays
// of length `radius` per hit pixel, directions keyed by `key` (rt_ao_math.h ao_key); null buffers are skipped
hipError_t launch_ao(const FrameArgs& a, void* ao, void* occluded, uint32_t rays, float radius, uint32_t key,
                     unsigned long long* counters, hipStream_t st);
// rt_indirect.hip: the one-bounce diffuse layer of a.cam at a.W x a.H against a.sc (prim_al made), shaded with a.L,
// a.ambient and a.shadows: rt_ao.hip's `rays` rays to their nearest hits within `radius`, an escaped ray bringing
// sky_scale times the frames' miss colour; W*H float4 {r, g, b, open share} and W*H hit counts, null buffers skipped
hipError_t launch_indirect(const FrameArgs& a, void* layer, void* occluded, uint32_t rays, float radius, uint32_t key,
                           float sky_scale, unsigned long long* counters, hipStream_t st);
// rt_filter.hip: the guide-driven filter of a W x H layer of `channels` floats a pixel (rt_filter_math.h: the
// parameters, which the caller checked, and the pass plan): packs hits and normals into `rec` (W*H), then `passes`
// passes from `in` to `out` through `pong` (as large as the layer; may be null for one pass)
hipError_t launch_filter(uint32_t W, uint32_t H, const void* hits, const void* normals, float4* rec, const void* in,
                         void* out, float* pong, uint32_t passes, uint32_t channels, float depth_sigma,
                         uint32_t normal_power, hipStream_t st);
// ... and the multiply of a W x H layer into packed RGBA8 pixels in place: m = floor + (1 - floor) * layer
hipError_t launch_apply_layer(uint32_t* rgba8, const float* layer, uint32_t W, uint32_t H, float floor,
                              hipStream_t st);
// ... and a W x H float4 layer's r, g, b added into packed RGBA8 pixels in place, times `gain` and (albedo != null) the
// pixel's albedo bytes / 255 (rt_indirect_math.h add_layer_pixel)
hipError_t launch_add_layer(uint32_t* rgba8, const void* layer4, const uint32_t* albedo, uint32_t W, uint32_t H,
                            float gain, hipStream_t st);
// rt_reproject.hip: a W x H layer of `channels` floats a pixel carried from the previous camera `prev` into `cam`
// (rt_reproject_math.h: the parameters, which the caller checked): `hits` and `cur` of the current frame to `out` and
// `count_out`; h_hits, h_layer and h_count the previous frame's, h_hits null for no history
hipError_t launch_reproject(const CamArgs& cam, uint32_t W, uint32_t H, const void* hits, const void* cur, void* out,
                            void* count_out, const void* h_hits, const void* h_layer, const void* h_count,
                            const PrevCamera& prev, uint32_t channels, float max_count, float depth_tol, hipStream_t st);

// screen_bins.hip: the per-frame screen-space bins
struct BinBuild {
    const float4* spheres;      // by sphere index
    const uint32_t* first_ref;  // per sphere: one leaf reference of it (launch_first_refs)
    uint32_t n_spheres;
    float K[9], R[9], o[3];     // the frame's camera (CamArgs)
    uint32_t W, H, nbx, nby;
    uint32_t tw, th;            // the frame's wave tile (FramePlan::grid): powers of two, <= 8
    double shrink;             // 1; 0.9 under the test hook RT_TEST_BIN_SHRINK
    uint32_t capacity;          // entries `ent` holds
    uint32_t cap;               // a bin over it walks (<= kBinCap)
    uint32_t mean_max;          // the frame walks over this mean list length
    uint32_t frame_id;
    uint4* rects;               // [n_spheres] scratch
    uint32_t* counts;           // [nbx * nby + 1], then in the same allocation (rt_bins_math.h):
    uint32_t* cursor;           // [nbx * nby],
    uint32_t* decide;           // [kBinDecWords] bins_decide's partial results and arrival counter,
    uint32_t* info;             // [kBinInfoWords]
    uint32_t* offs;             // [nbx * nby + 1]
    uint2* hdr;                 // [nbx * nby], the tile words behind them (FrameArgs::bin_nb)
    uint4* ent;                 // [2 * capacity]
    unsigned long long* tiles;  // [nbx * nby * tiles per bin] tile words (rt_bins_math.h)
    uint4* wide;               // [2 * kBinWideCap]
    uint32_t* mirror;          // the renderer's pinned copy of info (device pointer)
    void* temp;                 // the scan's scratch
    size_t temp_bytes;
};
hipError_t launch_first_refs(const float4* prim_sp, const uint32_t* prim_idx, uint32_t n_slots,
                             const float4* spheres, uint32_t n_spheres, uint32_t* first_ref,
                             hipStream_t st);
size_t bins_scan_temp_bytes(uint32_t n_items);
hipError_t launch_screen_bins(const BinBuild& b, hipStream_t st);

// rt_last_error(NULL): the calling thread's last failure without a handle
extern thread_local std::string g_last_error;
int fail(rt_renderer* r, int code, const std::string& msg);
int hip_fail(rt_renderer* r, hipError_t e, const char* what);

#define RT_HIP(r, call)                                   \
    do {                                                  \
        hipError_t e_ = (call);                           \
        if (e_ != hipSuccess) return hip_fail((r), e_, #call); \
    } while (0)

template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;  // elements
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
};

template <typename T>
int ensure(rt_renderer* r, DevBuf<T>& b, size_t n) {
    if (b.n >= n && b.p) return RT_OK;
    b.release();
    if (n == 0) n = 1;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&b.p), n * sizeof(T));
    if (e != hipSuccess) {
        b.p = nullptr;
        return hip_fail(r, e, "hipMalloc");
    }
    b.n = n;
    return RT_OK;
}

// A device array derived from the scene's leaf references and a key of up to
// 13 floats (a camera origin, a basis): its records stand for the scene
// generation and the key they were made for.  query() sizes the array and says
// whether the records must be remade (a reallocation forgets what they were
// made for); commit() follows the kernel that remade them.
template <typename T>
struct DerivedRecords {
    DevBuf<T> buf;
    uint64_t gen = ~0ull;  // no scene yet
    float key[13] = {};
    int query(rt_renderer* r, size_t n, uint64_t scene_gen, const float* k, size_t nk, bool* stale) {
        const T* before = buf.p;
        if (const int st = ensure(r, buf, n)) return st;
        if (buf.p != before) gen = ~0ull;
        *stale = gen != scene_gen || (nk && memcmp(key, k, nk * sizeof(float)) != 0);
        return RT_OK;
    }
    void commit(uint64_t scene_gen, const float* k, size_t nk) {
        if (nk) memcpy(key, k, nk * sizeof(float));
        gen = scene_gen;
    }
};

// rt_create_multi: the frame's tiles over several
// devices of this process; `r` (the handle) is devices[0]'s renderer
struct MultiState {
    static constexpr int F = 2;            // frames in flight
    static constexpr uint32_t kTs = 64;    // tile side
    std::vector<int> devs;                 // devs[0] = the handle's device
    std::vector<rt_renderer*> peers;       // peers[k] renders device k's tiles (peers[0] = the handle)
    uint32_t transport = 0;                // RT_TRANSPORT_RCCL / RT_TRANSPORT_PEER
    std::vector<ncclComm*> comms;          // one per device (ncclCommInitAll)
    std::vector<hipStream_t> cs;           // per-device comm stream
    // devices[0]'s output stream: what a NULL stream argument means for the
    // handle (rt_stream).  Not devices[0]'s render stream, so that the wait
    // for frame j's unpack does not hold frame j+1's tiles on device 0.
    hipStream_t out = nullptr;
    // per frame slot f: each device's packed slab, devices[0]'s receive buffer
    // of n slabs end to end, and the events that order their reuse (all
    // timing-disabled: they are waited on every frame)
    std::vector<void*> slab[F];
    void* recv[F] = {nullptr, nullptr};
    std::vector<hipEvent_t> rendered[F], sent[F];
    hipEvent_t recvd[F] = {nullptr, nullptr}, unpacked[F] = {nullptr, nullptr}, out_ready = nullptr;
    bool used[F] = {false, false};
    // rt_get_multi_timing: timing events, recorded only once the caller has
    // asked for timing: device k's render start / end, devices[0]'s
    // unpack end; timed[f] = slot f's frame recorded them
    bool timing = false;
    bool timed[F] = {false, false};
    std::vector<hipEvent_t> t_start[F], t_end[F];
    hipEvent_t t_unpacked[F] = {nullptr, nullptr};
    uint64_t frame = 0;
    // a resize that failed part-way leaves the devices at different sizes:
    // rt_render refuses the handle until a resize succeeds
    bool broken = false;
    // test-only fault injection (RT_TEST_FAULT with RT_FLAG_TEST_HOOKS, read
    // once by rt_create_multi): "create:k" peer k's rt_create fails, "comm"
    // ncclCommInitAll fails, "slab:k" the slab allocation on peer k fails,
    // "queue:k" peer k's plain frames report themselves incomplete (as a
    // slot that was never published: RendererState::test_fault_queue)
    enum Fault { kNone = 0, kCreate, kComm, kSlab, kQueue };
    int fault = kNone;
    uint32_t fault_k = 0;
    // tile plan for the current size
    uint32_t W = 0, H = 0, S = 0;          // S = slab tiles
    size_t slab_bytes = 0;
    std::vector<std::vector<uint32_t>> ids;
    std::vector<uint32_t> all_ids;         // n * S, padding slots RT_TILE_SKIP
    uint32_t* d_all_ids = nullptr;         // on devices[0]
};

// The screen-space bins of a renderer (screen_bins.hip, DESIGN.md 5.1 round
// 10), rebuilt by every plain frame that reads them (rt_bins_host.cpp).
struct ScreenBinState {
    DerivedRecords<uint32_t> first_ref;  // per sphere, made once per scene
    DevBuf<uint4> rects, ent, wide;
    DevBuf<uint32_t> cnt, offs;  // cnt: counts, cursors, bins_decide's words, the frame's info words    // the bins' headers, then the tile words in the same allocation: 64 per
    // bin whatever the frame's wave tile (8 B a pixel, 16.6 MB at 1080p), so a
    // change of spp between frames reallocates nothing
    DevBuf<uint2> hdr;
    uint32_t tw = 1, th = 1;  // the wave tile of the last frame that built bins
    DevBuf<unsigned char> temp;
    uint32_t temp_items = 0;
    // the pinned host copy of the info words, which the next rt_render reads
    // without a sync (a frame that overflowed `ent` walks, and the next frame
    // gets a larger buffer), and its device pointer
    uint32_t* mirror = nullptr;
    uint32_t* mirror_dev = nullptr;
    // the RT_TEST_BIN_* hooks: cap, capacity_test, shrink, min_samples, mean_max (kBinMeanMax)
    uint32_t cap = 64, capacity_test = 0, mean_max = 48;
    double shrink = 1.0;
    uint64_t min_samples = kBinMinSamples;
    BinCadence cadence;                        // the dense skip; the last building frame's id
    uint32_t last_reason = RT_BINS_NO_FRAME;  // why the last frame had bins or not (rt_get_bin_info)
    uint32_t last_capacity = 0, nbx = 0, nby = 0;  // ... and that build's sizes
    hipEvent_t e0 = nullptr, e1 = nullptr;
    bool timing = false, timed = false;
    void release() {
        first_ref.buf.release();
        rects.release();
        ent.release();
        wide.release();
        cnt.release();
        offs.release();
        hdr.release();
        temp.release();
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        if (mirror) (void)hipHostFree(mirror);
    }
};

// The query path's scratch (rt_queries.cpp): its own stat lines (a query never
// touches the frames' counter sets) and the single-item wrappers' records.
struct QueryScratch {
    DevBuf<unsigned long long> counters;
    DevBuf<float4> ray;              // rt_pick, rt_pick_multi: one ray
    DevBuf<uint2> hit;               // rt_pick: one hit
    DevBuf<uint2> multi_hits;        // rt_pick_multi: up to RT_MULTIHIT_MAX hits
    DevBuf<uint32_t> multi_count;    // ... and the count
    DevBuf<float4> probe;            // rt_overlaps_at, rt_closest_at: the probe,
    DevBuf<uint32_t> overlap_idx;    // up to RT_OVERLAP_MAX indices
    DevBuf<uint32_t> overlap_count;  // and the count word
    DevBuf<uint2> near;              // rt_closest_at: up to RT_CLOSEST_MAX rt_near
    DevBuf<uint32_t> near_count;     // and the count
    DevBuf<float4> cast;             // rt_sweep_at, rt_pick_thick: one cast's ray,
    DevBuf<uint2> cast_hit;          // and its hit
    void release() {
        counters.release();
        ray.release();
        hit.release();
        multi_hits.release();
        multi_count.release();
        probe.release();
        overlap_idx.release();
        overlap_count.release();
        near.release();
        near_count.release();
        cast.release();
        cast_hit.release();
    }
};

// rt_filter_layer's scratch: the packed guide records of the last call's size and the
// one layer the passes alternate with the caller's output.  Like QueryScratch it
// only grows and is released with the handle.
struct FilterScratch {
    DevBuf<float4> rec;   // W*H x {n.x, n.y, n.z, t}
    DevBuf<float> pong;   // W*H*channels
    void release() {
        rec.release();
        pong.release();
    }
};

// what an rt_renderer holds (the C-ABI's opaque struct, below, is exactly this)
struct RendererState {
    rt_config cfg;
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // completion of the renderer's last queued work (render, tiles, unpack) on
    // whichever stream it ran: a launch on another stream is ordered after it
    // (the counters, queue heads and buffers are shared), and
    // rt_synchronize / rt_readback wait for it
    hipEvent_t done = nullptr;
    hipStream_t last_stream = nullptr;
    bool pending = false;
    // wave-queue failure report (FrameArgs::qerr): a pinned host-coherent word
    // the kernel stores a failed frame's id into; the host reports each new
    // value once (queue_report), from rt_render without any copy or sync
    uint32_t* qerr_host = nullptr;
    uint32_t* qerr_dev = nullptr;
    uint32_t frame_seq = 0;   // last frame id handed out (never 0)
    uint32_t qerr_seen = 0;   // last reported value of *qerr_host
    // test only (RT_TEST_FAULT=queue:k, RT_FLAG_TEST_HOOKS): plain frames
    // report themselves failed
    bool test_fault_queue = false;
    float pose[16];
    float K[9];
    uint32_t W = 0, H = 0;
    DevBuf<uint32_t> fb;
    DevBuf<float4> rad;
    DevBuf<float4> accum;            // RT_FLAG_PROGRESSIVE running sums
    uint32_t frames_accum = 0;       // frames in `accum` (0: next frame starts over)
    uint64_t accum_sig = 0;          // which pixels the sums belong to (frame / tile list)
    DevBuf<unsigned long long> counters;
    // the counters, queue heads and slot table in two sets of ctr_stride
    // words: a scene frame uses set ctr_set and its kernel zeroes the other
    // one for the next frame (FrameArgs::ctr_next), so no memset launch sits
    // between frames; ctr_zero[s] = leading words of set s known to be zero
    size_t ctr_stride = 0;
    uint32_t ctr_set = 0;
    size_t ctr_zero[2] = {0, 0};
    // superblock claim order of full frames (FrameArgs::sb_order) and the
    // superblock grid it was made for
    DevBuf<uint32_t> sb_order;
    uint32_t sb_nx = 0, sb_ny = 0;
    // device copies of recently used tile lists (rt_render_tiles: this rank's
    // list; rt_unpack_tiles on rank 0: one list per peer), least recently used
    // evicted; each host vector stays alive as the source of its async upload
    struct TileList {
        std::vector<uint32_t> host;
        DevBuf<uint32_t> dev;
        uint64_t used = 0;
    };
    std::vector<TileList> tile_lists;
    uint64_t tile_clock = 0;
    // display buffer mapped per frame: the Displayer's
    // registered GL PBO through the HIP graphics ops, or a caller's ops
    rt_display_ops disp{};
    void* disp_user = nullptr;
    bool gl_disp = false;  // disp are the built-in HIP graphics-interop ops
    // scene: the sphere list lives in d_spheres/d_albedo; `spheres` is a host
    // copy when the scene came from host memory (host builder input)
    uint32_t n_spheres = 0;
    std::vector<float> spheres;
    bool host_copy = false;
    // leaf-reference arrays' length (prim_sp / prim_idx / the screen records):
    // info.n_prim_refs, plus the gaps of the line-packed layout (pack_leaf_lines)
    uint32_t prim_slots = 0;
    bool leaf_packed = false;
    // test only: RT_TEST_CLAIM_DELAY at rt_create with RT_FLAG_TEST_HOOKS
    // (FrameArgs::wq_claim_delay)
    uint32_t test_claim_delay = 0;
    uint32_t last_instance = 0;  // Frame<> switches of the last scene launch (rt_last_instance)
    // test only, read at rt_create with RT_FLAG_TEST_HOOKS: the A/B switches
    // RT_SORT=0 (no sorted rounds), RT_LDS_STAGE=0 (no LDS leaf staging),
    // RT_LEAF_PACK=1 (line-packed leaf lists) and RT_SB_ORDER=1 (superblocks
    // claimed along a Hilbert curve); images and counters are the same
    bool sort_rounds = true, lds_stage = true, leaf_pack = false, sb_hilbert = false;
    rt_octree_params oct;
    bool has_scene = false;
    GpuOctreeBuilder gpu_build;
    CellTable cell_table;
    DevBuf<uint2> d_nodes;
    DevBuf<float4> d_prim_sp;
    DevBuf<uint32_t> d_prim_idx;
    DevBuf<float4> d_spheres;
    DevBuf<uint32_t> d_albedo;
    SceneArgs sc{};
    uint64_t scene_gen = 0;  // counts scene builds: what the derived records are made for
    // camera-relative screen records (SceneArgs::prim_cam); key: the camera origin
    DerivedRecords<float4> prim_cam;
    // image-plane screen records (SceneArgs::prim_cam8); key: the camera
    // origin, the basis and its check (cam8_basis)
    DerivedRecords<float2> prim_cam8;
    // the light-plane screen records, {u, v} in 8 bytes (SceneArgs::prim_shd8;
    // key: the basis), and their radius term (FrameArgs::shd_rr; d_shd_rr: the
    // kernel's max, in bits, copied into shd_rr_bits)
    DerivedRecords<float2> prim_shd8;
    DevBuf<uint32_t> d_shd_rr;
    uint32_t shd_rr_bits = 0;
    float shd_rr = 0.0f;
    // albedo by leaf reference (SceneArgs::prim_al); no key
    DerivedRecords<uint32_t> prim_al;
    // occluder lists (SceneArgs::prim_occ / occ_sp, occluder.hip): built with
    // the light-plane records, for the same scene and light; occ_cap: the
    // per-sphere cap (kOccCap, or RT_TEST_OCC_CAP under RT_FLAG_TEST_HOOKS);
    // occ_e0 / occ_e1 time the build (collected at the renderer's next
    // synchronisation, occ_collect_time); occ_M: the M the lists were made with
    OccluderLists occ;
    uint32_t occ_cap = kOccCap;
    double occ_mean_max = kOccMeanMax;  // (RT_TEST_OCC_MEAN under RT_FLAG_TEST_HOOKS)
    hipEvent_t occ_e0 = nullptr, occ_e1 = nullptr;
    bool occ_timed = false;
    double occ_M = 0.0;
    ScreenBinState bins;
    QueryScratch q;
    FilterScratch flt;
    rt_scene_info info{};
    std::string err;
    // multi-device handle (rt_create_multi): this renderer is devices[0]'s
    // part; the state holds the other devices' renderers and the transport
    MultiState* multi = nullptr;
    // the occluder lists stand for the current scene (made with its light-plane records)
    bool occluders_current() const { return occ.on() && prim_shd8.gen == scene_gen; }
};

}  // namespace rtamd

struct rt_renderer : rtamd::RendererState {};

namespace rtamd {

// rt_capi.cpp
int set_device(rt_renderer* r);
void fill_camera(const rt_renderer* r, CamArgs& cam);
const char* test_env(uint32_t flags, const char* name);
int order_after_last(rt_renderer* r, hipStream_t st);
int mark_queued(rt_renderer* r, hipStream_t st);
int queue_report(rt_renderer* r);
void occ_collect_time(rt_renderer* r);
// rt_scene.cpp
int build_scene(rt_renderer* r);
// rt_frame.cpp
void fill_frame_args(rt_renderer* r, FrameArgs& a);
void fill_shading(const rt_renderer* r, FrameArgs& a);  // a.L, a.ambient, a.shadows of the handle's config
int do_render(rt_renderer* r, FrameArgs& a, void* stream, rt_stats* stats);
int ensure_prim_al(rt_renderer* r, SceneArgs& sc, hipStream_t st);
int check_tiles(rt_renderer* r, const uint32_t* ids, uint32_t n_tiles, uint32_t ts,
                bool allow_skip = false);
int tile_list(rt_renderer* r, const uint32_t* ids, uint32_t n, hipStream_t s, const uint32_t** out);
void accum_pixels(rt_renderer* r, const uint32_t* ids, uint32_t n, uint32_t ts);
int render_tiles_one(rt_renderer* r, const uint32_t* tile_ids, uint32_t n_tiles, uint32_t ts,
                     void* dev_packed, void* stream, rt_stats* stats);
int unpack_tiles_one(rt_renderer* r, const void* dev_packed, const uint32_t* tile_ids,
                     uint32_t n_tiles, uint32_t ts, void* dev_rgba8, void* stream);
// the work counters of a stats launch: {primary, shadow, nodes, prims} per XCD
// group, one line each (kStatLineBase), summed into c
constexpr size_t kStatLineWords = 8 * kStatLineStride;
inline void sum_stat_lines(const unsigned long long* lines, unsigned long long c[4]) {
    for (uint32_t i = 0; i < 4; ++i) c[i] = 0;
    for (uint32_t q = 0; q < 8; ++q)
        for (uint32_t i = 0; i < 4; ++i) c[i] += lines[q * kStatLineStride + i];
}
// rt_bins_host.cpp: do_render's step 4b
int screen_bins(rt_renderer* r, FrameArgs& a, const FramePlan& plan, hipStream_t st);
// rt_multi.cpp: a multi-device handle's part of the calls above
int multi_render(rt_renderer* r, uint32_t* out, hipStream_t hs, rt_stats* stats);
int multi_wait(rt_renderer* r);
int multi_synchronize(rt_renderer* r);
int multi_queue_report(rt_renderer* r);
void multi_destroy(rt_renderer* r);
int multi_set_scene_device(rt_renderer* r, uint32_t n, const rt_octree_params* oct);

// " (device <ordinal>, peer <k>)": names the device in a multi-device error
inline std::string peer_name(const MultiState& m, size_t k) {
    return " (device " + std::to_string(m.devs[k]) + ", peer " + std::to_string(k) + ")";
}
// apply `fn` to every other device's renderer of a multi-device handle
template <typename Fn>
int for_peers(rt_renderer* r, Fn fn) {
    if (!r || !r->multi) return RT_OK;
    for (size_t k = 1; k < r->multi->peers.size(); ++k) {
        const int st = fn(r->multi->peers[k]);
        if (st) {
            r->err = r->multi->peers[k]->err + peer_name(*r->multi, k);
            return st;
        }
    }
    return RT_OK;
}
// the stream a NULL stream argument means: the renderer's own, or a
// multi-device handle's output stream on devices[0]
inline hipStream_t own_stream(const rt_renderer* r) { return r->multi ? r->multi->out : r->stream; }

}  // namespace rtamd
