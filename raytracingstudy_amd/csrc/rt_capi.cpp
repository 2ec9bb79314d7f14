// rt_capi.cpp — the C-ABI (include/rt.h) over the HIP kernels: handle
// lifetime, camera state, rt_render and the display binding.  The scene is
// rt_scene.cpp's, a frame's preparation and launch rt_frame.cpp's (its screen
// bins rt_bins_host.cpp's), the queries and the G-buffer rt_queries.cpp's, the
// multi-device handle rt_multi.cpp's; rt_host.h holds what they share.
//
// Host runtime that replaces KernelRenderer (include/renderer.cuh:25-50,
// src/renderer.cu:111-198): camera/octree state lives on the host and goes to
// the kernels by value; device buffers are owned here (the reference leaks
// its device-heap Camera/Octree, src/renderer.cu:189-198); every call returns
// a status (the reference's render path checks nothing, :145-151).
#include <mutex>

#include "rt_host.h"

using namespace rtamd;

namespace rtamd {

thread_local std::string g_last_error;

int fail(rt_renderer* r, int code, const std::string& msg) {
    g_last_error = msg;
    if (r) r->err = msg;
    return code;
}

int hip_fail(rt_renderer* r, hipError_t e, const char* what) {
    std::string m = std::string(what) + ": " + hipGetErrorString(e);
    return fail(r, RT_E_HIP, m);
}

int set_device(rt_renderer* r) {
    RT_HIP(r, hipSetDevice(r->device));
    return RT_OK;
}

// the renderer's intrinsic and pose as the kernels take them
void fill_camera(const rt_renderer* r, CamArgs& cam) {
    memcpy(cam.K, r->K, sizeof(r->K));
    for (int c = 0; c < 3; ++c)
        for (int row = 0; row < 3; ++row) cam.R[c * 3 + row] = r->pose[c * 4 + row];
    cam.o[0] = r->pose[12];
    cam.o[1] = r->pose[13];
    cam.o[2] = r->pose[14];
}

// A test hook's environment variable (RT_TEST_*): its value when the config
// carries RT_FLAG_TEST_HOOKS, else NULL.  Either way a set variable is named
// on stderr once per process, so a stray one is visible.
const char* test_env(uint32_t flags, const char* name) {
    const char* v = getenv(name);
    if (!v || !*v) return nullptr;
    const bool on = (flags & RT_FLAG_TEST_HOOKS) != 0;
    static std::mutex mu;
    static std::vector<std::string> said;
    {
        std::lock_guard<std::mutex> g(mu);
        const std::string key = std::string(name) + (on ? "+" : "-");
        if (std::find(said.begin(), said.end(), key) == said.end()) {
            said.push_back(key);
            fprintf(stderr, on ? "librt_amd: test hook %s=%s active (RT_FLAG_TEST_HOOKS)\n"
                               : "librt_amd: %s=%s ignored (test hooks need RT_FLAG_TEST_HOOKS)\n",
                    name, v);
        }
    }
    return on ? v : nullptr;
}

// Order work about to be queued on `st` after the renderer's last queued work
// when that ran on another stream (caller streams are typically non-blocking).
int order_after_last(rt_renderer* r, hipStream_t st) {
    if (r->pending && r->last_stream != st) RT_HIP(r, hipStreamWaitEvent(st, r->done, 0));
    return RT_OK;
}

int mark_queued(rt_renderer* r, hipStream_t st) {
    RT_HIP(r, hipEventRecord(r->done, st));
    r->last_stream = st;
    r->pending = true;
    return RT_OK;
}

// The occluder build's device time into info.occluder_build_ms: called where
// the renderer has just synchronised (stats frames, rt_synchronize,
// rt_readback), once the build's last kernel is done; never waits.
void occ_collect_time(rt_renderer* r) {
    if (!r->occ_timed || hipEventQuery(r->occ_e1) != hipSuccess) return;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, r->occ_e0, r->occ_e1) == hipSuccess) r->info.occluder_build_ms = ms;
    r->occ_timed = false;
}

// A frame the kernel found incomplete (its wave queue's bounded slot wait
// gave up, rt_kernels.hip) stored its id in the renderer's pinned word; each
// new value is reported once.  A plain host read: rt_render calls it before
// every frame with no sync, rt_synchronize / rt_readback / stats frames after
// theirs.
int queue_report(rt_renderer* r) {
    const uint32_t v = __atomic_load_n(r->qerr_host, __ATOMIC_ACQUIRE);
    if (v == r->qerr_seen) return RT_OK;
    r->qerr_seen = v;
    return fail(r, RT_E_HIP, "scene kernel: wave-queue slot never published: frame " +
                                 std::to_string(v) + " of this renderer is incomplete");
}

}  // namespace rtamd

extern "C" {

int rt_abi_version(void) { return RT_ABI_VERSION; }

int rt_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

void rt_config_default(rt_config* c) {
    memset(c, 0, sizeof(*c));
    c->width = 1280;  // main.cpp:6
    c->height = 720;
    c->spp = 1;
    c->seed = 0x2545F491u;
    c->device = -1;
    c->mode = RT_MODE_COMPAT;
    c->flags = 0;
    c->light_dir[0] = 1.0f;  // normalize(1,1,-1)
    c->light_dir[1] = 1.0f;
    c->light_dir[2] = -1.0f;
    c->ambient = 0.1f;
}

void rt_octree_params_default(rt_octree_params* p) {
    memset(p, 0, sizeof(*p));
    for (int i = 0; i < 3; ++i) {
        p->min[i] = 0.0f;   // src/renderer.cu:134
        p->max[i] = 1.28f;  // src/renderer.cu:135
    }
    p->resolution = 0.01f;  // src/renderer.cu:136
    p->max_depth = 0;
    p->leaf_capacity = 8;
}

void rt_resize_intrinsic(uint32_t width, uint32_t height, float K[9]) {
    // src/renderer.cu:162-170 (float arithmetic, integer cx/cy)
    const float rad = 80.f * 0.01745329251994329576923690768489f;
    const float f = static_cast<float>(width) / (2.0f * tanf(rad / 2.0f));
    for (int i = 0; i < 9; ++i) K[i] = 0.0f;
    K[0] = f;
    K[4] = f;
    K[8] = 1.0f;
    K[2] = static_cast<float>(width / 2u);
    K[5] = static_cast<float>(height / 2u);
}

int rt_create(const rt_config* cfg, rt_renderer** out) {
    if (!cfg || !out) return fail(nullptr, RT_E_INVALID, "rt_create: null argument");
    *out = nullptr;
    if (cfg->width == 0 || cfg->height == 0 || cfg->width > 32768 || cfg->height > 32768)
        return fail(nullptr, RT_E_INVALID, "rt_create: width/height out of range");
    if (cfg->mode != RT_MODE_COMPAT && cfg->mode != RT_MODE_SCENE)
        return fail(nullptr, RT_E_INVALID, "rt_create: unknown mode");
    if (!variant_available((cfg->flags >> RT_FLAG_VARIANT_SHIFT) & 0xFu))
        return fail(nullptr, RT_E_INVALID,
                    "rt_create: scene-kernel variant not in this build (0, 4, 7, 10 or 13)");
    if (((cfg->flags >> (RT_FLAG_OPT_SHIFT + kOptChunkShift)) & 7u) > kOptChunkMax)
        return fail(nullptr, RT_E_INVALID,
                    "rt_create: wave-queue ticket size field (flags bits 24..26) must be 0..4");
    rt_renderer* r = new (std::nothrow) rt_renderer();
    if (!r) return fail(nullptr, RT_E_NOMEM, "rt_create: out of host memory");
    r->cfg = *cfg;
    if (r->cfg.spp == 0) r->cfg.spp = 1;
    int dev = cfg->device;
    if (dev < 0) {
        if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    }
    r->device = dev;
    r->W = cfg->width;
    r->H = cfg->height;
    // test only (tests/test_gpu_variants.py, test_gpu_queue_report.py)
    if (const char* cd = test_env(cfg->flags, "RT_TEST_CLAIM_DELAY"))
        r->test_claim_delay = static_cast<uint32_t>(std::min(100000ul, strtoul(cd, nullptr, 10)));
    // test only (tests/test_gpu_occluders.py): the per-sphere cap of the occluder lists
    if (const char* oc = test_env(cfg->flags, "RT_TEST_OCC_CAP"))
        r->occ_cap = static_cast<uint32_t>(std::min<unsigned long>(kOccCapMax, strtoul(oc, nullptr, 10)));
    // ... and the scene rule's mean candidate count (a dense test scene on lists)
    if (const char* om = test_env(cfg->flags, "RT_TEST_OCC_MEAN")) r->occ_mean_max = strtod(om, nullptr);
    // test only (tests/test_gpu_bins.py): the per-bin cap of the screen-space
    // bins, a tiny entry buffer (the frame-level fallback), rectangles from
    // radii x 0.9 (a negative control: unsound lists), the frame size below
    // which a frame walks
    if (const char* v = test_env(cfg->flags, "RT_TEST_BIN_CAP"))
        r->bins.cap = static_cast<uint32_t>(std::min<unsigned long>(64ul, strtoul(v, nullptr, 10)));
    if (const char* v = test_env(cfg->flags, "RT_TEST_BIN_CAPACITY"))
        r->bins.capacity_test = static_cast<uint32_t>(std::max(1ul, std::min(1ul << 24, strtoul(v, nullptr, 10))));
    if (const char* v = test_env(cfg->flags, "RT_TEST_BIN_SHRINK")) r->bins.shrink = atoi(v) != 0 ? 0.9 : 1.0;
    if (const char* v = test_env(cfg->flags, "RT_TEST_BIN_MIN_SAMPLES")) r->bins.min_samples = strtoull(v, nullptr, 10);
    // ... and the mean list length over which a frame walks (tiny test frames are dense)
    if (const char* v = test_env(cfg->flags, "RT_TEST_BIN_MEAN"))
        r->bins.mean_max = static_cast<uint32_t>(std::min(1ul << 20, strtoul(v, nullptr, 10)));
    if (const char* fe = test_env(cfg->flags, "RT_TEST_FAULT"))
        r->test_fault_queue = strcmp(fe, "queue:0") == 0;
    // ... and the A/B switches ("0" off, any other number on)
    if (const char* v = test_env(cfg->flags, "RT_SORT")) r->sort_rounds = atoi(v) != 0;
    if (const char* v = test_env(cfg->flags, "RT_LDS_STAGE")) r->lds_stage = atoi(v) != 0;
    if (const char* v = test_env(cfg->flags, "RT_LEAF_PACK")) r->leaf_pack = atoi(v) != 0;
    if (const char* v = test_env(cfg->flags, "RT_SB_ORDER")) r->sb_hilbert = atoi(v) != 0;
    // src/renderer.cu:87-89: K0 = mat3(1000,0,640, 0,1000,340, 0,0,1), pose = mat4(1)
    const float K0[9] = {1000.f, 0.f, 640.f, 0.f, 1000.f, 340.f, 0.f, 0.f, 1.f};
    memcpy(r->K, K0, sizeof(K0));
    for (int i = 0; i < 16; ++i) r->pose[i] = (i % 5 == 0) ? 1.0f : 0.0f;
    rt_octree_params_default(&r->oct);
    int st;
    hipError_t e = hipSetDevice(dev);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate(&r->ev0);
    if (e == hipSuccess) e = hipEventCreate(&r->ev1);
    if (e == hipSuccess) e = hipEventCreate(&r->occ_e0);
    if (e == hipSuccess) e = hipEventCreate(&r->occ_e1);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&r->done, hipEventDisableTiming);
    // the frame-failure word: pinned, host-coherent, mapped for the kernels
    if (e == hipSuccess)
        e = hipHostMalloc(reinterpret_cast<void**>(&r->qerr_host), sizeof(uint32_t),
                          hipHostMallocMapped | hipHostMallocCoherent);
    if (e == hipSuccess) {
        *r->qerr_host = 0;
        e = hipHostGetDevicePointer(reinterpret_cast<void**>(&r->qerr_dev), r->qerr_host, 0);
    }
    // the screen-space bins' info words: pinned like the failure word
    if (e == hipSuccess) e = hipEventCreate(&r->bins.e0);
    if (e == hipSuccess) e = hipEventCreate(&r->bins.e1);
    if (e == hipSuccess)
        e = hipHostMalloc(reinterpret_cast<void**>(&r->bins.mirror), kBinInfoWords * sizeof(uint32_t),
                          hipHostMallocMapped | hipHostMallocCoherent);
    if (e == hipSuccess) {
        memset(r->bins.mirror, 0, kBinInfoWords * sizeof(uint32_t));
        e = hipHostGetDevicePointer(reinterpret_cast<void**>(&r->bins.mirror_dev), r->bins.mirror, 0);
    }
    if (e != hipSuccess) {
        st = hip_fail(nullptr, e, "rt_create");
        rt_destroy(r);
        return st;
    }
    const size_t px = (size_t)r->W * r->H;
    if ((st = ensure(r, r->fb, px)) || (st = ensure(r, r->counters, kCounterWords)) ||
        ((cfg->flags & RT_FLAG_PROGRESSIVE) && (st = ensure(r, r->accum, px))) ||
        ((cfg->flags & RT_FLAG_RADIANCE) && (st = ensure(r, r->rad, px)))) {
        g_last_error = r->err;
        rt_destroy(r);
        return st;
    }
    *out = r;
    return RT_OK;
}

int rt_destroy(rt_renderer* r) {
    if (!r) return RT_OK;
    if (r->multi) multi_destroy(r);
    (void)hipSetDevice(r->device);
    if (r->stream) (void)hipStreamSynchronize(r->stream);
    if (r->pending) (void)hipEventSynchronize(r->done);  // work on a caller's stream
    r->fb.release();
    r->rad.release();
    r->accum.release();
    r->counters.release();
    for (auto& e : r->tile_lists) e.dev.release();
    r->d_nodes.release();
    r->d_prim_sp.release();
    r->d_prim_idx.release();
    r->d_spheres.release();
    r->d_albedo.release();
    r->prim_cam.buf.release();
    r->prim_al.buf.release();
    r->prim_cam8.buf.release();
    r->prim_shd8.buf.release();
    r->d_shd_rr.release();
    r->q.release();
    r->flt.release();
    r->sb_order.release();
    r->gpu_build.release();
    r->cell_table.release();
    r->occ.release();
    r->bins.release();  // (its buffers, events and pinned words)
    if (r->occ_e0) (void)hipEventDestroy(r->occ_e0);
    if (r->occ_e1) (void)hipEventDestroy(r->occ_e1);
    if (r->ev0) (void)hipEventDestroy(r->ev0);
    if (r->ev1) (void)hipEventDestroy(r->ev1);
    if (r->done) (void)hipEventDestroy(r->done);
    if (r->stream) (void)hipStreamDestroy(r->stream);
    if (r->qerr_host) (void)hipHostFree(r->qerr_host);
    delete r;
    return RT_OK;
}

int rt_set_pose(rt_renderer* r, const float pose[16]) {
    if (!r || !pose) return fail(r, RT_E_INVALID, "rt_set_pose: null argument");
    if (memcmp(r->pose, pose, sizeof(r->pose)) != 0) r->frames_accum = 0;
    memcpy(r->pose, pose, sizeof(r->pose));
    return for_peers(r, [&](rt_renderer* p) { return rt_set_pose(p, pose); });
}

int rt_set_intrinsic(rt_renderer* r, const float K[9]) {
    if (!r || !K) return fail(r, RT_E_INVALID, "rt_set_intrinsic: null argument");
    if (memcmp(r->K, K, sizeof(r->K)) != 0) r->frames_accum = 0;
    memcpy(r->K, K, sizeof(r->K));
    return for_peers(r, [&](rt_renderer* p) { return rt_set_intrinsic(p, K); });
}

int rt_get_camera(const rt_renderer* r, float pose_out[16], float K_out[9]) {
    if (!r) return RT_E_INVALID;
    if (pose_out) memcpy(pose_out, r->pose, sizeof(r->pose));
    if (K_out) memcpy(K_out, r->K, sizeof(r->K));
    return RT_OK;
}

int rt_resize(rt_renderer* r, uint32_t width, uint32_t height) {
    if (!r) return fail(r, RT_E_INVALID, "rt_resize: null handle");
    if (width == 0 || height == 0 || width > 32768 || height > 32768)
        return fail(r, RT_E_INVALID, "rt_resize: width/height out of range");
    int st;
    // every queued frame that may still write the buffers released below has
    // finished first, on whichever stream it ran (a caller's, a multi-device
    // handle's comm and output streams)
    if (r->multi && (st = multi_wait(r))) return st;
    if ((st = set_device(r))) return st;
    RT_HIP(r, hipStreamSynchronize(r->stream));
    if (r->pending) RT_HIP(r, hipEventSynchronize(r->done));
    // a multi-device handle is inconsistent until every device has resized
    if (r->multi) r->multi->broken = true;
    r->W = width;
    r->H = height;
    r->frames_accum = 0;
    if ((st = ensure(r, r->fb, (size_t)width * height))) return st;
    if (r->cfg.flags & RT_FLAG_PROGRESSIVE)
        if ((st = ensure(r, r->accum, (size_t)width * height))) return st;
    if (r->cfg.flags & RT_FLAG_RADIANCE)
        if ((st = ensure(r, r->rad, (size_t)width * height))) return st;
    rt_resize_intrinsic(width, height, r->K);
    if ((st = for_peers(r, [&](rt_renderer* p) { return rt_resize(p, width, height); }))) return st;
    if (r->multi) r->multi->broken = false;  // the slabs are re-planned at the next frame
    return RT_OK;
}

int rt_render(rt_renderer* r, void* dev_rgba8, void* stream, rt_stats* stats) {
    if (!r) return fail(r, RT_E_INVALID, "rt_render: null handle");
    int st;
    // an earlier frame the kernel found incomplete: reported here, before
    // anything is queued, by a host read (no sync: the Displayer's frames
    // into a mapped PBO are never read back)
    if (r->multi) {
        if ((st = multi_queue_report(r))) return st;
    } else if ((st = queue_report(r))) {
        return st;
    }
    if ((st = set_device(r))) return st;
    // (a multi-device handle's renderers accumulate per tile list, in multi_render)
    if (!r->multi) accum_pixels(r, nullptr, 0, 0);
    FrameArgs a;
    fill_frame_args(r, a);
    a.out8 = dev_rgba8 ? static_cast<uint32_t*>(dev_rgba8) : r->fb.p;
    a.out32 = (r->cfg.flags & RT_FLAG_RADIANCE) ? r->rad.p : nullptr;
    // (a resize whose allocation failed leaves no internal framebuffer)
    if (!a.out8 || ((r->cfg.flags & RT_FLAG_RADIANCE) && !a.out32))
        return fail(r, RT_E_STATE, "rt_render: no framebuffer (a resize failed): resize again");
    const auto render_into = [&](hipStream_t hs) -> int {
        return r->multi ? multi_render(r, a.out8, hs, stats) : do_render(r, a, hs, stats);
    };
    if (dev_rgba8 || !r->disp.map) return render_into(static_cast<hipStream_t>(stream));
    // the reference's render(): map the PBO, launch into it, unmap
    // (src/renderer.cu:145-151)
    hipStream_t hs = stream ? static_cast<hipStream_t>(stream) : own_stream(r);
    if ((st = order_after_last(r, hs))) return st;
    const auto disp_fail = [&](const char* what, int e) {  // (the built-in ops' status is a hipError_t)
        std::string m = std::string("rt_render: display buffer ") + what + " failed (" + std::to_string(e) + ")";
        if (r->gl_disp) m += std::string(": ") + hipGetErrorString(static_cast<hipError_t>(e));
        return fail(r, RT_E_HIP, m);
    };
    void* ptr = nullptr;
    size_t bytes = 0;
    const int em = r->disp.map(r->disp_user, hs, &ptr, &bytes);
    if (em != 0) return disp_fail("map", em);
    if (!ptr || bytes < (size_t)r->W * r->H * 4) {
        (void)r->disp.unmap(r->disp_user, hs);
        return fail(r, RT_E_INVALID, "rt_render: display buffer smaller than W*H*4 bytes");
    }
    a.out8 = static_cast<uint32_t*>(ptr);
    st = render_into(hs);
    const int eu = r->disp.unmap(r->disp_user, hs);
    if (st) return st;
    return eu != 0 ? disp_fail("unmap", eu) : RT_OK;
}

namespace {
// built-in ops over a hipGraphicsResource_t (hipGraphicsGLRegisterBuffer);
// the status is the hipError_t
int gl_map(void* user, void* stream, void** ptr, size_t* bytes) {
    hipGraphicsResource_t res = static_cast<hipGraphicsResource_t>(user);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = hipGraphicsMapResources(1, &res, s);
    if (e != hipSuccess) return static_cast<int>(e);
    e = hipGraphicsResourceGetMappedPointer(ptr, bytes, res);
    if (e != hipSuccess) (void)hipGraphicsUnmapResources(1, &res, s);
    return static_cast<int>(e);
}
int gl_unmap(void* user, void* stream) {
    hipGraphicsResource_t res = static_cast<hipGraphicsResource_t>(user);
    return static_cast<int>(hipGraphicsUnmapResources(1, &res, static_cast<hipStream_t>(stream)));
}
}  // namespace

int rt_bind_display(rt_renderer* r, const rt_display_ops* ops, void* user) {
    if (!r) return fail(r, RT_E_INVALID, "rt_bind_display: null handle");
    if (ops && (!ops->map || !ops->unmap))
        return fail(r, RT_E_INVALID, "rt_bind_display: map and unmap are both required");
    r->disp = ops ? *ops : rt_display_ops{};
    r->disp_user = ops ? user : nullptr;
    r->gl_disp = false;
    return RT_OK;
}

int rt_bind_graphics_resource(rt_renderer* r, void* resource) {
    if (!r) return fail(r, RT_E_INVALID, "rt_bind_graphics_resource: null handle");
    static const rt_display_ops kGl = {gl_map, gl_unmap};
    const int st = rt_bind_display(r, resource ? &kGl : nullptr, resource);
    r->gl_disp = resource != nullptr;
    return st;
}

int rt_reset_accumulation(rt_renderer* r) {
    if (!r) return fail(r, RT_E_INVALID, "rt_reset_accumulation: null handle");
    r->frames_accum = 0;
    return for_peers(r, [](rt_renderer* p) { return rt_reset_accumulation(p); });
}

// After the renderer's work has completed: the wave queue's bounded wait
// (rt_kernels.hip) marks a frame whose slot was never published instead of
// hanging; every such frame not reported yet is reported now.
int rt_synchronize(rt_renderer* r) {
    if (!r) return RT_E_INVALID;
    int st;
    if (r->multi && (st = multi_synchronize(r))) return st;
    if ((st = set_device(r))) return st;
    // (a frame may have been queued on a caller's stream)
    RT_HIP(r, hipStreamSynchronize(r->stream));
    if (r->pending) RT_HIP(r, hipEventSynchronize(r->done));
    occ_collect_time(r);
    return queue_report(r);
}

int rt_readback(rt_renderer* r, uint8_t* host_rgba8, float* host_rgba32f) {
    if (const int st = rt_synchronize(r)) return st;
    const size_t px = (size_t)r->W * r->H;
    if (host_rgba8) RT_HIP(r, hipMemcpy(host_rgba8, r->fb.p, px * 4, hipMemcpyDeviceToHost));
    if (host_rgba32f) {
        if (!(r->cfg.flags & RT_FLAG_RADIANCE))
            return fail(r, RT_E_STATE, "rt_readback: radiance buffer needs RT_FLAG_RADIANCE");
        RT_HIP(r, hipMemcpy(host_rgba32f, r->rad.p, px * 16, hipMemcpyDeviceToHost));
    }
    return RT_OK;
}

void* rt_framebuffer(rt_renderer* r) { return r ? r->fb.p : nullptr; }

void* rt_stream(rt_renderer* r) { return r ? static_cast<void*>(own_stream(r)) : nullptr; }

uint32_t rt_last_instance(const rt_renderer* r) { return r ? r->last_instance : 0u; }

const char* rt_last_error(const rt_renderer* r) {
    if (r) return r->err.c_str();
    return g_last_error.c_str();
}

}  // extern "C"
