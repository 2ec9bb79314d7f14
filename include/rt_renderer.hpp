// rt_renderer.hpp — header-only C++ host surface with the reference's
// KernelRenderer method names (include/renderer.cuh:25-50), forwarding to the
// C-ABI in rt.h.  A maintainer swaps `#include "renderer.cuh"` for this header
// in Displayer (src/window/displayer.cpp, include/window/displayer.h) and
// passes glm::value_ptr(...) where the reference passed glm matrices by value.
//
// Differences from the reference, all additive:
//   * every method reports failure (throws rtamd::Error with the library's
//     message) instead of returning void silently (src/renderer.cu:143-153);
//   * render() takes the device pointer the GL PBO maps to (the caller keeps
//     hipGraphicsMapResources / hipGraphicsUnmapResources, exactly where the
//     reference calls cudaGraphicsMapResources at src/renderer.cu:145-151),
//     or nullptr for the renderer's own framebuffer;
//   * setOctree (declared but never defined in the reference,
//     include/renderer.cuh:35) is implemented, and setScene adds spheres.
#pragma once

#include <stdexcept>
#include <string>
#include <vector>

#include "rt.h"

namespace rtamd {

class Error : public std::runtime_error {
public:
    Error(int code, const std::string& msg) : std::runtime_error(msg), code(code) {}
    int code;
};

inline void check(int code, const rt_renderer* r = nullptr) {
    if (code != RT_OK) throw Error(code, rt_last_error(r));
}

class KernelRenderer {
public:
    // Reference: KernelRenderer(cudaGraphicsResource_t, int width, int height)
    // (src/renderer.cu:124-141).  The graphics resource stays with the caller.
    KernelRenderer(int width, int height, uint32_t mode = RT_MODE_COMPAT, uint32_t spp = 1,
                   int device = -1) {
        rt_config cfg;
        rt_config_default(&cfg);
        cfg.width = static_cast<uint32_t>(width);
        cfg.height = static_cast<uint32_t>(height);
        cfg.mode = mode;
        cfg.spp = spp;
        cfg.device = device;
        check(rt_create(&cfg, &r_));
    }
    // The reference's exact constructor shape (src/renderer.cu:124-141): the
    // PBO resource (registered with hipGraphicsGLRegisterBuffer) is bound, so
    // render() maps, renders into and unmaps it.
    KernelRenderer(void* graphics_resource, int width, int height, uint32_t mode = RT_MODE_COMPAT,
                   uint32_t spp = 1)
        : KernelRenderer(width, height, mode, spp) {
        setGraphicsResource(graphics_resource);
    }
    explicit KernelRenderer(const rt_config& cfg) { check(rt_create(&cfg, &r_)); }
    // One process, several GPUs (rt_create_multi): every render()
    // draws the frame across `devices` (tiles round-robin, slabs to devices[0]
    // over RCCL or peer copies, one unpack); every other method is unchanged.
    // The Displayer (src/window/displayer.cpp:28) only swaps this constructor in.
    KernelRenderer(const rt_config& cfg, const std::vector<int>& devices,
                   uint32_t transport = RT_TRANSPORT_AUTO) {
        check(rt_create_multi(&cfg, devices.data(), static_cast<uint32_t>(devices.size()), transport,
                              &r_));
    }
    rt_multi_info multiInfo() const {
        rt_multi_info i;
        check(rt_get_multi_info(r_, &i), r_);
        return i;
    }
    ~KernelRenderer() { rt_destroy(r_); }
    KernelRenderer(const KernelRenderer&) = delete;
    KernelRenderer& operator=(const KernelRenderer&) = delete;

    // render() (src/renderer.cu:143-153): dev_rgba8 = mapped PBO pointer.
    void render(void* dev_rgba8 = nullptr, void* stream = nullptr, rt_stats* stats = nullptr) {
        check(rt_render(r_, dev_rgba8, stream, stats), r_);
    }
    // the reference assigns renderer->cudaResource after re-registering the
    // resized PBO (src/window/displayer.cpp:61-70)
    void setGraphicsResource(void* graphics_resource) {
        check(rt_bind_graphics_resource(r_, graphics_resource), r_);
    }
    // any toolkit's display buffer: render() maps, fills and unmaps it per
    // frame through `ops` (rt_bind_display; nullptr unbinds)
    void setDisplay(const rt_display_ops* ops, void* user) { check(rt_bind_display(r_, ops, user), r_); }
    // resize(int, int) (src/renderer.cu:155-187)
    void resize(int width, int height) {
        check(rt_resize(r_, static_cast<uint32_t>(width), static_cast<uint32_t>(height)), r_);
    }
    // setPosition(glm::mat4) (src/renderer.cu:111-113): pass glm::value_ptr(pose)
    void setPosition(const float* pose_colmajor16) { check(rt_set_pose(r_, pose_colmajor16), r_); }
    // setIntrinsic(glm::mat3) (src/renderer.cu:115-117): pass glm::value_ptr(K)
    void setIntrinsic(const float* K_colmajor9) { check(rt_set_intrinsic(r_, K_colmajor9), r_); }
    // setOctree(glm::vec3 min, glm::vec3 max, float resolution) (include/renderer.cuh:35)
    void setOctree(const float* min3, const float* max3, float resolution) {
        check(rt_set_octree(r_, min3, max3, resolution), r_);
    }
    // new: spheres (cx, cy, cz, r) x n, optional RGBA8 albedo
    void setScene(const std::vector<float>& spheres, const std::vector<uint32_t>& albedo = {},
                  const rt_octree_params* oct = nullptr) {
        const uint32_t n = static_cast<uint32_t>(spheres.size() / 4);
        check(rt_set_scene(r_, spheres.data(), albedo.empty() ? nullptr : albedo.data(), n, oct),
              r_);
    }
    // new: sphere list already in device memory (built into an octree on the GPU)
    void setSceneDevice(const void* dev_spheres, uint32_t n, const void* dev_albedo = nullptr,
                        const rt_octree_params* oct = nullptr, void* stream = nullptr) {
        check(rt_set_scene_device(r_, dev_spheres, dev_albedo, n, oct, stream), r_);
    }
    // new: binary sphere file (rt_save_spheres format)
    void setSceneFile(const std::string& path, const rt_octree_params* oct = nullptr) {
        std::vector<float> sp;
        std::vector<uint32_t> al;
        loadSpheres(path, sp, al);
        setScene(sp, al, oct);
    }
    static void loadSpheres(const std::string& path, std::vector<float>& spheres,
                            std::vector<uint32_t>& albedo) {
        uint32_t n = 0;
        check(rt_load_spheres(path.c_str(), nullptr, nullptr, 0, &n));
        spheres.resize(4 * size_t(n));
        albedo.resize(n);
        check(rt_load_spheres(path.c_str(), spheres.data(), albedo.data(), n, &n));
    }
    static void saveSpheres(const std::string& path, const std::vector<float>& spheres,
                            const std::vector<uint32_t>& albedo = {}) {
        check(rt_save_spheres(path.c_str(), spheres.data(), albedo.empty() ? nullptr : albedo.data(),
                              static_cast<uint32_t>(spheres.size() / 4)));
    }
    // multi-GPU: render only the listed 64x64 tiles into a packed device slab
    // (rt_render_tiles), and scatter packed slabs into a frame (rt_unpack_tiles)
    void renderTiles(const std::vector<uint32_t>& ids, uint32_t tile_size, void* dev_packed,
                     void* stream = nullptr, rt_stats* stats = nullptr) {
        check(rt_render_tiles(r_, ids.data(), static_cast<uint32_t>(ids.size()), tile_size,
                              dev_packed, stream, stats),
              r_);
    }
    void unpackTiles(const void* dev_packed, const std::vector<uint32_t>& ids, uint32_t tile_size,
                     void* dev_rgba8 = nullptr, void* stream = nullptr) {
        check(rt_unpack_tiles(r_, dev_packed, ids.data(), static_cast<uint32_t>(ids.size()),
                              tile_size, dev_rgba8, stream),
              r_);
    }
    // ray queries against the scene octree (rt_trace_rays): n rt_ray in device
    // memory -> n rt_hit in device memory; kind RT_QUERY_NEAREST / RT_QUERY_ANY
    void traceRays(const void* dev_rays, uint32_t n, void* dev_hits,
                   uint32_t kind = RT_QUERY_NEAREST, void* stream = nullptr,
                   rt_stats* stats = nullptr) {
        check(rt_trace_rays(r_, dev_rays, n, kind, dev_hits, stream, stats), r_);
    }
    // the nearest sphere under image coordinates (u, v), e.g. the Displayer's
    // mouse position (rt_pick); false on a miss.  point3: origin + t * dir, or null
    bool pick(float u, float v, rt_hit* hit = nullptr, float* point3 = nullptr) {
        rt_hit h;
        check(rt_pick(r_, u, v, &h, point3), r_);
        if (hit) *hit = h;
        return h.sphere != RT_NO_HIT;
    }
    // the k nearest spheres along each ray, by (t, sphere index)
    // (rt_trace_rays_multi): n rt_ray -> n*k rt_hit, ray-major, and n uint32
    // counts (or null), all in device memory; 1 <= k <= RT_MULTIHIT_MAX
    void traceRaysMulti(const void* dev_rays, uint32_t n, uint32_t k, void* dev_hits,
                        void* dev_counts = nullptr, void* stream = nullptr,
                        rt_stats* stats = nullptr) {
        check(rt_trace_rays_multi(r_, dev_rays, n, k, dev_hits, dev_counts, stream, stats), r_);
    }
    // the k nearest spheres under image coordinates (u, v), front to back
    // (rt_pick_multi): a repeated click selects hits[1], hits[2], ...; returns
    // how many of hits[0 .. k) are spheres
    uint32_t pickMulti(float u, float v, uint32_t k, rt_hit* hits) {
        uint32_t count = 0;
        check(rt_pick_multi(r_, u, v, k, hits, &count), r_);
        return count;
    }
    // the scene spheres each probe sphere touches (rt_query_overlaps): n rt_probe
    // -> n*k sphere indices, probe-major, the k smallest ascending, and n count
    // words (or null; RT_OVERLAP_MORE: the set is larger), all in device memory;
    // 1 <= k <= RT_OVERLAP_MAX; flags RT_OVERLAP_SKIP_SELF
    void queryOverlaps(const void* dev_probes, uint32_t n, uint32_t k, void* dev_indices,
                       void* dev_counts = nullptr, uint32_t flags = 0, void* stream = nullptr,
                       rt_stats* stats = nullptr) {
        check(rt_query_overlaps(r_, dev_probes, n, k, flags, dev_indices, dev_counts, stream, stats), r_);
    }
    // the scene spheres within `radius` of a point, e.g. a brush around pick()'s
    // point (rt_overlaps_at); returns how many of indices[0 .. k) are spheres,
    // *more (may be null): the set is larger than k
    uint32_t overlapsAt(const float center[3], float radius, uint32_t k, uint32_t* indices,
                        bool* more = nullptr) {
        uint32_t count = 0;
        check(rt_overlaps_at(r_, center, radius, k, indices, &count), r_);
        if (more) *more = (count & RT_OVERLAP_MORE) != 0;
        return count & ~RT_OVERLAP_MORE;
    }
    // the k scene spheres nearest each probe point within its search radius, by
    // (signed surface distance, sphere index) (rt_query_closest): n rt_probe ->
    // n*k rt_near, probe-major, and n uint32 counts (or null), all in device
    // memory; 1 <= k <= RT_CLOSEST_MAX; flags RT_CLOSEST_SKIP_SELF
    void queryClosest(const void* dev_probes, uint32_t n, uint32_t k, void* dev_near,
                      void* dev_counts = nullptr, uint32_t flags = 0, void* stream = nullptr,
                      rt_stats* stats = nullptr) {
        check(rt_query_closest(r_, dev_probes, n, k, flags, dev_near, dev_counts, stream, stats), r_);
    }
    // the k spheres nearest a point within max_dist (INFINITY: unbounded), e.g. to
    // snap a click that pick() missed (rt_closest_at); returns how many of
    // near[0 .. k) are spheres
    uint32_t closestAt(const float point[3], float max_dist, uint32_t k, rt_near* near) {
        uint32_t count = 0;
        check(rt_closest_at(r_, point, max_dist, k, near, &count), r_);
        return count;
    }
    // the first sphere a ball of radius R touches while its centre moves along
    // each ray (rt_sweep_spheres): n rt_ray and n radii (or null: every cast
    // uses `radius`) -> n rt_hit, all in device memory; `dir` of unit length;
    // flags RT_SWEEP_ENTRY_ONLY | RT_SWEEP_SKIP_SELF
    void sweepSpheres(const void* dev_rays, uint32_t n, float radius, void* dev_hits,
                      const void* dev_radii = nullptr, uint32_t flags = 0, void* stream = nullptr,
                      rt_stats* stats = nullptr) {
        check(rt_sweep_spheres(r_, dev_rays, dev_radii, radius, n, flags, dev_hits, stream, stats), r_);
    }
    // one cast from `origin` along the unit `dir` up to tmax, e.g. a time of
    // impact (rt_sweep_at); point (may be null): the ball's centre at contact
    rt_hit sweepAt(const float origin[3], const float dir[3], float radius, float tmax, uint32_t flags = 0,
                   float point[3] = nullptr) {
        rt_hit h{};
        check(rt_sweep_at(r_, origin, dir, radius, tmax, flags, &h, point), r_);
        return h;
    }
    // pick() with a cursor of finite radius (rt_pick_thick)
    rt_hit pickThick(float u, float v, float radius, float point[3] = nullptr) {
        rt_hit h{};
        check(rt_pick_thick(r_, u, v, radius, &h, point), r_);
        return h;
    }
    // first-hit G-buffer of the current camera (rt_render_gbuffer): W*H rt_hit,
    // float[4] normals and packed RGBA8 albedo in device memory, each optional
    void renderGBuffer(void* dev_hits, void* dev_normals = nullptr, void* dev_albedo = nullptr,
                       void* stream = nullptr, rt_stats* stats = nullptr) {
        const rt_gbuffer g{dev_hits, dev_normals, dev_albedo};
        check(rt_render_gbuffer(r_, &g, stream, stats), r_);
    }
    // ambient-occlusion layer of the current camera (rt_render_ao): `rays` (1, 2,
    // .. 64) any-hit rays of length `radius` from every hit pixel; W*H float
    // (1 = open) and W*H uint32 occluded counts in device memory, each optional
    void renderAO(uint32_t rays, float radius, void* dev_ao, void* dev_occluded = nullptr, uint32_t salt = 0,
                  void* stream = nullptr, rt_stats* stats = nullptr) {
        const rt_ao_params p{rays, radius, salt, 0u};
        const rt_ao_out o{dev_ao, dev_occluded};
        check(rt_render_ao(r_, &p, &o, stream, stats), r_);
    }
    // one-bounce diffuse light layer of the current camera (rt_render_indirect):
    // renderAO's rays to their nearest hits, each shaded as a frame shades it; W*H
    // float[4] {r, g, b, open share} and W*H uint32 hit counts in device memory,
    // each optional
    void renderIndirect(uint32_t rays, float radius, void* dev_layer, void* dev_occluded = nullptr, uint32_t salt = 0,
                        float sky_scale = 1.0f, void* stream = nullptr, rt_stats* stats = nullptr) {
        const rt_indirect_params p{rays, radius, salt, sky_scale, 0u};
        const rt_indirect_out o{dev_layer, dev_occluded};
        check(rt_render_indirect(r_, &p, &o, stream, stats), r_);
    }
    // a W*H float[4] layer added into RGBA8 pixels in place (rt_add_layer), times
    // gain and, with renderGBuffer's albedo, the pixel's albedo; dev_rgba8 null: the
    // internal framebuffer
    void addLayer(const void* dev_layer4, float gain = 1.0f, const void* dev_albedo = nullptr,
                  void* dev_rgba8 = nullptr, void* stream = nullptr) {
        check(rt_add_layer(r_, dev_rgba8, dev_layer4, dev_albedo, gain, stream), r_);
    }
    // guide-driven filter of a per-pixel layer (rt_filter_layer): W*H*channels floats
    // from dev_in to dev_out, steered by renderGBuffer's hits and normals
    void filterLayer(const void* dev_in, void* dev_out, const void* dev_hits, const void* dev_normals,
                     uint32_t passes = 3, uint32_t channels = 1, float depth_sigma = 0.05f,
                     uint32_t normal_power = 5, void* stream = nullptr, rt_stats* stats = nullptr) {
        const rt_filter_params p{passes, channels, depth_sigma, normal_power, 0u};
        const rt_gbuffer g{const_cast<void*>(dev_hits), const_cast<void*>(dev_normals), nullptr};
        check(rt_filter_layer(r_, &p, &g, dev_in, dev_out, stream, stats), r_);
    }
    // a W*H float layer multiplied into RGBA8 pixels in place (rt_apply_layer):
    // m = floor + (1 - floor) * layer; dev_rgba8 null: the internal framebuffer
    void applyLayer(const void* dev_layer, float floor = 0.0f, void* dev_rgba8 = nullptr, void* stream = nullptr) {
        check(rt_apply_layer(r_, dev_rgba8, dev_layer, floor, stream), r_);
    }
    // a layer carried across camera motion (rt_reproject_layer): this frame's layer
    // dev_cur blended with the previous frame's mean, reprojected into the current
    // camera; hist null: no history (first frame, after a resize or a scene change)
    void reprojectLayer(const void* dev_hits, const rt_history* hist, const void* dev_cur, void* dev_out,
                        void* dev_count_out, uint32_t channels = 1, float max_count = 32.0f, float depth_tol = 0.05f,
                        void* stream = nullptr, rt_stats* stats = nullptr) {
        const rt_reproject_params p{channels, max_count, depth_tol, 0u};
        check(rt_reproject_layer(r_, &p, dev_hits, hist, dev_cur, dev_out, dev_count_out, stream, stats), r_);
    }
    rt_scene_info sceneInfo() const {
        rt_scene_info i;
        check(rt_get_scene_info(r_, &i), r_);
        return i;
    }
    // the last frame's tile words (rt_export_bin_tiles): bins * tiles-per-bin
    // words, and that frame's wave tile in pixels
    std::vector<uint64_t> exportBinTiles(uint32_t* tw = nullptr, uint32_t* th = nullptr) {
        rt_bin_info bi;
        uint32_t tpb = 0;
        check(rt_get_bin_info(r_, &bi), r_);
        check(rt_export_bin_tiles(r_, tw, th, &tpb, nullptr), r_);
        std::vector<uint64_t> words(static_cast<size_t>(bi.bins) * tpb);
        check(rt_export_bin_tiles(r_, nullptr, nullptr, nullptr, words.data()), r_);
        return words;
    }
    void readback(uint8_t* host_rgba8, float* host_rgba32f = nullptr) {
        check(rt_readback(r_, host_rgba8, host_rgba32f), r_);
    }
    void synchronize() { check(rt_synchronize(r_), r_); }
    rt_renderer* handle() { return r_; }

private:
    rt_renderer* r_ = nullptr;
};

}  // namespace rtamd
