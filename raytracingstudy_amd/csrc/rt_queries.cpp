// rt_queries.cpp — the calls that read a scene without rendering a frame
// (DESIGN.md 5.7): ray, multi-hit, sphere-overlap, closest-sphere and
// swept-sphere queries, their single-item wrappers, the first-hit G-buffer, the
// ambient-occlusion layer and the one-bounce diffuse layer.  The reference has none
// (Octree::traverse is a stub, include/octree.h:19-21; its render kernel
// writes one colour per pixel, src/renderer.cu:57-82).  A query reads scene
// (the G-buffer and the AO layer: and camera) state only: it takes no frame id, leaves the
// progressive sums, the frames' counter sets and the qerr word alone, and is
// ordered after the handle's earlier work like every launch.  Each entry point
// checks its own arguments in its own order (rt.h states the codes); what
// follows the checks is stated once, in query_begin and query_launch.  The
// layer calls at the end (rt_filter_layer, rt_apply_layer; DESIGN.md 5.16;
// rt_add_layer, 5.18; rt_reproject_layer, 5.17) read no scene at all, only the handle's size and,
// the last, its camera; they share the stream ordering and the stats bracket.
#include "rt_ao_math.h"
#include "rt_filter_math.h"
#include "rt_host.h"
#include "rt_indirect_math.h"

using namespace rtamd;

namespace {

// The device, the stream (the caller's, or the handle's own) and the ordering
// after the handle's last work (stream_begin: all the layer calls need), and
// the query kernels' leading argument: a FrameArgs
// (kernargs() reinterprets the argument segment as one, rt_query.hip) holding
// the scene, the rest zero.
int stream_begin(rt_renderer* r, void* stream, hipStream_t& hs) {
    int st;
    if ((st = set_device(r))) return st;
    hs = stream ? static_cast<hipStream_t>(stream) : own_stream(r);
    return order_after_last(r, hs);
}
int query_begin(rt_renderer* r, void* stream, hipStream_t& hs, FrameArgs& a) {
    int st;
    if ((st = stream_begin(r, stream, hs))) return st;
    memset(&a, 0, sizeof(a));
    a.sc = r->sc;
    return RT_OK;
}

// The query path's own stat lines (a stats launch never touches the frames'
// counter sets): zeroed on `hs` with the start event behind them; after the
// launch and the end event, read back into `stats` (nodes, tests and ms).
int query_stats_begin(rt_renderer* r, hipStream_t hs, unsigned long long*& ctr) {
    int st;
    if ((st = ensure(r, r->q.counters, kStatLineWords))) return st;
    ctr = r->q.counters.p;
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

// launch(ctr) on `hs`, ctr the stat lines of a stats launch or null: between
// the stats bracket when `stats` is given, and marked as the handle's last
// work.  The caller adds its ray count to `stats`.
template <typename Launch>
int query_launch(rt_renderer* r, const char* api, hipStream_t hs, rt_stats* stats, Launch launch) {
    int st;
    unsigned long long* ctr = nullptr;
    if (stats && (st = query_stats_begin(r, hs, ctr))) return st;
    hipError_t e = launch(ctr);
    if (e != hipSuccess) return hip_fail(r, e, (std::string(api) + ": kernel launch").c_str());
    if (stats) RT_HIP(r, hipEventRecord(r->ev1, hs));
    if ((st = mark_queued(r, hs))) return st;
    return stats ? query_stats_read(r, ctr, stats) : RT_OK;
}

// n == 0: nothing to do, and a stats call reports nothing done
int nothing_queried(rt_stats* stats) {
    if (stats) memset(stats, 0, sizeof(*stats));
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

// One cast (rt_sweep_at, rt_pick_thick; the caller checked its arguments):
// uploads the ray, sweeps it on the handle's own stream and waits.  hit_out as
// rt_sweep_spheres writes it; point_out (may be null) = origin + t * dir.
int sweep_one(rt_renderer* r, const float4 ray[2], float radius, uint32_t flags, rt_hit* hit_out,
              float point_out[3]) {
    int st;
    if ((st = set_device(r))) return st;
    if ((st = ensure(r, r->q.cast, 2)) || (st = ensure(r, r->q.cast_hit, 1))) return st;
    hipStream_t hs = own_stream(r);
    if ((st = order_after_last(r, hs))) return st;
    RT_HIP(r, hipMemcpyAsync(r->q.cast.p, ray, 2 * sizeof(float4), hipMemcpyHostToDevice, hs));
    if ((st = rt_sweep_spheres(r, r->q.cast.p, nullptr, radius, 1, flags, r->q.cast_hit.p, hs, nullptr)))
        return st;
    uint2 h;
    RT_HIP(r, hipMemcpyAsync(&h, r->q.cast_hit.p, sizeof(h), hipMemcpyDeviceToHost, hs));
    RT_HIP(r, hipStreamSynchronize(hs));
    memcpy(&hit_out->t, &h.x, sizeof(float));
    hit_out->sphere = h.y;
    if (point_out) {
        const float o[3] = {ray[0].x, ray[0].y, ray[0].z}, d[3] = {ray[1].x, ray[1].y, ray[1].z};
        for (int i = 0; i < 3; ++i) point_out[i] = o[i] + hit_out->t * d[i];
    }
    return RT_OK;
}

}  // namespace

// The four single-item wrappers below (rt_pick, rt_pick_multi, rt_overlaps_at,
// rt_closest_at; the two one-cast calls share sweep_one above) stay plain functions: their scratch buffers and copies back
// differ in number and type, so a shared helper could hold only "order, upload
// one record" (three lines of each), would need the rest passed in as two
// callbacks, and would be no shorter than what it replaces.
extern "C" {

int rt_trace_rays(rt_renderer* r, const void* dev_rays, uint32_t n, uint32_t kind, void* dev_hits,
                  void* stream, rt_stats* stats) {
    if (!r) return fail(r, RT_E_INVALID, "rt_trace_rays: null handle");
    if (kind != RT_QUERY_NEAREST && kind != RT_QUERY_ANY)
        return fail(r, RT_E_INVALID, "rt_trace_rays: unknown query kind");
    if (!r->has_scene) return fail(r, RT_E_NOSCENE, "rt_trace_rays: no scene (rt_set_scene first)");
    if (n == 0) return nothing_queried(stats);
    if (!dev_rays || !dev_hits) return fail(r, RT_E_INVALID, "rt_trace_rays: null buffer");
    hipStream_t hs;
    FrameArgs a;
    int st;
    if ((st = query_begin(r, stream, hs, a))) return st;
    st = query_launch(r, "rt_trace_rays", hs, stats, [&](unsigned long long* ctr) {
        return launch_query(a, dev_rays, dev_hits, n, kind == RT_QUERY_ANY, ctr, hs);
    });
    if (!st && stats) (kind == RT_QUERY_ANY ? stats->shadow_rays : stats->primary_rays) = n;
    return st;
}

int rt_pick(rt_renderer* r, float u, float v, rt_hit* hit_out, float point_out[3]) {
    if (!r || !hit_out) return fail(r, RT_E_INVALID, "rt_pick: null argument");
    if (!r->has_scene) return fail(r, RT_E_NOSCENE, "rt_pick: no scene (rt_set_scene first)");
    float4 ray[2];
    pick_ray(r, u, v, ray);
    int st;
    if ((st = set_device(r))) return st;
    if ((st = ensure(r, r->q.ray, 2)) || (st = ensure(r, r->q.hit, 1))) return st;
    hipStream_t hs = own_stream(r);
    if ((st = order_after_last(r, hs))) return st;
    RT_HIP(r, hipMemcpyAsync(r->q.ray.p, ray, sizeof(ray), hipMemcpyHostToDevice, hs));
    if ((st = rt_trace_rays(r, r->q.ray.p, 1, RT_QUERY_NEAREST, r->q.hit.p, hs, nullptr))) return st;
    uint2 h;
    RT_HIP(r, hipMemcpyAsync(&h, r->q.hit.p, sizeof(h), hipMemcpyDeviceToHost, hs));
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
// by (t, sphere index).
int rt_trace_rays_multi(rt_renderer* r, const void* dev_rays, uint32_t n, uint32_t k, void* dev_hits,
                        void* dev_counts, void* stream, rt_stats* stats) {
    if (!r) return fail(r, RT_E_INVALID, "rt_trace_rays_multi: null handle");
    if (k == 0 || k > RT_MULTIHIT_MAX)
        return fail(r, RT_E_INVALID, "rt_trace_rays_multi: k must be 1 .. RT_MULTIHIT_MAX");
    if (!r->has_scene)
        return fail(r, RT_E_NOSCENE, "rt_trace_rays_multi: no scene (rt_set_scene first)");
    if (n == 0) return nothing_queried(stats);
    if (!dev_rays || !dev_hits) return fail(r, RT_E_INVALID, "rt_trace_rays_multi: null buffer");
    hipStream_t hs;
    FrameArgs a;
    int st;
    if ((st = query_begin(r, stream, hs, a))) return st;
    st = query_launch(r, "rt_trace_rays_multi", hs, stats, [&](unsigned long long* ctr) {
        return launch_multihit(a, dev_rays, dev_hits, dev_counts, n, k, ctr, hs);
    });
    if (!st && stats) stats->primary_rays = n;
    return st;
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
    if ((st = ensure(r, r->q.ray, 2)) || (st = ensure(r, r->q.multi_hits, RT_MULTIHIT_MAX)) ||
        (st = ensure(r, r->q.multi_count, 1)))
        return st;
    hipStream_t hs = own_stream(r);
    if ((st = order_after_last(r, hs))) return st;
    RT_HIP(r, hipMemcpyAsync(r->q.ray.p, ray, sizeof(ray), hipMemcpyHostToDevice, hs));
    if ((st = rt_trace_rays_multi(r, r->q.ray.p, 1, k, r->q.multi_hits.p, r->q.multi_count.p, hs, nullptr)))
        return st;
    uint2 h[RT_MULTIHIT_MAX];
    uint32_t count = 0;
    RT_HIP(r, hipMemcpyAsync(h, r->q.multi_hits.p, k * sizeof(uint2), hipMemcpyDeviceToHost, hs));
    RT_HIP(r, hipMemcpyAsync(&count, r->q.multi_count.p, sizeof(count), hipMemcpyDeviceToHost, hs));
    RT_HIP(r, hipStreamSynchronize(hs));
    for (uint32_t s = 0; s < k; ++s) {
        memcpy(&hits_out[s].t, &h[s].x, sizeof(float));
        hits_out[s].sphere = h[s].y;
    }
    if (count_out) *count_out = count;
    return RT_OK;
}

// Sphere-overlap queries: the scene spheres each probe sphere
// touches, the k smallest indices.
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
    if (n == 0) return nothing_queried(stats);
    hipStream_t hs;
    FrameArgs a;
    if (const int st = query_begin(r, stream, hs, a)) return st;
    const float slack_m = overlap_slack_m(r->info.root_min, r->info.root_max);
    // (no rays: both ray counts stay 0)
    return query_launch(r, "rt_query_overlaps", hs, stats, [&](unsigned long long* ctr) {
        return launch_overlap(a, dev_probes, dev_indices, dev_counts, n, k,
                              (flags & RT_OVERLAP_SKIP_SELF) != 0, slack_m, ctr, hs);
    });
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
    if ((st = ensure(r, r->q.probe, 1)) || (st = ensure(r, r->q.overlap_idx, RT_OVERLAP_MAX)) ||
        (st = ensure(r, r->q.overlap_count, 1)))
        return st;
    hipStream_t hs = own_stream(r);
    if ((st = order_after_last(r, hs))) return st;
    RT_HIP(r, hipMemcpyAsync(r->q.probe.p, &probe, sizeof(probe), hipMemcpyHostToDevice, hs));
    if ((st = rt_query_overlaps(r, r->q.probe.p, 1, k, 0, r->q.overlap_idx.p, r->q.overlap_count.p, hs,
                                nullptr)))
        return st;
    uint32_t idx[RT_OVERLAP_MAX], count = 0;
    RT_HIP(r, hipMemcpyAsync(idx, r->q.overlap_idx.p, k * sizeof(uint32_t), hipMemcpyDeviceToHost, hs));
    RT_HIP(r, hipMemcpyAsync(&count, r->q.overlap_count.p, sizeof(count), hipMemcpyDeviceToHost, hs));
    RT_HIP(r, hipStreamSynchronize(hs));
    memcpy(indices_out, idx, k * sizeof(uint32_t));
    if (count_out) *count_out = count;
    return RT_OK;
}

// Closest-sphere queries: the k scene spheres whose surfaces
// are nearest each probe point, within its search radius.
int rt_query_closest(rt_renderer* r, const void* dev_probes, uint32_t n, uint32_t k, uint32_t flags,
                     void* dev_near, void* dev_counts, void* stream, rt_stats* stats) {
    if (!r) return fail(r, RT_E_INVALID, "rt_query_closest: null handle");
    if (k == 0 || k > RT_CLOSEST_MAX)
        return fail(r, RT_E_INVALID, "rt_query_closest: k must be 1 .. RT_CLOSEST_MAX");
    if (flags & ~static_cast<uint32_t>(RT_CLOSEST_SKIP_SELF))
        return fail(r, RT_E_INVALID, "rt_query_closest: unknown flag bits");
    if (n > 0 && (!dev_probes || !dev_near)) return fail(r, RT_E_INVALID, "rt_query_closest: null buffer");
    if (!r->has_scene) return fail(r, RT_E_NOSCENE, "rt_query_closest: no scene (rt_set_scene first)");
    if (n == 0) return nothing_queried(stats);
    hipStream_t hs;
    FrameArgs a;
    if (const int st = query_begin(r, stream, hs, a)) return st;
    const float slack_m = closest_slack_m(r->info.root_min, r->info.root_max);
    // (no rays: both ray counts stay 0)
    return query_launch(r, "rt_query_closest", hs, stats, [&](unsigned long long* ctr) {
        return launch_closest(a, dev_probes, dev_near, dev_counts, n, k, (flags & RT_CLOSEST_SKIP_SELF) != 0,
                              slack_m, ctr, hs);
    });
}

int rt_closest_at(rt_renderer* r, const float point[3], float max_dist, uint32_t k, rt_near* near_out,
                  uint32_t* count_out) {
    if (!r || !point || !near_out) return fail(r, RT_E_INVALID, "rt_closest_at: null argument");
    if (k == 0 || k > RT_CLOSEST_MAX)
        return fail(r, RT_E_INVALID, "rt_closest_at: k must be 1 .. RT_CLOSEST_MAX");
    if (!r->has_scene) return fail(r, RT_E_NOSCENE, "rt_closest_at: no scene (rt_set_scene first)");
    const float4 probe = make_float4(point[0], point[1], point[2], max_dist);
    int st;
    if ((st = set_device(r))) return st;
    if ((st = ensure(r, r->q.probe, 1)) || (st = ensure(r, r->q.near, RT_CLOSEST_MAX)) ||
        (st = ensure(r, r->q.near_count, 1)))
        return st;
    hipStream_t hs = own_stream(r);
    if ((st = order_after_last(r, hs))) return st;
    RT_HIP(r, hipMemcpyAsync(r->q.probe.p, &probe, sizeof(probe), hipMemcpyHostToDevice, hs));
    if ((st = rt_query_closest(r, r->q.probe.p, 1, k, 0, r->q.near.p, r->q.near_count.p, hs, nullptr)))
        return st;
    uint2 h[RT_CLOSEST_MAX];
    uint32_t count = 0;
    RT_HIP(r, hipMemcpyAsync(h, r->q.near.p, k * sizeof(uint2), hipMemcpyDeviceToHost, hs));
    RT_HIP(r, hipMemcpyAsync(&count, r->q.near_count.p, sizeof(count), hipMemcpyDeviceToHost, hs));
    RT_HIP(r, hipStreamSynchronize(hs));
    for (uint32_t s = 0; s < k; ++s) {
        memcpy(&near_out[s].dist, &h[s].x, sizeof(float));
        near_out[s].sphere = h[s].y;
    }
    if (count_out) *count_out = count;
    return RT_OK;
}

// Swept-sphere queries: the first scene sphere a ball of
// radius R touches while its centre moves along each ray.
int rt_sweep_spheres(rt_renderer* r, const void* dev_rays, const void* dev_radii, float radius, uint32_t n,
                     uint32_t flags, void* dev_hits, void* stream, rt_stats* stats) {
    if (!r) return fail(r, RT_E_INVALID, "rt_sweep_spheres: null handle");
    if (flags & ~static_cast<uint32_t>(RT_SWEEP_ENTRY_ONLY | RT_SWEEP_SKIP_SELF))
        return fail(r, RT_E_INVALID, "rt_sweep_spheres: unknown flag bits");
    if (n > 0 && (!dev_rays || !dev_hits)) return fail(r, RT_E_INVALID, "rt_sweep_spheres: null buffer");
    if (!r->has_scene) return fail(r, RT_E_NOSCENE, "rt_sweep_spheres: no scene (rt_set_scene first)");
    if (n == 0) return nothing_queried(stats);
    hipStream_t hs;
    FrameArgs a;
    int st;
    if ((st = query_begin(r, stream, hs, a))) return st;
    const float slack_m = sweep_slack_m(r->info.root_min, r->info.root_max);
    st = query_launch(r, "rt_sweep_spheres", hs, stats, [&](unsigned long long* ctr) {
        return launch_sweep(a, dev_rays, dev_radii, radius, dev_hits, n, (flags & RT_SWEEP_ENTRY_ONLY) != 0,
                            (flags & RT_SWEEP_SKIP_SELF) != 0, slack_m, ctr, hs);
    });
    if (!st && stats) stats->primary_rays = n;
    return st;
}

int rt_sweep_at(rt_renderer* r, const float origin[3], const float dir[3], float radius, float tmax,
                uint32_t flags, rt_hit* hit_out, float point_out[3]) {
    if (!r || !origin || !dir || !hit_out) return fail(r, RT_E_INVALID, "rt_sweep_at: null argument");
    if (flags & ~static_cast<uint32_t>(RT_SWEEP_ENTRY_ONLY | RT_SWEEP_SKIP_SELF))
        return fail(r, RT_E_INVALID, "rt_sweep_at: unknown flag bits");
    if (!r->has_scene) return fail(r, RT_E_NOSCENE, "rt_sweep_at: no scene (rt_set_scene first)");
    const float4 ray[2] = {make_float4(origin[0], origin[1], origin[2], 0.0f),
                           make_float4(dir[0], dir[1], dir[2], tmax)};
    return sweep_one(r, ray, radius, flags, hit_out, point_out);
}

int rt_pick_thick(rt_renderer* r, float u, float v, float radius, rt_hit* hit_out, float point_out[3]) {
    if (!r || !hit_out) return fail(r, RT_E_INVALID, "rt_pick_thick: null argument");
    if (!r->has_scene) return fail(r, RT_E_NOSCENE, "rt_pick_thick: no scene (rt_set_scene first)");
    float4 ray[2];
    pick_ray(r, u, v, ray);
    return sweep_one(r, ray, radius, 0, hit_out, point_out);
}

// First-hit G-buffer of the current camera: no
// fill_frame_args (which advances the frame id and the sums), nothing of the
// frames' framebuffer.
int rt_render_gbuffer(rt_renderer* r, const rt_gbuffer* out, void* stream, rt_stats* stats) {
    if (!r) return fail(r, RT_E_INVALID, "rt_render_gbuffer: null handle");
    if (!out || (!out->dev_hits && !out->dev_normals && !out->dev_albedo))
        return fail(r, RT_E_INVALID, "rt_render_gbuffer: no output buffer");
    if (!r->has_scene) return fail(r, RT_E_NOSCENE, "rt_render_gbuffer: no scene (rt_set_scene first)");
    hipStream_t hs;
    FrameArgs a;
    int st;
    if ((st = query_begin(r, stream, hs, a))) return st;
    // ... and the camera and size (rt_gbuffer.hip)
    fill_camera(r, a.cam);
    a.W = r->W;
    a.H = r->H;
    // the frames' own albedo table: whichever of the two runs first makes it,
    // here ahead of the stats bracket (its launch is not the G-buffer's time)
    if (out->dev_albedo && (st = ensure_prim_al(r, a.sc, hs))) return st;
    st = query_launch(r, "rt_render_gbuffer", hs, stats, [&](unsigned long long* ctr) {
        return launch_gbuffer(a, out->dev_hits, out->dev_normals, out->dev_albedo, ctr, hs);
    });
    if (!st && stats) stats->primary_rays = static_cast<uint64_t>(r->W) * r->H;
    return st;
}

// The ambient-occlusion layer of the current camera: like the
// G-buffer, no fill_frame_args and nothing of the frames' framebuffer.
int rt_render_ao(rt_renderer* r, const rt_ao_params* p, const rt_ao_out* out, void* stream, rt_stats* stats) {
    if (!r) return fail(r, RT_E_INVALID, "rt_render_ao: null handle");
    if (!p) return fail(r, RT_E_INVALID, "rt_render_ao: null parameters");
    if (!out || (!out->dev_ao && !out->dev_occluded))
        return fail(r, RT_E_INVALID, "rt_render_ao: no output buffer");
    if (!ao_rays_ok(p->rays)) return fail(r, RT_E_INVALID, "rt_render_ao: rays must be 1, 2, 4, 8, 16, 32 or 64");
    if (!ao_radius_ok(p->radius)) return fail(r, RT_E_INVALID, "rt_render_ao: radius must be > 0");
    if (p->flags) return fail(r, RT_E_INVALID, "rt_render_ao: unknown flag bits");
    if (!r->has_scene) return fail(r, RT_E_NOSCENE, "rt_render_ao: no scene (rt_set_scene first)");
    hipStream_t hs;
    FrameArgs a;
    int st;
    if ((st = query_begin(r, stream, hs, a))) return st;
    fill_camera(r, a.cam);
    a.W = r->W;
    a.H = r->H;
    // the frames' seed word (fill_frame_args' seedmix) under the caller's salt
    const uint32_t key = ao_key(mix32(r->cfg.seed ^ 0x9E3779B9u), p->salt);
    st = query_launch(r, "rt_render_ao", hs, stats, [&](unsigned long long* ctr) {
        return launch_ao(a, out->dev_ao, out->dev_occluded, p->rays, p->radius, key, ctr, hs);
    });
    if (!st && stats) {
        stats->primary_rays = static_cast<uint64_t>(r->W) * r->H;
        // the AO rays cast (rays x hit pixels) are the kernel's count, word 1 of the stat lines
        // query_launch just read (the stats path has waited for the launch); no other query writes it
        unsigned long long lines[kStatLineWords], c[4];
        RT_HIP(r, hipMemcpy(lines, r->q.counters.p, sizeof(lines), hipMemcpyDeviceToHost));
        sum_stat_lines(lines, c);
        stats->shadow_rays = c[1];
    }
    return st;
}

// The one-bounce diffuse layer of the current camera:
// rt_render_ao's rays to their nearest hits, each hit shaded as a frame shades it
// (fill_shading: the frames' own L, ambient and shadow switch), and like it no
// fill_frame_args and nothing of the frames' framebuffer.
int rt_render_indirect(rt_renderer* r, const rt_indirect_params* p, const rt_indirect_out* out, void* stream,
                       rt_stats* stats) {
    if (!r) return fail(r, RT_E_INVALID, "rt_render_indirect: null handle");
    if (!p) return fail(r, RT_E_INVALID, "rt_render_indirect: null parameters");
    if (!out || (!out->dev_layer && !out->dev_occluded))
        return fail(r, RT_E_INVALID, "rt_render_indirect: no output buffer");
    if (!ao_rays_ok(p->rays))
        return fail(r, RT_E_INVALID, "rt_render_indirect: rays must be 1, 2, 4, 8, 16, 32 or 64");
    if (!ao_radius_ok(p->radius)) return fail(r, RT_E_INVALID, "rt_render_indirect: radius must be > 0");
    if (!indirect_scale_ok(p->sky_scale))
        return fail(r, RT_E_INVALID, "rt_render_indirect: sky_scale must be finite and >= 0");
    if (p->flags) return fail(r, RT_E_INVALID, "rt_render_indirect: unknown flag bits");
    if (!r->has_scene) return fail(r, RT_E_NOSCENE, "rt_render_indirect: no scene (rt_set_scene first)");
    hipStream_t hs;
    FrameArgs a;
    int st;
    if ((st = query_begin(r, stream, hs, a))) return st;
    fill_camera(r, a.cam);
    a.W = r->W;
    a.H = r->H;
    fill_shading(r, a);
    // the frames' own albedo table, made ahead of the stats bracket like the G-buffer's
    if ((st = ensure_prim_al(r, a.sc, hs))) return st;
    const uint32_t key = ao_key(mix32(r->cfg.seed ^ 0x9E3779B9u), p->salt);
    st = query_launch(r, "rt_render_indirect", hs, stats, [&](unsigned long long* ctr) {
        return launch_indirect(a, out->dev_layer, out->dev_occluded, p->rays, p->radius, key, p->sky_scale, ctr, hs);
    });
    if (!st && stats) {
        stats->primary_rays = static_cast<uint64_t>(r->W) * r->H;
        // the bounce rays and the shadow rays at their hits are the kernel's count, word 1 of the
        // stat lines query_launch just read (rt_render_ao's way)
        unsigned long long lines[kStatLineWords], c[4];
        RT_HIP(r, hipMemcpy(lines, r->q.counters.p, sizeof(lines), hipMemcpyDeviceToHost));
        sum_stat_lines(lines, c);
        stats->shadow_rays = c[1];
    }
    return st;
}

void rt_filter_params_default(rt_filter_params* p) {
    if (!p) return;
    p->passes = 3;
    p->channels = 1;
    p->depth_sigma = 0.05f;
    p->normal_power = 5;
    p->flags = 0;
}

// The guide-driven filter of a per-pixel layer.  It reads the
// handle's size and nothing else of it: no scene, no camera, no frame.  The
// stats bracket is the queries' (its stat lines stay zero: no kernel here counts).
int rt_filter_layer(rt_renderer* r, const rt_filter_params* p, const rt_gbuffer* guides, const void* dev_in,
                    void* dev_out, void* stream, rt_stats* stats) {
    if (!r) return fail(r, RT_E_INVALID, "rt_filter_layer: null handle");
    if (!p) return fail(r, RT_E_INVALID, "rt_filter_layer: null parameters");
    if (!guides || !guides->dev_hits || !guides->dev_normals)
        return fail(r, RT_E_INVALID, "rt_filter_layer: the hits and the normals of a G-buffer are required");
    if (!dev_in || !dev_out) return fail(r, RT_E_INVALID, "rt_filter_layer: null layer");
    if (dev_in == dev_out) return fail(r, RT_E_INVALID, "rt_filter_layer: the input and the output must be distinct");
    if (!filter_passes_ok(p->passes)) return fail(r, RT_E_INVALID, "rt_filter_layer: passes must be 1..5");
    if (!filter_channels_ok(p->channels)) return fail(r, RT_E_INVALID, "rt_filter_layer: channels must be 1 or 4");
    if (!filter_depth_sigma_ok(p->depth_sigma)) return fail(r, RT_E_INVALID, "rt_filter_layer: depth_sigma must be > 0");
    if (!filter_normal_power_ok(p->normal_power)) return fail(r, RT_E_INVALID, "rt_filter_layer: normal_power must be 0..7");
    if (p->flags) return fail(r, RT_E_INVALID, "rt_filter_layer: unknown flag bits");
    hipStream_t hs;
    int st;
    if ((st = stream_begin(r, stream, hs))) return st;
    const size_t n = static_cast<size_t>(r->W) * r->H;
    if ((st = ensure(r, r->flt.rec, n))) return st;
    if (filter_needs_scratch(p->passes) && (st = ensure(r, r->flt.pong, n * p->channels))) return st;
    return query_launch(r, "rt_filter_layer", hs, stats, [&](unsigned long long*) {
        return launch_filter(r->W, r->H, guides->dev_hits, guides->dev_normals, r->flt.rec.p, dev_in, dev_out,
                             filter_needs_scratch(p->passes) ? r->flt.pong.p : nullptr, p->passes, p->channels,
                             p->depth_sigma, p->normal_power, hs);
    });
}

// The multiply of a layer into a frame's pixels, in place: the caller's buffer
// (a mapped display buffer included: this call maps nothing) or the internal
// framebuffer.  Nothing of the progressive sums: the next frame overwrites it.
int rt_apply_layer(rt_renderer* r, void* dev_rgba8, const void* dev_layer, float floor, void* stream) {
    if (!r) return fail(r, RT_E_INVALID, "rt_apply_layer: null handle");
    if (!dev_layer) return fail(r, RT_E_INVALID, "rt_apply_layer: null layer");
    if (!apply_floor_ok(floor)) return fail(r, RT_E_INVALID, "rt_apply_layer: floor must be in [0, 1]");
    uint32_t* px = dev_rgba8 ? static_cast<uint32_t*>(dev_rgba8) : r->fb.p;
    // (a resize whose allocation failed leaves no internal framebuffer)
    if (!px) return fail(r, RT_E_STATE, "rt_apply_layer: no framebuffer (a resize failed): resize again");
    hipStream_t hs;
    int st;
    if ((st = stream_begin(r, stream, hs))) return st;
    return query_launch(r, "rt_apply_layer", hs, nullptr, [&](unsigned long long*) {
        return launch_apply_layer(px, static_cast<const float*>(dev_layer), r->W, r->H, floor, hs);
    });
}

// A float4 layer's r, g and b added into a frame's pixels, in place (DESIGN.md
// 5.18): rt_apply_layer's buffers, stream and ordering.
int rt_add_layer(rt_renderer* r, void* dev_rgba8, const void* dev_layer4, const void* dev_albedo, float gain,
                 void* stream) {
    if (!r) return fail(r, RT_E_INVALID, "rt_add_layer: null handle");
    if (!dev_layer4) return fail(r, RT_E_INVALID, "rt_add_layer: null layer");
    if (!indirect_scale_ok(gain)) return fail(r, RT_E_INVALID, "rt_add_layer: gain must be finite and >= 0");
    uint32_t* px = dev_rgba8 ? static_cast<uint32_t*>(dev_rgba8) : r->fb.p;
    if (!px) return fail(r, RT_E_STATE, "rt_add_layer: no framebuffer (a resize failed): resize again");
    hipStream_t hs;
    int st;
    if ((st = stream_begin(r, stream, hs))) return st;
    return query_launch(r, "rt_add_layer", hs, nullptr, [&](unsigned long long*) {
        return launch_add_layer(px, dev_layer4, static_cast<const uint32_t*>(dev_albedo), r->W, r->H, gain, hs);
    });
}

void rt_reproject_params_default(rt_reproject_params* p) {
    if (!p) return;
    p->channels = 1;
    p->max_count = 32.0f;
    p->depth_tol = 0.05f;
    p->flags = 0;
}

// A layer carried across camera motion: the handle's size and
// current camera, and the caller's buffers of this frame and the previous one.
// No scene, no frame; the handle keeps nothing between two calls.
int rt_reproject_layer(rt_renderer* r, const rt_reproject_params* p, const void* dev_hits, const rt_history* hist,
                       const void* dev_cur, void* dev_out, void* dev_count_out, void* stream, rt_stats* stats) {
    if (!r) return fail(r, RT_E_INVALID, "rt_reproject_layer: null handle");
    if (!p) return fail(r, RT_E_INVALID, "rt_reproject_layer: null parameters");
    if (!dev_hits) return fail(r, RT_E_INVALID, "rt_reproject_layer: the current G-buffer's hits are required");
    if (!dev_cur || !dev_out || !dev_count_out) return fail(r, RT_E_INVALID, "rt_reproject_layer: null layer or count");
    if (hist && (!hist->dev_hits || !hist->dev_layer || !hist->dev_count))
        return fail(r, RT_E_INVALID, "rt_reproject_layer: a history needs its hits, its layer and its count");
    if (dev_out == dev_cur || (hist && dev_out == hist->dev_layer))
        return fail(r, RT_E_INVALID, "rt_reproject_layer: the output must be distinct from the layers it reads");
    if (hist && dev_count_out == hist->dev_count)
        return fail(r, RT_E_INVALID, "rt_reproject_layer: the count output must be distinct from the history's count");
    if (!reproject_channels_ok(p->channels)) return fail(r, RT_E_INVALID, "rt_reproject_layer: channels must be 1 or 4");
    if (!reproject_max_count_ok(p->max_count))
        return fail(r, RT_E_INVALID, "rt_reproject_layer: max_count must be finite and >= 1");
    if (!reproject_depth_tol_ok(p->depth_tol)) return fail(r, RT_E_INVALID, "rt_reproject_layer: depth_tol must be > 0");
    if (p->flags) return fail(r, RT_E_INVALID, "rt_reproject_layer: unknown flag bits");
    hipStream_t hs;
    int st;
    if ((st = stream_begin(r, stream, hs))) return st;
    CamArgs cam;
    fill_camera(r, cam);
    PrevCamera prev{};
    if (hist) prev = prev_camera(hist->pose, hist->K);
    return query_launch(r, "rt_reproject_layer", hs, stats, [&](unsigned long long*) {
        return launch_reproject(cam, r->W, r->H, dev_hits, dev_cur, dev_out, dev_count_out,
                                hist ? hist->dev_hits : nullptr, hist ? hist->dev_layer : nullptr,
                                hist ? hist->dev_count : nullptr, prev, p->channels, p->max_count, p->depth_tol, hs);
    });
}

}  // extern "C"
