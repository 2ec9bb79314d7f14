// rt_cli — headless native driver over the C++ host surface (rt_renderer.hpp).
//
// Plays the reference's main.cpp / Window / Displayer loop without a window
// (main.cpp:4-13, src/window/window.cpp:98-108): builds a renderer, sets the
// Displayer's pose each frame, renders, and optionally writes a PPM.  Used by
// tests/test_native_cli.py and for rocprof runs without Python.
//
//   rt_cli [--config c1|c2|c3|c4|c5] [--width W --height H --spp S --spheres N
//           --depth D] [--frames F] [--out image.ppm] [--scene in.rtsph]
//          [--save-scene out.rtsph] [--host-build] [--gpus N [--same-device]]
//          [--progressive] [--panel] [--walk] [--test-poison] [--gbuffer hits.bin]
//          [--ao ao.pgm [--ao-rays R] [--ao-radius X] [--ao-filter PASSES]]
//          [--indirect image.ppm [--indirect-rays R] [--indirect-radius X]]
//
// --panel prints the stats panel (rt_camera.hpp StatsPanel: the reference's
// ImGui window numbers plus Mrays/s, spp, GPUs) after every frame; --walk
// moves the camera through the Displayer's controller (W held every frame);
// --progressive accumulates samples while the camera stays put.  --gbuffer
// renders the first-hit G-buffer of the last frame's camera (rt_render_gbuffer)
// and writes its hits as W*H raw little-endian rt_hit records {f32 t, u32 sphere}.
// --ao renders that camera's ambient-occlusion layer (rt_render_ao; R rays a
// pixel, default 16, of length X, default 0.1) and writes it as a binary PGM,
// 255 = open.  --ao-filter PASSES (1..5) filters the layer under the G-buffer's
// guides first (rt_filter_layer at its default tolerances) and writes the
// filtered layer instead, (uint8)(value * 255).
// --indirect renders that camera's one-bounce diffuse layer (rt_render_indirect;
// R rays a pixel, default 4, of length X, default 0.25, sky_scale 1), adds it into
// the last frame under the G-buffer's albedo (rt_add_layer, gain 1) and writes
// the result as a PPM.
//
// --gpus N: one process drives N devices through the C-ABI's
// multi-device handle (rt_create_multi): device k renders the 64x64 tiles
// t = k, k+N, ... into a packed slab, the slabs go to device 0 over RCCL and
// are unpacked there into the frame, two frames in flight.  --same-device puts
// all N renderers on device 0 (a rehearsal of the plan on one GPU; peer-copy
// transport, since RCCL refuses a device twice).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <hip/hip_runtime_api.h>

#include <chrono>
#include <string>
#include <vector>


#include "../../include/rt_camera.hpp"
#include "../../include/rt_renderer.hpp"

int write_ppm(const std::string& out, const std::vector<uint8_t>& img, int W, int H) {
    FILE* f = fopen(out.c_str(), "wb");
    if (!f) {
        fprintf(stderr, "cannot write %s\n", out.c_str());
        return 1;
    }
    fprintf(f, "P6\n%d %d\n255\n", W, H);
    for (size_t i = 0; i < (size_t)W * H; ++i) fwrite(&img[4 * i], 1, 3, f);
    fclose(f);
    return 0;
}

// One process, N devices: the C-ABI's multi-device handle
// (rt_create_multi) renders every frame across the devices: tiles
// round-robin, each device's slab to device 0 over RCCL (grouped ncclSend /
// ncclRecv on per-device comm streams; peer copies for a --same-device
// rehearsal), one unpack, two frames in flight.
int run_multi(const rt_config& rc, const float pose[16], int gpus, bool same_device, int frames,
              const std::string& out, int W, int H, int spp, int depth, long n,
              const std::string& scene_in) {
    const int ndev = rt_device_count();
    if (ndev < 1) throw rtamd::Error(RT_E_HIP, "no HIP device");
    if (!same_device && ndev < gpus) throw rtamd::Error(RT_E_INVALID, "fewer devices than --gpus");
    std::vector<float> sp;
    std::vector<uint32_t> al;
    if (!scene_in.empty()) {
        rtamd::KernelRenderer::loadSpheres(scene_in, sp, al);
    } else {
        sp.resize(4 * (size_t)n);
        al.resize((size_t)n);
        rtamd::check(rt_generate_spheres((uint32_t)n, 0x2545F491u, sp.data(), al.data()));
    }
    rt_octree_params p;
    rt_octree_params_default(&p);
    p.max_depth = (uint32_t)depth;
    std::vector<int> devs(gpus);
    for (int k = 0; k < gpus; ++k) devs[k] = same_device ? 0 : k;
    rtamd::KernelRenderer r(rc, devs);
    r.resize(W, H);
    r.setPosition(pose);
    r.setScene(sp, al, &p);
    const rt_multi_info mi = r.multiInfo();
    rt_stats st{};
    r.render(nullptr, nullptr, &st);  // counted frame (devices one after another)
    const uint64_t rays = st.primary_rays + st.shadow_rays;
    r.synchronize();
    // timed: frames back to back, two in flight, one wait at the end
    const int timed = frames > 0 ? frames : 1;
    auto t0 = std::chrono::steady_clock::now();
    for (int f = 0; f < timed; ++f) {
        r.setPosition(pose);  // the Displayer sets the pose every frame
        r.render();
    }
    r.synchronize();
    const double ms =
        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() / timed;
    printf("%d devices (%s, transport %s): %dx%d spp %d: %.3f ms/frame over %d frames "
           "(tiles + %s gather + unpack, 2 in flight), %llu rays, %.1f Mrays/s\n",
           gpus, same_device ? "all on device 0" : "devices 0..N-1",
           mi.transport == RT_TRANSPORT_RCCL ? "rccl" : "peer", W, H, spp, ms, timed,
           mi.transport == RT_TRANSPORT_RCCL ? "RCCL" : "peer-copy", (unsigned long long)rays,
           rays / (ms * 1e3));
    if (!out.empty()) {
        std::vector<uint8_t> img((size_t)W * H * 4);
        r.readback(img.data());
        return write_ppm(out, img, W, H);
    }
    return 0;
}

int main(int argc, char** argv) {
    std::string cfg = "c2", out, scene_in, scene_out, gbuffer_out, ao_out;
    int ao_rays = 16, ao_filter = 0;
    float ao_radius = 0.1f;
    std::string indirect_out;
    int indirect_rays = 4;
    float indirect_radius = 0.25f;
    bool host_build = false, same_device = false, progressive = false, panel = false,
         walk = false, poison = false;
    int gpus = 1;
    bool multi = false;  // --gpus given (even 1: a 1-device RCCL communicator)
    int W = 0, H = 0, spp = 0, frames = 3;
    long n = -1;
    int depth = 0;
    for (int i = 1; i < argc; ++i) {
        auto next = [&](const char* what) -> const char* {
            if (i + 1 >= argc) {
                fprintf(stderr, "missing value for %s\n", what);
                exit(2);
            }
            return argv[++i];
        };
        if (!strcmp(argv[i], "--config")) cfg = next("--config");
        else if (!strcmp(argv[i], "--width")) W = atoi(next("--width"));
        else if (!strcmp(argv[i], "--height")) H = atoi(next("--height"));
        else if (!strcmp(argv[i], "--spp")) spp = atoi(next("--spp"));
        else if (!strcmp(argv[i], "--spheres")) n = atol(next("--spheres"));
        else if (!strcmp(argv[i], "--depth")) depth = atoi(next("--depth"));
        else if (!strcmp(argv[i], "--frames")) frames = atoi(next("--frames"));
        else if (!strcmp(argv[i], "--out")) out = next("--out");
        else if (!strcmp(argv[i], "--scene")) scene_in = next("--scene");
        else if (!strcmp(argv[i], "--save-scene")) scene_out = next("--save-scene");
        else if (!strcmp(argv[i], "--gbuffer")) gbuffer_out = next("--gbuffer");
        else if (!strcmp(argv[i], "--ao")) ao_out = next("--ao");
        else if (!strcmp(argv[i], "--ao-rays")) ao_rays = atoi(next("--ao-rays"));
        else if (!strcmp(argv[i], "--ao-radius")) ao_radius = (float)atof(next("--ao-radius"));
        else if (!strcmp(argv[i], "--ao-filter")) ao_filter = atoi(next("--ao-filter"));
        else if (!strcmp(argv[i], "--indirect")) indirect_out = next("--indirect");
        else if (!strcmp(argv[i], "--indirect-rays")) indirect_rays = atoi(next("--indirect-rays"));
        else if (!strcmp(argv[i], "--indirect-radius")) indirect_radius = (float)atof(next("--indirect-radius"));
        else if (!strcmp(argv[i], "--host-build")) host_build = true;
        else if (!strcmp(argv[i], "--gpus")) gpus = atoi(next("--gpus")), multi = true;
        else if (!strcmp(argv[i], "--same-device")) same_device = true;
        else if (!strcmp(argv[i], "--progressive")) progressive = true;
        else if (!strcmp(argv[i], "--panel")) panel = true;
        else if (!strcmp(argv[i], "--walk")) walk = true;
        else if (!strcmp(argv[i], "--test-poison")) poison = true;  // RT_FLAG_TEST_POISON (tests)
        else {
            fprintf(stderr, "unknown argument %s\n", argv[i]);
            return 2;
        }
    }
    struct C { const char* name; int w, h, spp; long n; int depth; uint32_t mode; };
    const C table[] = {{"c1", 256, 256, 1, 0, 7, RT_MODE_COMPAT},
                       {"c2", 1920, 1080, 1, 1000, 7, RT_MODE_SCENE},
                       {"c3", 1920, 1080, 64, 100000, 7, RT_MODE_SCENE},
                       {"c4", 3840, 2160, 64, 100000, 7, RT_MODE_SCENE},
                       {"c5", 1920, 1080, 256, 1000000, 12, RT_MODE_SCENE}};
    const C* c = nullptr;
    for (const C& e : table)
        if (cfg == e.name) c = &e;
    if (!c) {
        fprintf(stderr, "unknown config %s\n", cfg.c_str());
        return 2;
    }
    W = W ? W : c->w;
    H = H ? H : c->h;
    spp = spp ? spp : c->spp;
    n = n >= 0 ? n : c->n;
    depth = depth ? depth : c->depth;
    try {
        rt_config rc;
        rt_config_default(&rc);
        rc.width = W;
        rc.height = H;
        rc.spp = spp;
        rc.mode = c->mode;
        if (host_build) rc.flags |= RT_FLAG_HOST_BUILD;
        if (progressive) rc.flags |= RT_FLAG_PROGRESSIVE;
        if (poison) rc.flags |= RT_FLAG_TEST_POISON;
        rtamd::KernelRenderer r(rc);
        r.resize(W, H);
        // Displayer default orientation (include/window/displayer.h:47-52):
        // rot = diag(1,-1,-1); compat at (0,0,3), scene at (0.64,0.64,2.2)
        const bool scene = c->mode == RT_MODE_SCENE;
        const float pose[16] = {1, 0, 0, 0, 0, -1, 0, 0, 0, 0, -1, 0,
                                scene ? 0.64f : 0.f, scene ? 0.64f : 0.f, scene ? 2.2f : 3.f, 1};
        if (scene) {
            std::vector<float> sp;
            std::vector<uint32_t> al;
            if (!scene_in.empty()) {
                rtamd::KernelRenderer::loadSpheres(scene_in, sp, al);
            } else {
                sp.resize(4 * (size_t)n);
                al.resize((size_t)n);
                rtamd::check(rt_generate_spheres((uint32_t)n, 0x2545F491u, sp.data(), al.data()));
            }
            if (!scene_out.empty()) rtamd::KernelRenderer::saveSpheres(scene_out, sp, al);
            rt_octree_params p;
            rt_octree_params_default(&p);
            p.max_depth = (uint32_t)depth;
            r.setScene(sp, al, &p);
            const rt_scene_info si = r.sceneInfo();
            printf("scene: %u spheres, %u nodes, %u leaves, %u refs, depth %u/%u, %s build %.2f ms\n",
                   si.n_spheres, si.n_nodes, si.n_leaves, si.n_prim_refs, si.depth_reached,
                   si.max_depth, si.builder == RT_BUILDER_HOST ? "host" : "device", si.build_ms);
        }
        if (multi) {
            if (gpus < 1 || gpus > RT_MAX_DEVICES) throw rtamd::Error(RT_E_INVALID, "--gpus must be 1..16");
            if (!scene) throw rtamd::Error(RT_E_INVALID, "--gpus needs a scene config");
            if (!gbuffer_out.empty()) throw rtamd::Error(RT_E_INVALID, "--gbuffer is single-device here");
            if (!ao_out.empty()) throw rtamd::Error(RT_E_INVALID, "--ao is single-device here");
            if (!indirect_out.empty()) throw rtamd::Error(RT_E_INVALID, "--indirect is single-device here");
            return run_multi(rc, pose, gpus, same_device, frames, out, W, H, spp, depth, n,
                             scene_in);
        }
        rt_stats st{};
        double best = 1e30;
        // the Displayer's controller, starting at this config's camera position
        rtamd::CameraController cam;
        for (int i = 0; i < 3; ++i) cam.pos[i] = pose[12 + i];
        rtamd::StatsPanel stats_panel;
        for (int f = 0; f < frames; ++f) {
            auto t0 = std::chrono::steady_clock::now();
            if (walk) {
                rtamd::Keys k;
                k.w = true;
                cam.processInput(k, r);  // like Displayer::processInput, every frame
            } else {
                r.setPosition(pose);
            }
            r.render(nullptr, nullptr, &st);
            auto t1 = std::chrono::steady_clock::now();
            const double ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
            best = std::min(best, ms);
            if (panel) {
                stats_panel.update(ms, st, 1);
                printf("-- frame %d --\n%s", f, stats_panel.text().c_str());
            }
        }
        const double rays = (double)st.primary_rays + (double)st.shadow_rays;
        printf("%s %dx%d spp %d: kernel %.3f ms, wall %.3f ms, %.0f rays (%llu primary + %llu shadow), "
               "%.1f Mrays/s\n",
               c->name, W, H, spp, st.ms, best, rays, (unsigned long long)st.primary_rays,
               (unsigned long long)st.shadow_rays, rays / (st.ms * 1e3));
        if (!out.empty()) {
            std::vector<uint8_t> img((size_t)W * H * 4);
            r.readback(img.data());
            FILE* f = fopen(out.c_str(), "wb");
            if (!f) {
                fprintf(stderr, "cannot write %s\n", out.c_str());
                return 1;
            }
            fprintf(f, "P6\n%d %d\n255\n", W, H);
            for (size_t i = 0; i < (size_t)W * H; ++i) fwrite(&img[4 * i], 1, 3, f);
            fclose(f);
        }
        if (!gbuffer_out.empty()) {
            // after the last frame: the id / depth buffer of the camera it used
            const size_t npix = (size_t)W * H;
            void* d_hits = nullptr;
            if (hipMalloc(&d_hits, npix * sizeof(rt_hit)) != hipSuccess)
                throw rtamd::Error(RT_E_HIP, "hipMalloc of the hits buffer");
            std::vector<rt_hit> hits(npix);
            try {
                r.renderGBuffer(d_hits);
                r.synchronize();
            } catch (...) {
                (void)hipFree(d_hits);
                throw;
            }
            const hipError_t e = hipMemcpy(hits.data(), d_hits, npix * sizeof(rt_hit), hipMemcpyDeviceToHost);
            (void)hipFree(d_hits);
            if (e != hipSuccess) throw rtamd::Error(RT_E_HIP, "hipMemcpy of the hits buffer");
            size_t n_hit = 0;
            for (const rt_hit& h : hits) n_hit += h.sphere != RT_NO_HIT;
            FILE* f = fopen(gbuffer_out.c_str(), "wb");
            if (!f || fwrite(hits.data(), sizeof(rt_hit), npix, f) != npix) {
                fprintf(stderr, "cannot write %s\n", gbuffer_out.c_str());
                if (f) fclose(f);
                return 1;
            }
            fclose(f);
            printf("gbuffer: %zu of %zu pixels hit a sphere\n", n_hit, npix);
        }
        if (!ao_out.empty()) {
            // after the last frame: the occlusion layer of the camera it used
            if (!scene) throw rtamd::Error(RT_E_INVALID, "--ao needs a scene config");
            const size_t npix = (size_t)W * H;
            // the counts; with --ao-filter also the float layer, the G-buffer's guides and the filtered layer
            struct DevBufs {
                void* p[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
                ~DevBufs() {
                    for (void* q : p)
                        if (q) (void)hipFree(q);
                }
            } d;
            enum { kOcc, kAo, kHits, kNormals, kFiltered };
            const size_t bytes[5] = {npix * sizeof(uint32_t), npix * sizeof(float), npix * sizeof(rt_hit),
                                     npix * 4 * sizeof(float), npix * sizeof(float)};
            for (int b = 0; b < (ao_filter ? 5 : 1); ++b)
                if (hipMalloc(&d.p[b], bytes[b]) != hipSuccess)
                    throw rtamd::Error(RT_E_HIP, "hipMalloc of the occlusion buffers");
            std::vector<uint32_t> occ(npix);
            std::vector<float> filtered(ao_filter ? npix : 0);
            rt_stats ast{}, fst{};
            if (ao_filter) r.renderGBuffer(d.p[kHits], d.p[kNormals], nullptr);
            r.renderAO((uint32_t)ao_rays, ao_radius, d.p[kAo], d.p[kOcc], 0, nullptr, &ast);
            if (ao_filter) {
                rt_filter_params fp;
                rt_filter_params_default(&fp);
                r.filterLayer(d.p[kAo], d.p[kFiltered], d.p[kHits], d.p[kNormals], (uint32_t)ao_filter, fp.channels,
                              fp.depth_sigma, fp.normal_power, nullptr, &fst);
                if (hipMemcpy(filtered.data(), d.p[kFiltered], bytes[kFiltered], hipMemcpyDeviceToHost) != hipSuccess)
                    throw rtamd::Error(RT_E_HIP, "hipMemcpy of the filtered layer");
            }
            if (hipMemcpy(occ.data(), d.p[kOcc], bytes[kOcc], hipMemcpyDeviceToHost) != hipSuccess)
                throw rtamd::Error(RT_E_HIP, "hipMemcpy of the occlusion buffer");
            std::vector<uint8_t> grey(npix);
            unsigned long long total = 0;
            for (size_t i = 0; i < npix; ++i) {
                total += occ[i];
                if (ao_filter) {
                    const float g = filtered[i] * 255.0f;
                    grey[i] = g >= 255.0f ? 255 : g > 0.0f ? (uint8_t)g : 0;
                } else {
                    grey[i] = (uint8_t)(((uint32_t)ao_rays - occ[i]) * 255u / (uint32_t)ao_rays);
                }
            }
            FILE* f = fopen(ao_out.c_str(), "wb");
            if (!f || fprintf(f, "P5\n%d %d\n255\n", W, H) < 0 || fwrite(grey.data(), 1, npix, f) != npix) {
                fprintf(stderr, "cannot write %s\n", ao_out.c_str());
                if (f) fclose(f);
                return 1;
            }
            fclose(f);
            printf("ao: %llu of %llu rays occluded (%d rays a pixel, radius %g), %.3f ms\n", total,
                   (unsigned long long)ast.shadow_rays, ao_rays, ao_radius, ast.ms);
            if (ao_filter) printf("ao-filter: %d passes, %.3f ms\n", ao_filter, fst.ms);
        }
        if (!indirect_out.empty()) {
            // after the last frame: its image with the camera's one-bounce layer added (no reprojection, no filter)
            if (!scene) throw rtamd::Error(RT_E_INVALID, "--indirect needs a scene config");
            const size_t npix = (size_t)W * H;
            struct DevBufs {
                void* p[3] = {nullptr, nullptr, nullptr};
                ~DevBufs() {
                    for (void* q : p)
                        if (q) (void)hipFree(q);
                }
            } d;
            enum { kLayer, kOcc, kAlbedo };
            const size_t bytes[3] = {npix * 4 * sizeof(float), npix * sizeof(uint32_t), npix * sizeof(uint32_t)};
            for (int b = 0; b < 3; ++b)
                if (hipMalloc(&d.p[b], bytes[b]) != hipSuccess)
                    throw rtamd::Error(RT_E_HIP, "hipMalloc of the indirect buffers");
            rt_stats ist{};
            r.renderGBuffer(nullptr, nullptr, d.p[kAlbedo]);
            r.renderIndirect((uint32_t)indirect_rays, indirect_radius, d.p[kLayer], d.p[kOcc], 0, 1.0f, nullptr, &ist);
            r.addLayer(d.p[kLayer], 1.0f, d.p[kAlbedo]);
            std::vector<uint8_t> img(npix * 4);
            r.readback(img.data());
            std::vector<uint32_t> occ(npix);
            if (hipMemcpy(occ.data(), d.p[kOcc], bytes[kOcc], hipMemcpyDeviceToHost) != hipSuccess)
                throw rtamd::Error(RT_E_HIP, "hipMemcpy of the hit counts");
            unsigned long long total = 0;
            for (size_t i = 0; i < npix; ++i) total += occ[i];
            if (write_ppm(indirect_out, img, W, H)) return 1;
            printf("indirect: %llu bounce rays hit, %llu bounce and shadow rays cast (%d rays a pixel, radius %g), %.3f ms\n",
                   total, (unsigned long long)ist.shadow_rays, indirect_rays, indirect_radius, ist.ms);
        }
    } catch (const rtamd::Error& e) {
        fprintf(stderr, "rt_cli: %s (code %d)\n", e.what(), e.code);
        return 1;
    }
    return 0;
}
