// rt_reproject.hip — a per-pixel layer carried across camera motion
// (rt_reproject_layer; include/rt.h).  The reference has no
// counterpart: its render kernel writes one colour per pixel and keeps nothing
// between frames (src/renderer.cu:57-82).
//
// One pixel per lane.  The lane rebuilds its pixel-centre ray (get_ray, the
// G-buffer kernel's), takes its hit point to the previous camera
// (rt_reproject_math.h) and gathers the four pixels around it from the previous
// frame's {hits, layer, count}; a tap counts iff it shows the same sphere at the
// point's distance.  The accepted taps' bilinear mean is blended with this
// frame's value at 1 / count.  The pass is a gather of 4 taps x 3 loads from
// addresses clamped into the image, whether the tap counts or not.  Two thriftier
// forms were measured against this one in alternating runs and gave the same
// bits at the same time, so they are gone
// (one 16-byte load for a row's two rt_hit records; a tap's layer and count
// loaded only once its hit is accepted: profiles/r31/reproject_ab.log).  Compiled
// like rt_gbuffer.hip (-ffp-contract=off, IEEE division and square root): the
// arithmetic is tests/reproject_ref.py's.
#include <hip/hip_runtime.h>

#include "rt_layer.h"
#include "rt_params.h"
#include "rt_reproject_math.h"
#include "rt_shade.h"  // get_ray: Camera::getRay as the G-buffer kernel casts it

namespace rtamd {

namespace {

// A 256-thread block is a 16x16 pixel tile, each of its 4 waves 16x4 of it: under a
// small camera motion a wave's taps fall in 5 or 6 row segments of the history.
constexpr uint32_t kReprojectTile = 16;
constexpr uint32_t kReprojectThreads = kReprojectTile * kReprojectTile;

struct ReprojectArgs {
    uint32_t W, H;
    const uint2* hits;       // the current camera's
    const float* cur;        // this frame's layer, read only
    float* out;
    float* count_out;
    const uint2* h_hits;     // the previous frame's, or null: no history
    const float* h_layer;
    const float* h_count;
    PrevCamera prev;
    float max_count, depth_tol;
};

template <uint32_t kC>
__global__ void __launch_bounds__(kReprojectThreads) reproject_kernel(CamArgs cam, ReprojectArgs g) {
    const uint32_t x = blockIdx.x * kReprojectTile + (threadIdx.x & (kReprojectTile - 1u));
    const uint32_t y = blockIdx.y * kReprojectTile + threadIdx.x / kReprojectTile;
    if (x >= g.W || y >= g.H) return;
    const size_t pix = static_cast<size_t>(y) * g.W + x;
    const uint2 h = g.hits[pix];
    LayerPixel<kC> o;
    o.load(g.cur, pix);
    float n = 1.0f;
    if (h.y != kNoHit && g.h_hits) {
        float d[3];
        get_ray(cam, static_cast<float>(x), static_cast<float>(y), d[0], d[1], d[2]);
        const Reprojection rp = reproject_point(g.prev, cam.o, d, __uint_as_float(h.x));
        if (rp.front) {
            // the corner as integers, clamped from the float (a NaN becomes -1) so that every
            // address formed below lies in the image; whether a tap counts was decided in float
            const int iu = static_cast<int>(fminf(fmaxf(rp.u0, -1.0f), static_cast<float>(g.W)));
            const int iv = static_cast<int>(fminf(fmaxf(rp.v0, -1.0f), static_cast<float>(g.H)));
            const bool in_u[2] = {tap_inside(rp.u0, g.W), tap_inside(rp.u0 + 1.0f, g.W)};
            const bool in_v[2] = {tap_inside(rp.v0, g.H), tap_inside(rp.v0 + 1.0f, g.H)};
            const int last_x = static_cast<int>(g.W) - 1, last_y = static_cast<int>(g.H) - 1;
            size_t q[4];  // tap k = 2 * j + i
            uint2 hh[4];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const size_t row = static_cast<size_t>(min(max(iv + j, 0), last_y)) * g.W;
                q[2 * j] = row + static_cast<size_t>(min(max(iu, 0), last_x));
                q[2 * j + 1] = row + static_cast<size_t>(min(max(iu + 1, 0), last_x));
                hh[2 * j] = g.h_hits[q[2 * j]];
                hh[2 * j + 1] = g.h_hits[q[2 * j + 1]];
            }
            bool ok[4];
            LayerPixel<kC> hv[4];
            float hc[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                ok[k] = in_v[k >> 1] && in_u[k & 1] &&
                        tap_accepted(h.y, hh[k].y, rp.dist, __uint_as_float(hh[k].x), g.depth_tol);
                hv[k].load(g.h_layer, q[k]);
                hc[k] = g.h_count[q[k]];
            }
            float sw = 0.0f, sc = 0.0f;
            LayerPixel<kC> sv;
            for (uint32_t c = 0; c < kC; ++c) sv.v[c] = 0.0f;
#pragma unroll
            for (int k = 0; k < 4; ++k) {  // j outer, i inner
                if (!ok[k]) continue;
                const float w = tap_weight(k & 1, k >> 1, rp.a, rp.b);
                sw += w;
                for (uint32_t c = 0; c < kC; ++c) sv.v[c] += w * hv[k].v[c];
                sc += w * hc[k];
            }
            if (sw > 0.0f) {
                n = reproject_count(sc / sw, g.max_count);
                const float alpha = 1.0f / n;
                for (uint32_t c = 0; c < kC; ++c) o.v[c] = reproject_blend(sv.v[c] / sw, o.v[c], alpha);
            }
        }
    }
    o.store(g.out, pix);
    g.count_out[pix] = n;
}

}  // namespace

// cam: the handle's current camera; hits, cur, out, count_out: W*H records of the
// current frame; h_hits, h_layer, h_count under `prev`: the previous frame's, or
// h_hits null for no history.  The caller checked the parameters field by field
// (reproject_channels_ok, reproject_max_count_ok, reproject_depth_tol_ok, the
// flags) and the pointers.
hipError_t launch_reproject(const CamArgs& cam, uint32_t W, uint32_t H, const void* hits, const void* cur, void* out,
                            void* count_out, const void* h_hits, const void* h_layer, const void* h_count,
                            const PrevCamera& prev, uint32_t channels, float max_count, float depth_tol, hipStream_t st) {
    if (W == 0 || H == 0) return hipSuccess;
    ReprojectArgs g;
    g.W = W, g.H = H;
    g.hits = static_cast<const uint2*>(hits);
    g.cur = static_cast<const float*>(cur);
    g.out = static_cast<float*>(out);
    g.count_out = static_cast<float*>(count_out);
    g.h_hits = static_cast<const uint2*>(h_hits);
    g.h_layer = static_cast<const float*>(h_layer);
    g.h_count = static_cast<const float*>(h_count);
    g.prev = prev;
    g.max_count = max_count, g.depth_tol = depth_tol;
    const dim3 grid((W + kReprojectTile - 1u) / kReprojectTile, (H + kReprojectTile - 1u) / kReprojectTile);
    const dim3 block(kReprojectThreads);
    if (channels == 4u) hipLaunchKernelGGL(reproject_kernel<4>, grid, block, 0, st, cam, g);
    else hipLaunchKernelGGL(reproject_kernel<1>, grid, block, 0, st, cam, g);
    return hipGetLastError();
}

}  // namespace rtamd
