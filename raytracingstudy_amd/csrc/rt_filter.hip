// rt_filter.hip — the guide-driven filter of a per-pixel layer (rt_filter_layer)
// and the multiply of a layer into an RGBA8 frame (rt_apply_layer); include/rt.h,
// DESIGN.md 5.16; and a float4 layer added into one (rt_add_layer, 5.18).  The reference has no counterpart: its render kernel writes one
// colour per pixel (src/renderer.cu:57-82).
//
// The filter is an edge-avoiding a-trous wavelet filter: per pass 25 taps of a
// B3-spline kernel at spacing 2^s, each weighted by how well the tap's normal and
// depth agree with the pixel's (rt_filter_math.h).  The memory path charges by
// load instruction, so a first kernel packs the two guide buffers into one
// 16-byte record a pixel, {n.x, n.y, n.z, t} with t = +inf marking a miss: a tap
// then costs one dwordx4 of guides and one load of the layer.  One pixel per lane.
// At tap spacing 1, 2 and 4 a block stages its 16x16 tile plus the halo in LDS
// once and the 25 taps read that image (a 3-pass call 0.239 -> 0.129 ms on C3's
// frame against 25 global loads a pixel, profiles/r30/filter_lds_ab4.log); at
// spacing 8 and 16 the halo is 9 and 25 times the tile, and the taps stay 25
// guarded global loads.  Compiled like rt_gbuffer.hip (-ffp-contract=off, IEEE
// division): the arithmetic is tests/filter_ref.py's.
#include <hip/hip_runtime.h>

#include "rt_filter_math.h"
#include "rt_indirect_math.h"  // add_layer_pixel
#include "rt_layer.h"  // LayerPixel: a layer's pixel as one dword or one dwordx4
#include "rt_params.h"

namespace rtamd {

namespace {

// A 256-thread block is a 16x16 pixel tile, each of its 4 waves 16x4 of it (a
// wave's loads of one tap are 4 row segments of 256 B of records).
constexpr uint32_t kFilterTile = 16;
constexpr uint32_t kFilterThreads = kFilterTile * kFilterTile;
constexpr int kFilterLdsMaxStep = 4;    // the largest tap spacing whose tile and halo are staged in LDS
constexpr uint32_t kFlatThreads = 256;  // the pack and apply kernels: one pixel per lane, row-major

// {n.x, n.y, n.z, t} per pixel from rt_render_gbuffer's hits and normals; a miss
// (sphere == RT_NO_HIT) gets t = +inf, which no hit carries (a hit's t is below
// the primary ray's tmax = +inf), so nothing the filter reads is lost.
__global__ void __launch_bounds__(kFlatThreads) filter_pack_kernel(const uint2* hits, const float4* normals,
                                                                   float4* rec, size_t n) {
    const size_t i = static_cast<size_t>(blockIdx.x) * kFlatThreads + threadIdx.x;
    if (i >= n) return;
    const uint2 h = hits[i];
    float4 g = normals[i];
    g.w = h.y == kNoHit ? __builtin_inff() : __uint_as_float(h.x);
    rec[i] = g;
}

// One pass at tap spacing `step` (here 8 and 16; W, H <= 32768: the tap coordinates fit an int)
// from global memory.
template <uint32_t kC>
__global__ void __launch_bounds__(kFilterThreads) filter_pass_kernel(const float4* rec, const float* in, float* out,
                                                                     uint32_t W, uint32_t H, int step,
                                                                     float depth_sigma, uint32_t normal_power) {
    const uint32_t x = blockIdx.x * kFilterTile + (threadIdx.x & (kFilterTile - 1u));
    const uint32_t y = blockIdx.y * kFilterTile + threadIdx.x / kFilterTile;
    if (x >= W || y >= H) return;
    const size_t pix = static_cast<size_t>(y) * W + x;
    const float4 gp = rec[pix];
    LayerPixel<kC> vp;
    vp.load(in, pix);
    if (gp.w == __builtin_inff()) {  // a miss copies its value
        vp.store(out, pix);
        return;
    }
    const float n_p[3] = {gp.x, gp.y, gp.z};
    const float iz = filter_inv_depth(depth_sigma, gp.w);
    float sw = 0.0f;
    LayerPixel<kC> sv;
    for (uint32_t c = 0; c < kC; ++c) sv.v[c] = 0.0f;
#pragma unroll
    for (int j = -kFilterReach; j <= kFilterReach; ++j) {
        const int qy = static_cast<int>(y) + j * step;
#pragma unroll
        for (int i = -kFilterReach; i <= kFilterReach; ++i) {
            const int qx = static_cast<int>(x) + i * step;
            if (qx < 0 || qx >= static_cast<int>(W) || qy < 0 || qy >= static_cast<int>(H)) continue;
            const size_t q = static_cast<size_t>(qy) * W + static_cast<size_t>(qx);
            const float4 gq = rec[q];
            if (gq.w == __builtin_inff()) continue;  // a miss tap never contributes
            const float n_q[3] = {gq.x, gq.y, gq.z};
            const float w = filter_weight(filter_tap_k(i) * filter_tap_k(j), n_p, n_q, gp.w, gq.w, iz, normal_power);
            LayerPixel<kC> vq;
            vq.load(in, q);
            sw += w;
            for (uint32_t c = 0; c < kC; ++c) sv.v[c] += w * vq.v[c];
        }
    }
    // (false for a NaN sum: garbage guides copy the value)
    LayerPixel<kC> o;
    for (uint32_t c = 0; c < kC; ++c) o.v[c] = sw > 0.0f ? sv.v[c] / sw : vp.v[c];
    o.store(out, pix);
}

// The same pass at kStep 1, 2 or 4 from an LDS image of the block's tile plus its
// halo of 2 * kStep pixels, staged once (20, 24 or 32 pixels a side: at most
// 32 KB a block with four channels).  A record
// outside the image is staged as a miss (both are skipped), so the taps need no
// bounds test; the sums run in the same order over the same values.
template <uint32_t kC, int kStep>
__global__ void __launch_bounds__(kFilterThreads) filter_pass_lds_kernel(const float4* rec, const float* in, float* out,
                                                                         uint32_t W, uint32_t H, float depth_sigma,
                                                                         uint32_t normal_power) {
    constexpr int kHalo = kFilterReach * kStep, kSide = static_cast<int>(kFilterTile) + 2 * kHalo;
    __shared__ float4 s_rec[kSide * kSide];
    __shared__ LayerPixel<kC> s_val[kSide * kSide];
    const int x0 = static_cast<int>(blockIdx.x * kFilterTile) - kHalo, y0 = static_cast<int>(blockIdx.y * kFilterTile) - kHalo;
    for (int at = static_cast<int>(threadIdx.x); at < kSide * kSide; at += static_cast<int>(kFilterThreads)) {
        const int gx = x0 + at % kSide, gy = y0 + at / kSide;
        float4 g = make_float4(0.0f, 0.0f, 0.0f, __builtin_inff());
        LayerPixel<kC> v;
        for (uint32_t c = 0; c < kC; ++c) v.v[c] = 0.0f;
        if (gx >= 0 && gx < static_cast<int>(W) && gy >= 0 && gy < static_cast<int>(H)) {
            const size_t q = static_cast<size_t>(gy) * W + static_cast<size_t>(gx);
            g = rec[q];
            v.load(in, q);
        }
        s_rec[at] = g;
        s_val[at] = v;
    }
    __syncthreads();
    const int lx = static_cast<int>(threadIdx.x & (kFilterTile - 1u)), ly = static_cast<int>(threadIdx.x / kFilterTile);
    const uint32_t x = blockIdx.x * kFilterTile + lx, y = blockIdx.y * kFilterTile + ly;
    if (x >= W || y >= H) return;
    const size_t pix = static_cast<size_t>(y) * W + x;
    const int centre = (ly + kHalo) * kSide + lx + kHalo;
    const float4 gp = s_rec[centre];
    const LayerPixel<kC> vp = s_val[centre];
    if (gp.w == __builtin_inff()) {
        vp.store(out, pix);
        return;
    }
    const float n_p[3] = {gp.x, gp.y, gp.z};
    const float iz = filter_inv_depth(depth_sigma, gp.w);
    float sw = 0.0f;
    LayerPixel<kC> sv;
    for (uint32_t c = 0; c < kC; ++c) sv.v[c] = 0.0f;
#pragma unroll
    for (int j = -kFilterReach; j <= kFilterReach; ++j) {
#pragma unroll
        for (int i = -kFilterReach; i <= kFilterReach; ++i) {
            const int q = centre + j * kStep * kSide + i * kStep;
            const float4 gq = s_rec[q];
            if (gq.w == __builtin_inff()) continue;
            const float n_q[3] = {gq.x, gq.y, gq.z};
            const float w = filter_weight(filter_tap_k(i) * filter_tap_k(j), n_p, n_q, gp.w, gq.w, iz, normal_power);
            const LayerPixel<kC> vq = s_val[q];
            sw += w;
            for (uint32_t c = 0; c < kC; ++c) sv.v[c] += w * vq.v[c];
        }
    }
    LayerPixel<kC> o;
    for (uint32_t c = 0; c < kC; ++c) o.v[c] = sw > 0.0f ? sv.v[c] / sw : vp.v[c];
    o.store(out, pix);
}

// m = floor + gain * layer with gain = 1.0f - floor; R, G and B scaled by m and
// truncated like the frames' own conversion (rt_shade.h pack_rgba8), A kept.
__device__ __forceinline__ uint32_t scale_channel(uint32_t c, float m) {
    // (a NaN product stores 255, a negative one 0)
    return static_cast<uint32_t>(fmaxf(fminf(static_cast<float>(c) * m, 255.0f), 0.0f));
}
__global__ void __launch_bounds__(kFlatThreads) apply_layer_kernel(uint32_t* rgba8, const float* layer, size_t n,
                                                                   float floor, float gain) {
    const size_t i = static_cast<size_t>(blockIdx.x) * kFlatThreads + threadIdx.x;
    if (i >= n) return;
    const float t = gain * layer[i];
    const float m = floor + t;
    const uint32_t p = rgba8[i];
    rgba8[i] = scale_channel(p & 0xFFu, m) | (scale_channel((p >> 8) & 0xFFu, m) << 8) |
               (scale_channel((p >> 16) & 0xFFu, m) << 16) | (p & 0xFF000000u);
}

// A float4 layer's r, g and b added into the frame's bytes (rt_add_layer;
// rt_indirect_math.h add_layer_pixel), each times gain and, with an albedo buffer,
// the pixel's albedo byte / 255; the layer's w is not read, A is kept.
template <bool kAlbedo>
__global__ void __launch_bounds__(kFlatThreads) add_layer_kernel(uint32_t* rgba8, const float* layer,
                                                                 const uint32_t* albedo, size_t n, float gain) {
    const size_t i = static_cast<size_t>(blockIdx.x) * kFlatThreads + threadIdx.x;
    if (i >= n) return;
    LayerPixel<4> v;
    v.load(layer, i);
    rgba8[i] = add_layer_pixel(rgba8[i], v.v, kAlbedo ? albedo[i] : 0u, kAlbedo, gain);
}

// one pass: from the LDS image up to tap spacing kFilterLdsMaxStep, from global memory beyond
template <uint32_t kC>
void launch_pass(dim3 grid, dim3 block, hipStream_t st, const float4* rec, const float* src, float* dst, uint32_t W,
                 uint32_t H, int step, float depth_sigma, uint32_t normal_power) {
    switch (step <= kFilterLdsMaxStep ? step : 0) {
    case 1:
        hipLaunchKernelGGL((filter_pass_lds_kernel<kC, 1>), grid, block, 0, st, rec, src, dst, W, H, depth_sigma,
                           normal_power);
        break;
    case 2:
        hipLaunchKernelGGL((filter_pass_lds_kernel<kC, 2>), grid, block, 0, st, rec, src, dst, W, H, depth_sigma,
                           normal_power);
        break;
    case 4:
        hipLaunchKernelGGL((filter_pass_lds_kernel<kC, 4>), grid, block, 0, st, rec, src, dst, W, H, depth_sigma,
                           normal_power);
        break;
    default:
        hipLaunchKernelGGL((filter_pass_kernel<kC>), grid, block, 0, st, rec, src, dst, W, H, step, depth_sigma,
                           normal_power);
    }
}

}  // namespace

// hits / normals: rt_render_gbuffer's buffers for W x H; rec: W*H records of the
// handle's; in / out: W*H*channels floats, distinct; pong: as large, or null when
// filter_needs_scratch(passes) is false.  The caller checked the parameters
// (filter_params_ok).
hipError_t launch_filter(uint32_t W, uint32_t H, const void* hits, const void* normals, float4* rec, const void* in,
                         void* out, float* pong, uint32_t passes, uint32_t channels, float depth_sigma,
                         uint32_t normal_power, hipStream_t st) {
    if (W == 0 || H == 0) return hipSuccess;
    const size_t n = static_cast<size_t>(W) * H;
    const uint32_t flat_blocks = static_cast<uint32_t>((n + kFlatThreads - 1u) / kFlatThreads);
    hipLaunchKernelGGL(filter_pack_kernel, dim3(flat_blocks), dim3(kFlatThreads), 0, st,
                       static_cast<const uint2*>(hits), static_cast<const float4*>(normals), rec, n);
    const dim3 grid((W + kFilterTile - 1u) / kFilterTile, (H + kFilterTile - 1u) / kFilterTile);
    const dim3 block(kFilterThreads);
    const float* bufs_r[3] = {static_cast<const float*>(in), static_cast<const float*>(out), pong};
    float* bufs_w[3] = {nullptr, static_cast<float*>(out), pong};
    for (uint32_t s = 0; s < passes; ++s) {
        const float* src = bufs_r[filter_pass_src(s, passes)];
        float* dst = bufs_w[filter_pass_dst(s, passes)];
        const int step = static_cast<int>(filter_pass_step(s));
        if (channels == 4u) launch_pass<4>(grid, block, st, rec, src, dst, W, H, step, depth_sigma, normal_power);
        else launch_pass<1>(grid, block, st, rec, src, dst, W, H, step, depth_sigma, normal_power);
    }
    return hipGetLastError();
}

// rgba8: W*H packed pixels, modified in place; layer: W*H floats
hipError_t launch_apply_layer(uint32_t* rgba8, const float* layer, uint32_t W, uint32_t H, float floor,
                              hipStream_t st) {
    if (W == 0 || H == 0) return hipSuccess;
    const size_t n = static_cast<size_t>(W) * H;
    const uint32_t blocks = static_cast<uint32_t>((n + kFlatThreads - 1u) / kFlatThreads);
    hipLaunchKernelGGL(apply_layer_kernel, dim3(blocks), dim3(kFlatThreads), 0, st, rgba8, layer, n, floor,
                       1.0f - floor);
    return hipGetLastError();
}

// rgba8: W*H packed pixels, modified in place; layer4: W*H float4; albedo: W*H packed RGBA8, or null (white)
hipError_t launch_add_layer(uint32_t* rgba8, const void* layer4, const uint32_t* albedo, uint32_t W, uint32_t H,
                            float gain, hipStream_t st) {
    if (W == 0 || H == 0) return hipSuccess;
    const size_t n = static_cast<size_t>(W) * H;
    const uint32_t blocks = static_cast<uint32_t>((n + kFlatThreads - 1u) / kFlatThreads);
    const float* layer = static_cast<const float*>(layer4);
    if (albedo)
        hipLaunchKernelGGL((add_layer_kernel<true>), dim3(blocks), dim3(kFlatThreads), 0, st, rgba8, layer, albedo, n, gain);
    else
        hipLaunchKernelGGL((add_layer_kernel<false>), dim3(blocks), dim3(kFlatThreads), 0, st, rgba8, layer, albedo, n, gain);
    return hipGetLastError();
}

}  // namespace rtamd
