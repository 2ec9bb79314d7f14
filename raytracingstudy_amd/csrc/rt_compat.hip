// rt_compat.hip — the kernels that restate the reference's frame, and the one
// that puts packed tiles back into it:
//   * compat_kernel : byte-exact restatement of the reference's single CUDA
//                     kernel `raytracing` (src/renderer.cu:57-82, grid
//                     (W/32+1, H/32+1) x block (32,32): root-box slab test,
//                     R = Octree::traverse() = 200, miss colour), and its
//                     tile-packed form compat_tiles_kernel.
//   * unpack_kernel : scatters packed per-rank tiles into the frame.
// Their launchers follow.  The scene kernels are rt_kernels.hip.
// Compiled with -ffp-contract=off: every f32/f64 expression is evaluated in
// source order with IEEE division/sqrt, exactly like oracle/oracle.c.
#include <hip/hip_runtime.h>

#include "rt_params.h"
#include "rt_shade.h"  // get_ray, sat

namespace rtamd {

// src/renderer.cu:3-55 — `hit_sphere`: slab test of the root box [0,1.28]^3
// with the negative-direction axes mirrored about the centre 0.64 (f32
// origin/inverse widened to f64, f64 slab products rounded to f32, NaN-dropping
// fmaxf/fminf, no t >= 0 test).
__device__ __forceinline__ double mirror_o(float o, float d) {
    return d < 0.0f ? static_cast<double>(0.64f * 2.0f - o) : static_cast<double>(o);
}
__device__ __forceinline__ double mirror_inv(float d) {
    return d < 0.0f ? static_cast<double>(-(1.0f / d)) : static_cast<double>(1.0f / d);
}
__device__ __forceinline__ bool hit_root_box(const float o[3], float d0, float d1, float d2) {
    const double bmin = static_cast<double>(0.0f);
    const double bmax = static_cast<double>(1.28f);
    const double rx = mirror_o(o[0], d0), ry = mirror_o(o[1], d1), rz = mirror_o(o[2], d2);
    const double ix = mirror_inv(d0), iy = mirror_inv(d1), iz = mirror_inv(d2);
    const float tx0 = static_cast<float>((bmin - rx) * ix);
    const float tx1 = static_cast<float>((bmax - rx) * ix);
    const float ty0 = static_cast<float>((bmin - ry) * iy);
    const float ty1 = static_cast<float>((bmax - ry) * iy);
    const float tz0 = static_cast<float>((bmin - rz) * iz);
    const float tz1 = static_cast<float>((bmax - rz) * iz);
    return fmaxf(fmaxf(tx0, ty0), tz0) < fminf(fminf(tx1, ty1), tz1);
}

// getRay under ONE CANDIDATE contraction of include/camera.h:31-34 (dz = 1
// folds; an fadd of two products fused through its first operand), a guess at
// what nvcc's default -fmad=true does to the reference binary.  Which order
// that binary really uses cannot be checked without nvcc: unpinned
// (DESIGN.md 2.1).  The default (get_ray) is the SOURCE semantics.  Same
// operations as the oracle's contracted getRay, contract = 1.
__device__ __forceinline__ void get_ray_fma(const CamArgs& c, float u, float v, float& wx,
                                            float& wy, float& wz) {
    const float dx = (u - c.K[2]) / c.K[0];
    const float dy = (v - c.K[5]) / c.K[4];
    wx = fmaf(c.R[0], dx, c.R[3] * dy) + c.R[6];
    wy = fmaf(c.R[1], dx, c.R[4] * dy) + c.R[7];
    wz = fmaf(c.R[2], dx, c.R[5] * dy) + c.R[8];
    const float len = sqrtf(fmaf(wz, wz, fmaf(wx, wx, wy * wy)));
    wx /= len;
    wy /= len;
    wz /= len;
}

__device__ __forceinline__ uint32_t compat_pixel(const CamArgs& cam, uint32_t x, uint32_t y,
                                                 uint32_t contract) {
    float d0, d1, d2;
    if (contract)
        get_ray_fma(cam, static_cast<float>(x), static_cast<float>(y), d0, d1, d2);
    else
        get_ray(cam, static_cast<float>(x), static_cast<float>(y), d0, d1, d2);
    if (hit_root_box(cam.o, d0, d1, d2)) return 0xFFFFFFFFu;
    const uint32_t g = static_cast<uint32_t>(sat(d1) * 255.0f);
    const uint32_t b = static_cast<uint32_t>(sat(d2) * 255.0f);
    return 200u | (g << 8) | (b << 16) | (255u << 24);
}

// One wave = 64 consecutive pixels of a row; one packed 32-bit store per lane.
__global__ void __launch_bounds__(kBlockThreads) compat_kernel(FrameArgs a) {
    const uint32_t x = blockIdx.x * 64u + (threadIdx.x & 63u);
    const uint32_t y = blockIdx.y * 4u + (threadIdx.x >> 6);
    if (x >= a.W || y >= a.H) return;
    __builtin_nontemporal_store(compat_pixel(a.cam, x, y, a.contract), a.out8 + (size_t)y * a.W + x);
}

// Tile-packed compat: block = 64 x 4 strip of one tile.
__global__ void __launch_bounds__(kBlockThreads) compat_tiles_kernel(FrameArgs a) {
    const uint32_t ts = a.tile_size;
    const uint32_t strips = ts / 4u * (ts / 64u);
    const uint32_t k = blockIdx.x / strips;
    const uint32_t sidx = blockIdx.x % strips;
    const uint32_t lx = (sidx % (ts / 64u)) * 64u + (threadIdx.x & 63u);
    const uint32_t ly = (sidx / (ts / 64u)) * 4u + (threadIdx.x >> 6);
    const uint32_t tile = a.tiles[k];
    const uint32_t x = (tile % a.tiles_x) * ts + lx;
    const uint32_t y = (tile / a.tiles_x) * ts + ly;
    const uint32_t v = (x < a.W && y < a.H) ? compat_pixel(a.cam, x, y, a.contract) : 0u;
    a.out8[(size_t)k * ts * ts + ly * ts + lx] = v;
}

__global__ void __launch_bounds__(kBlockThreads)
    unpack_kernel(const uint32_t* __restrict__ packed, const uint32_t* __restrict__ tiles,
                  uint32_t n_tiles, uint32_t ts, uint32_t tiles_x, uint32_t W, uint32_t H,
                  uint32_t* __restrict__ img) {
    const size_t i = (size_t)blockIdx.x * kBlockThreads + threadIdx.x;
    const size_t per = (size_t)ts * ts;
    if (i >= per * n_tiles) return;
    const uint32_t k = static_cast<uint32_t>(i / per);
    const uint32_t r = static_cast<uint32_t>(i % per);
    const uint32_t tile = tiles[k];
    if (tile == 0xFFFFFFFFu) return;  // RT_TILE_SKIP: a padding slot
    const uint32_t x = (tile % tiles_x) * ts + r % ts;
    const uint32_t y = (tile / tiles_x) * ts + r / ts;
    if (x < W && y < H) img[(size_t)y * W + x] = packed[i];
}

// ---------------------------------------------------------------------------
// launchers (called from rt_frame.cpp)
// ---------------------------------------------------------------------------

hipError_t launch_compat(const FrameArgs& a, hipStream_t st) {
    if (a.tiles) {
        const uint32_t strips = a.tile_size / 4u * (a.tile_size / 64u);
        hipLaunchKernelGGL(compat_tiles_kernel, dim3(a.n_tiles * strips), dim3(kBlockThreads), 0,
                           st, a);
    } else {
        hipLaunchKernelGGL(compat_kernel, dim3((a.W + 63) / 64, (a.H + 3) / 4), dim3(kBlockThreads),
                           0, st, a);
    }
    return hipGetLastError();
}

hipError_t launch_unpack(const uint32_t* packed, const uint32_t* tiles, uint32_t n_tiles,
                         uint32_t ts, uint32_t tiles_x, uint32_t W, uint32_t H, uint32_t* img,
                         hipStream_t st) {
    const size_t total = (size_t)ts * ts * n_tiles;
    const uint32_t blocks = static_cast<uint32_t>((total + kBlockThreads - 1) / kBlockThreads);
    if (blocks) {
        hipLaunchKernelGGL(unpack_kernel, dim3(blocks), dim3(kBlockThreads), 0, st, packed, tiles,
                           n_tiles, ts, tiles_x, W, H, img);
    }
    return hipGetLastError();
}

}  // namespace rtamd
