// rt_records.hip — the per-reference records the walks screen and shade by:
// camera-relative and image-plane screens (per frame camera), light-plane
// screen (per scene and light), albedo by leaf reference (per scene).  One
// thread per leaf reference; launched from rt_frame.cpp and rt_scene.cpp.
// Compiled like rt_kernels.hip (-ffp-contract=off, IEEE division / sqrt).
#include <hip/hip_runtime.h>

#include "rt_params.h"

namespace rtamd {

// Camera-relative screen records of every leaf reference (and the kPrimPad
// tail) for camera origin o (SceneArgs::prim_cam):
// {o - c in f32, exactly isect's oc}, and C' = |o - c|^2 - r^2 minus the
// slack, computed in f64 and rounded toward -inf, so C' <= the bound the
// screen's soundness needs.  One thread per reference: 16 B read, 16 B written.
__global__ void __launch_bounds__(kBlockThreads)
    cam_screen_kernel(const float4* __restrict__ prim_sp, uint32_t n, float ox, float oy, float oz,
                      float4* __restrict__ out) {
    const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
    if (i >= n) return;
    const float4 c = prim_sp[i];
    const float x = ox - c.x, y = oy - c.y, z = oz - c.z;
    const double oo = static_cast<double>(x) * x + static_cast<double>(y) * y + static_cast<double>(z) * z;
    const double rr = static_cast<double>(c.w) * c.w;
    const double u = 1.0 / 16777216.0;  // 2^-24, the f32 unit roundoff
    const double cd = oo - rr - (kScreenSlackOc * u) * oo - (kScreenSlackR * u) * rr;
    out[i] = make_float4(x, y, z, __double2float_rd(cd));
}

// Light-plane screen records (SceneArgs::prim_shd8): per
// reference the centre's {u, v} = {c.e1, c.e2} (f64, rounded to nearest); the
// radius term is the largest rr' = ((r (1 + 4u) + delta)^2 (1 + 4u)) rounded
// up, delta = the slack for this scene (kShadowSlackM u M).  One thread per
// reference.
__global__ void __launch_bounds__(kBlockThreads)
    shd_screen_kernel(const float4* __restrict__ prim_sp, uint32_t n, float e0, float e1, float e2,
                      float e3, float e4, float e5, double delta, float2* __restrict__ out8,
                      uint32_t* __restrict__ rr_max) {
    const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
    uint32_t rb = 0u;
    if (i < n) {
        const float4 c = prim_sp[i];
        const double u = static_cast<double>(c.x) * e0 + static_cast<double>(c.y) * e1 + static_cast<double>(c.z) * e2;
        const double v = static_cast<double>(c.x) * e3 + static_cast<double>(c.y) * e4 + static_cast<double>(c.z) * e5;
        const double ur = 1.0 / 16777216.0;
        const double rg = static_cast<double>(c.w) * (1.0 + 4.0 * ur) + delta;
        const float rr = __double2float_ru(rg * rg * (1.0 + 4.0 * ur));
        out8[i] = make_float2(static_cast<float>(u), static_cast<float>(v));
        rb = __float_as_uint(rr);
    }
    // the largest rr' (non-negative floats order as their bits; a NaN
    // radius, the test-only pad fill, orders above every number): the
    // block's maximum into rr_max[blockIdx.x], reduced by max_bits_kernel
    // (atomics on one word serialise across the XCDs: one per record, or one
    // per wave, took C5d's 4.9 M records 0.87 ms)
    __shared__ uint32_t wmax[kBlockThreads / 64];
    for (int d = 32; d > 0; d >>= 1) rb = max(rb, static_cast<uint32_t>(__shfl_xor(static_cast<int>(rb), d, 64)));
    if ((threadIdx.x & 63u) == 0u) wmax[threadIdx.x >> 6] = rb;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t m = 0u;
        for (uint32_t w = 0; w < kBlockThreads / 64; ++w) m = max(m, wmax[w]);
        rr_max[blockIdx.x] = m;
    }
}

// out[0] = the largest of in[0 .. n) (one block)
__global__ void __launch_bounds__(kBlockThreads)
    max_bits_kernel(const uint32_t* __restrict__ in, uint32_t n, uint32_t* __restrict__ out) {
    __shared__ uint32_t wmax[kBlockThreads / 64];
    uint32_t m = 0u;
    for (uint32_t i = threadIdx.x; i < n; i += kBlockThreads) m = max(m, in[i]);
    for (int d = 32; d > 0; d >>= 1) m = max(m, static_cast<uint32_t>(__shfl_xor(static_cast<int>(m), d, 64)));
    if ((threadIdx.x & 63u) == 0u) wmax[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t w = 1; w < kBlockThreads / 64; ++w) m = max(m, wmax[w]);
        out[0] = m;
    }
}

hipError_t launch_shd_screen(const float4* prim_sp, uint32_t n, const float e[6], double delta,
                             float2* out8, uint32_t* rr_max, hipStream_t st) {
    // rr_max: (blocks + 1) words, the scene's largest rr' bits in the last
    if (n) {
        const uint32_t nb = (n + kBlockThreads - 1) / kBlockThreads;
        hipLaunchKernelGGL(shd_screen_kernel, dim3(nb), dim3(kBlockThreads), 0, st, prim_sp, n, e[0],
                           e[1], e[2], e[3], e[4], e[5], delta, out8, rr_max);
        hipLaunchKernelGGL(max_bits_kernel, dim3(1), dim3(kBlockThreads), 0, st, rr_max, nb, rr_max + nb);
    }
    return hipGetLastError();
}

hipError_t launch_cam_screen(const float4* prim_sp, uint32_t n, const float o[3], float4* out,
                             hipStream_t st) {
    if (n) {
        hipLaunchKernelGGL(cam_screen_kernel, dim3((n + kBlockThreads - 1) / kBlockThreads),
                           dim3(kBlockThreads), 0, st, prim_sp, n, o[0], o[1], o[2], out);
    }
    return hipGetLastError();
}

// Image-plane screen records (SceneArgs::prim_cam8).
// For basis B (f32 rows, orthonormal to f32 rounding) and camera origin o,
// a sphere's centre direction a = B(c - o)/|c - o| projects to q = a.xy/a.z.
// A ray the exact test accepts passes within r' = r (1 + 1e-6) of c, so its
// direction b is within theta (sin theta = r'/|c - o|) of a, and for unit
// vectors |q_a - q_b| <= |a x b| / (a_z b_z) <= sin theta / (a_z cos(beta +
// theta)), beta the angle of a from B's z axis.  rho adds the f32 errors of
// the lane's point (4e-6 (1 + |q| + rho)^2, ~5x the bound), the stored
// centre's (its 8 low mantissa bits carry rho^2: <= 2^-14 |q| a component)
// and 1e-5 relative; rho^2 is rounded up to bf16.  Spheres near or behind
// the camera plane, or a frame whose rays B does not keep in front (ok = 0),
// get rho^2 = +inf: always passed.
__global__ void __launch_bounds__(kBlockThreads)
    cam8_screen_kernel(const float4* __restrict__ prim_sp, uint32_t n, float ox, float oy, float oz,
                       float b0, float b1, float b2, float b3, float b4, float b5, float b6, float b7,
                       float b8, uint32_t ok, float2* __restrict__ out) {
    const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
    if (i >= n) return;
    const float4 c = prim_sp[i];
    const double vx = static_cast<double>(c.x) - ox, vy = static_cast<double>(c.y) - oy,
                 vz = static_cast<double>(c.z) - oz;
    const double X = static_cast<double>(b0) * vx + static_cast<double>(b1) * vy + static_cast<double>(b2) * vz;
    const double Y = static_cast<double>(b3) * vx + static_cast<double>(b4) * vy + static_cast<double>(b5) * vz;
    const double Z = static_cast<double>(b6) * vx + static_cast<double>(b7) * vy + static_cast<double>(b8) * vz;
    const double dist = sqrt(vx * vx + vy * vy + vz * vz);
    const double rp = static_cast<double>(c.w) * (1.0 + 1e-6);
    uint32_t hx = 0u, hy = 0u, rb = 0x7F800000u;  // rho^2 = +inf: always pass
    bool pass_all = !ok || !(dist > rp * 1.0001) || !(Z > 0.0) || !isfinite(dist) || !(c.w >= 0.0f);
    if (!pass_all) {
        const double az = Z / dist;
        const double beta = acos(fmin(1.0, az));
        const double th = asin(fmin(1.0, rp / dist));
        if (!(beta + th < 1.45)) {  // ~83 degrees: the bound's cos(beta + theta) too small
            pass_all = true;
        } else {
            const float qx = static_cast<float>(X / Z), qy = static_cast<float>(Y / Z);
            const double q = fabs(static_cast<double>(qx)) + fabs(static_cast<double>(qy));
            const double rho_g = sin(th) / (az * cos(beta + th));
            const double eps_c = 1.5 * (1.0 / 16384.0) * q;
            const double m = 1.0 + q + rho_g;
            const double rho = rho_g * (1.0 + 1e-5) + eps_c + 4e-6 * m * m;
            const float r2 = __double2float_ru(rho * rho * (1.0 + 1e-6));
            uint32_t bits = __float_as_uint(r2);
            if (bits & 0xFFFFu) bits = (bits & 0xFFFF0000u) + 0x10000u;  // bf16, rounded up
            if (isfinite(r2) && bits < 0x7F800000u) {
                rb = bits;
                hx = __float_as_uint(qx);
                hy = __float_as_uint(qy);
            } else {
                pass_all = true;
            }
        }
    }
    // low bytes: rho^2's bf16, high byte in x, low byte in y
    const uint32_t sx = (hx & ~0xFFu) | (rb >> 24), sy = (hy & ~0xFFu) | ((rb >> 16) & 0xFFu);
    out[i] = make_float2(__uint_as_float(sx), __uint_as_float(sy));
}

hipError_t launch_cam8_screen(const float4* prim_sp, uint32_t n, const float o[3], const float B[9],
                              uint32_t ok, float2* out, hipStream_t st) {
    if (n) {
        hipLaunchKernelGGL(cam8_screen_kernel, dim3((n + kBlockThreads - 1) / kBlockThreads),
                           dim3(kBlockThreads), 0, st, prim_sp, n, o[0], o[1], o[2], B[0], B[1], B[2],
                           B[3], B[4], B[5], B[6], B[7], B[8], ok, out);
    }
    return hipGetLastError();
}

// Albedo by leaf reference (SceneArgs::prim_al): out[i] = albedo[prim_idx[i]]
// for the n real reference slots (a packed layout's gaps name sphere 0).
__global__ void __launch_bounds__(kBlockThreads)
    albedo_refs_kernel(const uint32_t* __restrict__ prim_idx, const uint32_t* __restrict__ albedo,
                       uint32_t n, uint32_t n_spheres, uint32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t k = prim_idx[i];
    out[i] = k < n_spheres ? albedo[k] : 0u;
}

hipError_t launch_albedo_refs(const uint32_t* prim_idx, const uint32_t* albedo, uint32_t n,
                              uint32_t n_spheres, uint32_t* out, hipStream_t st) {
    if (n) {
        hipLaunchKernelGGL(albedo_refs_kernel, dim3((n + kBlockThreads - 1) / kBlockThreads),
                           dim3(kBlockThreads), 0, st, prim_idx, albedo, n, n_spheres, out);
    }
    return hipGetLastError();
}

}  // namespace rtamd
