// rt_layer.h — a per-pixel float layer's pixel as the layer kernels move it
// (rt_filter.hip, rt_reproject.hip): one channel is one dword, four channels one
// dwordx4 (the C ABI asks 16-byte alignment of a four-channel layer).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rtamd {

// a layer's pixel as kC floats: one dword or one dwordx4
template <uint32_t kC>
struct LayerPixel;
template <>
struct LayerPixel<1> {
    float v[1];
    __device__ __forceinline__ void load(const float* p, size_t i) { v[0] = p[i]; }
    __device__ __forceinline__ void store(float* p, size_t i) const { p[i] = v[0]; }
};
template <>
struct alignas(16) LayerPixel<4> {
    float v[4];
    __device__ __forceinline__ void load(const float* p, size_t i) {
        const float4 q = reinterpret_cast<const float4*>(p)[i];
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    }
    __device__ __forceinline__ void store(float* p, size_t i) const {
        reinterpret_cast<float4*>(p)[i] = make_float4(v[0], v[1], v[2], v[3]);
    }
};

}  // namespace rtamd
