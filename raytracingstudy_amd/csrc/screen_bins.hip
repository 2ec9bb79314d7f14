// screen_bins.hip — the per-frame screen-space bins of the primary rays
// (DESIGN.md 5.1 round 10): for this frame's camera, every 8x8-pixel bin gets
// the list of spheres a sample of its pixels can meet, nearest first by a
// lower bound on t; rt_bins.h answers the primary rays from it.
//
// Queued on the frame's stream before the frame kernel, every plain frame (the
// camera moves every frame in the Displayer), with no host synchronisation:
//   memset            the bins' counts and cursors, bins_decide's words, the
//                     info words (one allocation, one memset)
//   bins_count        per sphere: its class and rectangle (rt_bins_math.h,
//                     f64), one atomic per bin it overlaps; wide spheres
//                     join the frame-level list
//   exclusive scan    counts -> each bin's first entry (hipCUB)
//   bins_decide       a bin a thread: totals, the frame's fallback flag (entries
//                     over the buffer, wide list overflowed, lists too long on
//                     average), mirrored into the renderer's pinned words
//   bins_fill         per sphere: its entry into every bin it overlaps
//   bins_sort         a wave per bin: the header, the list sorted by
//                     (near bound, sphere index), a lane an entry, and the
//                     bin's tile words, a lane a wave tile (round 15)
// The order inside a list is a tracing order only: results do not depend on it.
#include <hipcub/hipcub.hpp>

#include "rt_bins_math.h"
#include "rt_host.h"

namespace rtamd {

namespace {

// The first leaf reference of every sphere (made once per scene): the bins'
// entries carry it, so a hit is shaded by reference like the walk's.  A slot
// counts only when its record is its sphere's (a line-packed layout's gaps
// name sphere 0).
__global__ void __launch_bounds__(kBlockThreads)
    first_ref_kernel(const float4* __restrict__ prim_sp, const uint32_t* __restrict__ prim_idx,
                     uint32_t n_slots, const float4* __restrict__ spheres, uint32_t n_spheres,
                     uint32_t* __restrict__ first_ref) {
    const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
    if (i >= n_slots) return;
    const uint32_t k = prim_idx[i];
    if (k >= n_spheres) return;
    const float4 a = prim_sp[i], b = spheres[k];
    if (__float_as_uint(a.x) != __float_as_uint(b.x) || __float_as_uint(a.y) != __float_as_uint(b.y) ||
        __float_as_uint(a.z) != __float_as_uint(b.z) || __float_as_uint(a.w) != __float_as_uint(b.w))
        return;
    atomicMin(first_ref + k, i);
}

struct BinCam {
    float K[9], R[9], o[3];
};

__device__ __forceinline__ BinRect rect_of(const float4 s, const BinCam& c, uint32_t W, uint32_t H,
                                           double shrink) {
    const float sp[4] = {s.x, s.y, s.z, s.w};
    return sphere_screen_rect(sp, c.K, c.R, c.o, W, H, shrink);
}

// per sphere {x0 | x1 << 16, y0 | y1 << 16, near bits, class}
__global__ void __launch_bounds__(kBlockThreads)
    bins_count_kernel(const float4* __restrict__ spheres, const uint32_t* __restrict__ first_ref,
                      uint32_t n, BinCam cam, uint32_t W, uint32_t H, double shrink, uint32_t nbx,
                      uint4* __restrict__ rects, uint32_t* __restrict__ counts,
                      uint32_t* __restrict__ info, uint4* __restrict__ wide) {
    const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t ref = first_ref[i];
    BinRect rc;
    rc.cls = kBinDropped;
    const float4 s = spheres[i];
    if (ref != kNoHit) rc = rect_of(s, cam, W, H, shrink);  // (a sphere in no leaf: no walk finds it either)
    rects[i] = make_uint4(rc.x0 | (rc.x1 << 16), rc.y0 | (rc.y1 << 16), __float_as_uint(rc.near_t), rc.cls);
    if (rc.cls == kBinWide) {
        const uint32_t k = atomicAdd(info + kBinInfoWide, 1u);
        if (k < kBinWideCap) {
            wide[2u * k] = make_uint4(__float_as_uint(s.x), __float_as_uint(s.y), __float_as_uint(s.z),
                                      __float_as_uint(s.w));
            wide[2u * k + 1u] = make_uint4(i, ref, 0u | (7u << 4) | (0u << 8) | (7u << 12), __float_as_uint(rc.near_t));
        }
    } else if (rc.cls == kBinBinned) {
        for (uint32_t by = rc.y0 >> kBinShift; by <= (rc.y1 >> kBinShift); ++by)
            for (uint32_t bx = rc.x0 >> kBinShift; bx <= (rc.x1 >> kBinShift); ++bx)
                atomicAdd(counts + by * nbx + bx, 1u);
    }
}

// A bin a thread (round 19; one block of 256 threads walked 127 bins each with
// dependent loads, 20 us of latency on the frame's stream at 1080p).  A block
// reduces its bins to {non-empty, longest, over the cap} and adds them to the
// `dec` words (zeroed by the build's memset) with device-scope atomics; the
// block that arrives last, by the counter among them, reads the sums and
// writes the frame's words.  Nobody waits for another block; the sums are of
// integers, so two builds of one frame give the same words.
// offs[nb] = the total (the scan ran over nb + 1 counts, the last 0).
__global__ void __launch_bounds__(kBlockThreads)
    bins_decide_kernel(const uint32_t* __restrict__ counts, const uint32_t* __restrict__ offs, uint32_t nb,
                       uint32_t capacity, uint32_t cap, uint32_t mean_max, uint32_t frame_id,
                       uint32_t* __restrict__ dec, uint32_t* __restrict__ info,
                       uint32_t* __restrict__ mirror) {
    constexpr uint32_t kWaves = kBlockThreads / 64u;
    __shared__ uint32_t s_ne[kWaves], s_mx[kWaves], s_ov[kWaves];
    const uint32_t b = blockIdx.x * kBlockThreads + threadIdx.x;
    const uint32_t c = b < nb ? counts[b] : 0u;
    uint32_t ne = c ? 1u : 0u, mx = c, ov = c > cap ? 1u : 0u;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        ne += __shfl_xor(ne, off, 64);
        mx = max(mx, static_cast<uint32_t>(__shfl_xor(mx, off, 64)));
        ov += __shfl_xor(ov, off, 64);
    }
    if ((threadIdx.x & 63u) == 0u) {
        s_ne[threadIdx.x >> 6] = ne;
        s_mx[threadIdx.x >> 6] = mx;
        s_ov[threadIdx.x >> 6] = ov;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t w = 1; w < kWaves; ++w) {
            ne += s_ne[w];
            mx = max(mx, s_mx[w]);
            ov += s_ov[w];
        }
        if (ne) atomicAdd(dec + kBinDecNonEmpty, ne);
        if (mx) atomicMax(dec + kBinDecLongest, mx);
        if (ov) atomicAdd(dec + kBinDecOver, ov);
        // (release: this block's adds before its arrival; acquire: every
        // block's adds before the last one's reads)
        __threadfence();
        if (atomicAdd(dec + kBinDecArrived, 1u) != gridDim.x - 1u) return;
        __threadfence();
        ne = __hip_atomic_load(dec + kBinDecNonEmpty, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        mx = __hip_atomic_load(dec + kBinDecLongest, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ov = __hip_atomic_load(dec + kBinDecOver, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t total = offs[nb], nw = info[kBinInfoWide];
        uint32_t flag = 0u;
        if (total > capacity) flag |= kBinFlagCapacity;
        if (nw > kBinWideCap) flag |= kBinFlagWide;
        if (static_cast<unsigned long long>(total) > static_cast<unsigned long long>(mean_max) * ne)
            flag |= kBinFlagDense;
        const uint32_t w[kBinInfoWords] = {flag, nw, total, ne, mx, ov, frame_id, 0u};
        for (uint32_t k = 0; k < kBinInfoWords; ++k) {
            info[k] = w[k];
            // the renderer's pinned copy (plain system-scope stores, the frame id last)
            if (k != kBinInfoFrame) __hip_atomic_store(mirror + k, w[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        __hip_atomic_store(mirror + kBinInfoFrame, frame_id, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

__global__ void __launch_bounds__(kBlockThreads)
    bins_fill_kernel(const float4* __restrict__ spheres, const uint32_t* __restrict__ first_ref, uint32_t n,
                     const uint4* __restrict__ rects, const uint32_t* __restrict__ offs,
                     uint32_t* __restrict__ cursor, const uint32_t* __restrict__ info, uint32_t nbx,
                     uint32_t capacity, uint4* __restrict__ ent) {
    if (info[kBinInfoFlag]) return;  // the frame walks: nothing reads the entries
    const uint32_t i = blockIdx.x * kBlockThreads + threadIdx.x;
    if (i >= n) return;
    const uint4 rc = rects[i];
    if (rc.w != kBinBinned) return;
    const float4 s = spheres[i];
    const uint32_t ref = first_ref[i];
    const uint32_t x0 = rc.x & 0xFFFFu, x1 = rc.x >> 16, y0 = rc.y & 0xFFFFu, y1 = rc.y >> 16;
    const uint4 rec = make_uint4(__float_as_uint(s.x), __float_as_uint(s.y), __float_as_uint(s.z),
                                 __float_as_uint(s.w));
    for (uint32_t by = y0 >> kBinShift; by <= (y1 >> kBinShift); ++by)
        for (uint32_t bx = x0 >> kBinShift; bx <= (x1 >> kBinShift); ++bx) {
            const uint32_t b = by * nbx + bx;
            const uint32_t e = offs[b] + atomicAdd(cursor + b, 1u);
            if (e >= capacity) continue;  // (never: the flag is clear, so the total fits)
            // the rectangle's pixels inside this bin, bin-local
            const uint32_t px = bx << kBinShift, py = by << kBinShift;
            const uint32_t lx0 = x0 > px ? x0 - px : 0u, lx1 = min(x1 - px, kBinSide - 1u);
            const uint32_t ly0 = y0 > py ? y0 - py : 0u, ly1 = min(y1 - py, kBinSide - 1u);
            ent[2ull * e] = rec;
            ent[2ull * e + 1ull] = make_uint4(i, ref, lx0 | (lx1 << 4) | (ly0 << 8) | (ly1 << 12), rc.z);
        }
}

// A wave per bin: the header {first entry, count | kBinWalk}; a list of
// 2 .. cap <= 64 entries is sorted ascending by (near bound, sphere index): a
// lane holds an entry, counts the entries before it and stores its own there.
// Then a lane owns one of the bin's tpb wave tiles (tw x th pixels) and
// gathers its tile word (rt_bins_math.h) over the cnt entries: bit `rank` for
// every entry whose rectangle overlaps the tile; lists of one entry too.
__global__ void __launch_bounds__(kBlockThreads)
    bins_sort_kernel(const uint32_t* __restrict__ counts, const uint32_t* __restrict__ offs, uint32_t nb,
                     uint32_t cap, const uint32_t* __restrict__ info, uint2* __restrict__ hdr,
                     uint4* __restrict__ ent, uint32_t tw, uint32_t th, uint32_t tpb,
                     unsigned long long* __restrict__ tiles) {
    const uint32_t b = blockIdx.x * (kBlockThreads / 64u) + (threadIdx.x >> 6);
    if (b >= nb) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t cnt = counts[b], off = offs[b];
    if (lane == 0u) hdr[b] = make_uint2(off, cnt > cap ? kBinWalk : cnt);
    if (info[kBinInfoFlag] || cnt < 1u || cnt > cap || cnt > 64u) return;
    uint4 a = make_uint4(0u, 0u, 0u, 0u), m = make_uint4(0u, 0u, 0u, 0u);
    if (lane < cnt) {
        a = ent[2ull * (off + lane)];
        m = ent[2ull * (off + lane) + 1ull];
    }
    // near bounds are non-negative floats: they order as their bits
    const unsigned long long key = (static_cast<unsigned long long>(m.w) << 32) | m.x;
    uint32_t rank = 0u;
    for (uint32_t k = 0; k < cnt; ++k) {
        const unsigned long long o = __shfl(key, static_cast<int>(k), 64);
        rank += o < key ? 1u : 0u;
    }
    // (every lane has read its entry: the shuffles above are after the loads)
    if (lane < cnt && cnt >= 2u) {
        ent[2ull * (off + rank)] = a;
        ent[2ull * (off + rank) + 1ull] = m;
    }
    // (the keys of a list differ, each sphere enters a bin once: the ranks are 0 .. cnt - 1)
    unsigned long long word = 0ull;
    for (uint32_t k = 0; k < cnt; ++k) {
        const uint32_t rc = __shfl(m.z, static_cast<int>(k), 64);
        const uint32_t rk = __shfl(rank, static_cast<int>(k), 64);
        if (lane < tpb && bin_rect_overlaps_tile(rc, lane, tw, th)) word |= 1ull << rk;
    }
    if (lane < tpb) tiles[static_cast<size_t>(b) * tpb + lane] = word;
}

}  // namespace

hipError_t launch_first_refs(const float4* prim_sp, const uint32_t* prim_idx, uint32_t n_slots,
                             const float4* spheres, uint32_t n_spheres, uint32_t* first_ref,
                             hipStream_t st) {
    hipError_t e = hipMemsetAsync(first_ref, 0xFF, static_cast<size_t>(n_spheres ? n_spheres : 1u) * sizeof(uint32_t), st);
    if (e != hipSuccess) return e;
    if (n_slots)
        hipLaunchKernelGGL(first_ref_kernel, dim3((n_slots + kBlockThreads - 1) / kBlockThreads),
                           dim3(kBlockThreads), 0, st, prim_sp, prim_idx, n_slots, spheres, n_spheres, first_ref);
    return hipGetLastError();
}

size_t bins_scan_temp_bytes(uint32_t n_items) {
    size_t bytes = 0;
    uint32_t* p = nullptr;
    if (hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, p, p, n_items, nullptr) != hipSuccess) return 0;
    return bytes ? bytes : 1;
}

hipError_t launch_screen_bins(const BinBuild& b, hipStream_t st) {
    const uint32_t nb = b.nbx * b.nby;
    hipError_t e;
    // counts[nb + 1], cursor[nb], bins_decide's words and the info words are one allocation
    if ((e = hipMemsetAsync(b.counts, 0, bin_zeroed_words(nb) * sizeof(uint32_t), st)) != hipSuccess) return e;
    BinCam cam;
    memcpy(cam.K, b.K, sizeof(cam.K));
    memcpy(cam.R, b.R, sizeof(cam.R));
    memcpy(cam.o, b.o, sizeof(cam.o));
    const uint32_t ns = (b.n_spheres + kBlockThreads - 1) / kBlockThreads;
    if (b.n_spheres)
        hipLaunchKernelGGL(bins_count_kernel, dim3(ns), dim3(kBlockThreads), 0, st, b.spheres, b.first_ref,
                           b.n_spheres, cam, b.W, b.H, b.shrink, b.nbx, b.rects, b.counts, b.info, b.wide);
    size_t bytes = b.temp_bytes;
    if ((e = hipcub::DeviceScan::ExclusiveSum(b.temp, bytes, b.counts, b.offs, nb + 1u, st)) != hipSuccess)
        return e;
    hipLaunchKernelGGL(bins_decide_kernel, dim3((nb + kBlockThreads - 1) / kBlockThreads), dim3(kBlockThreads),
                       0, st, b.counts, b.offs, nb, b.capacity, b.cap, b.mean_max, b.frame_id, b.decide,
                       b.info, b.mirror);
    if (b.n_spheres)
        hipLaunchKernelGGL(bins_fill_kernel, dim3(ns), dim3(kBlockThreads), 0, st, b.spheres, b.first_ref,
                           b.n_spheres, b.rects, b.offs, b.cursor, b.info, b.nbx, b.capacity, b.ent);
    hipLaunchKernelGGL(bins_sort_kernel, dim3((nb + kBlockThreads / 64u - 1u) / (kBlockThreads / 64u)),
                       dim3(kBlockThreads), 0, st, b.counts, b.offs, nb, b.cap, b.info, b.hdr, b.ent, b.tw,
                       b.th, bin_tiles_per_bin(b.tw, b.th), b.tiles);
    return hipGetLastError();
}

}  // namespace rtamd
