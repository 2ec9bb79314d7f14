// occluder.hip — per-sphere occluder lists for the frame's shadow rays
// (DESIGN.md §5.1 "Round 7").
//
// Every shadow ray of a renderer has the direction L, and its origin lies
// within R_i of the centre of the sphere i the primary ray hit.  The spheres
// that can occlude it are therefore a property of the scene and the light:
// those whose light-plane disc overlaps sphere i's and that are not wholly
// behind it along L.  Pair rule (f64; its slack terms dwarf f64 rounding):
//   keep j for i  iff  |uv_i - uv_j| <= R_i + sr_j
//                 and  w_j + r_j (1 + kOccBehindR) + R_i + delta >= w_i
// with uv = the centre's light-plane coordinates (the basis of
// shd_screen_kernel), w = c.L, sr_j >= sqrt(rr'_j) of that kernel's record
// and delta its scene slack (kShadowSlackM u M).  A list is sorted
// nearest-first along L (key w_j - r_j, then sphere index), so two builds
// give identical arrays whatever order the atomics ran in.
//
// The builder bins the centres into a uniform grid on the light plane whose
// cells are at least 2 max(R, sr) wide, so a sphere's partners lie in its 3x3
// cells.  count(): per-sphere geometry and bounds, grid parameters, cell
// histogram -> scan -> fill, a bound on the pair work from the histogram
// (over budget: no lists, the pair passes return at once), per-sphere
// candidate counts -> scan.  fill(): the lists, sorted in place, and the
// header of every leaf reference.
#include <hip/hip_runtime.h>
#include <math.h>

#include "octree_gpu.h"
#include "rt_params.h"

namespace rtamd {
namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kScanItems = 8;                       // per thread
constexpr uint32_t kScanBlock = kThreads * kScanItems;   // per block
constexpr uint32_t kGeo = 6;                             // doubles per sphere: u, v, w, R, sr, r

struct OccPar {
    double u0, v0, h;
    double delta, M;
    float L[3], e[6];
    uint32_t gx, gy, gmax;
    uint32_t cap;
    uint32_t off;  // 1: no lists (invalid spheres, or the pair work over budget)
    // reductions of the first pass (floats in an order-preserving encoding)
    uint32_t umin, umax, vmin, vmax, smax;
    OccluderLists::Totals tot;
};

__device__ __forceinline__ uint32_t enc(float f) {
    const uint32_t b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float dec(uint32_t e) {
    return __uint_as_float((e & 0x80000000u) ? (e & 0x7FFFFFFFu) : ~e);
}

__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
    for (int d = 32; d > 0; d >>= 1) v = min(v, static_cast<uint32_t>(__shfl_xor(static_cast<int>(v), d, 64)));
    return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
    for (int d = 32; d > 0; d >>= 1) v = max(v, static_cast<uint32_t>(__shfl_xor(static_cast<int>(v), d, 64)));
    return v;
}

__global__ void occ_init_kernel(OccPar* p, double delta, double M, float l0, float l1, float l2,
                                float e0, float e1, float e2, float e3, float e4, float e5,
                                uint32_t gmax, uint32_t cap) {
    OccPar q{};
    q.delta = delta;
    q.M = M;
    q.L[0] = l0, q.L[1] = l1, q.L[2] = l2;
    q.e[0] = e0, q.e[1] = e1, q.e[2] = e2, q.e[3] = e3, q.e[4] = e4, q.e[5] = e5;
    q.gmax = gmax;
    q.cap = cap;
    q.umin = q.vmin = 0xFFFFFFFFu;
    *p = q;
}

// Pass 0: per-sphere geometry {u, v, w, R, sr, r} and the reductions that
// size the grid.  An invalid sphere is counted (the scene then gets no lists):
// defensive only, rt_set_scene / rt_set_scene_device refuse such scenes, so no
// API path reaches it.
__global__ void __launch_bounds__(kThreads)
    occ_prep_kernel(const float4* __restrict__ spheres, uint32_t n, OccPar* __restrict__ p,
                    double* __restrict__ geo) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    uint32_t umin = 0xFFFFFFFFu, umax = 0u, vmin = 0xFFFFFFFFu, vmax = 0u, smax = 0u, bad = 0u;
    if (i < n) {
        const float4 c = spheres[i];
        const bool ok = isfinite(c.x) && isfinite(c.y) && isfinite(c.z) && isfinite(c.w) && c.w > 0.0f;
        double* g = geo + size_t(kGeo) * i;
        if (ok) {
            const double x = c.x, y = c.y, z = c.z, r = c.w;
            const double u = x * p->e[0] + y * p->e[1] + z * p->e[2];
            const double v = x * p->e[3] + y * p->e[4] + z * p->e[5];
            const double w = x * p->L[0] + y * p->L[1] + z * p->L[2];
            const double ur = 1.0 / 16777216.0;
            const double R = r * (1.0 + kOccRel) +
                             static_cast<double>(kShadowEps) * (1.0 + kOccNormM * ur * p->M / r) +
                             kOccAbsM * ur * p->M;
            // >= sqrt(rr') of shd_screen_kernel's record: rr' = RU((r (1 + 4u) + delta)^2 (1 + 4u))
            const double sr = (r * (1.0 + 4.0 * ur) + p->delta) * (1.0 + 4.0 * ur);
            g[0] = u, g[1] = v, g[2] = w, g[3] = R, g[4] = sr, g[5] = r;
            const float uf = static_cast<float>(u), vf = static_cast<float>(v);
            umin = umax = enc(uf);
            vmin = vmax = enc(vf);
            const double s = R > sr ? R : sr;
            const float sf = __double2float_ru(s);
            smax = isfinite(sf) ? __float_as_uint(sf) : 0x7F7FFFFFu;
            if (!isfinite(uf) || !isfinite(vf) || !isfinite(sf) || !isfinite(w)) bad = 1u;
        } else {
            for (uint32_t k = 0; k < kGeo; ++k) g[k] = 0.0;
            bad = 1u;
        }
        if (bad) umin = vmin = 0xFFFFFFFFu, umax = vmax = smax = 0u;
    }
    umin = wave_min(umin), vmin = wave_min(vmin);
    umax = wave_max(umax), vmax = wave_max(vmax), smax = wave_max(smax);
    const uint32_t nb = static_cast<uint32_t>(__popcll(__ballot(bad != 0u)));
    if ((threadIdx.x & 63u) == 0u) {
        atomicMin(&p->umin, umin);
        atomicMin(&p->vmin, vmin);
        atomicMax(&p->umax, umax);
        atomicMax(&p->vmax, vmax);
        atomicMax(&p->smax, smax);
        if (nb) atomicAdd(&p->tot.n_bad, nb);
    }
}

// The grid: cells at least 2 max(R, sr) wide (a pair's centres are at most
// R_i + sr_j apart), at most gmax cells an axis.
__global__ void occ_grid_kernel(OccPar* p) {
    if (p->tot.n_bad || p->umax < p->umin) {
        p->off = 1u;
        p->tot.skipped = 1u;
        p->gx = p->gy = 1u;
        p->u0 = p->v0 = 0.0;
        p->h = 1.0;
        return;
    }
    const double ulo = dec(p->umin), uhi = dec(p->umax), vlo = dec(p->vmin), vhi = dec(p->vmax);
    const double pad = 1e-6 * (fabs(ulo) + fabs(uhi) + fabs(vlo) + fabs(vhi) + 1.0);
    const double eu = uhi - ulo + 2.0 * pad, ev = vhi - vlo + 2.0 * pad;
    const double smax = __uint_as_float(p->smax);
    double h = 2.0000001 * smax;
    const double ext = eu > ev ? eu : ev;
    if (h * p->gmax < ext) h = ext / p->gmax;
    p->h = h;
    p->u0 = ulo - pad;
    p->v0 = vlo - pad;
    const double fx = floor(eu / h) + 1.0, fy = floor(ev / h) + 1.0;
    p->gx = fx < p->gmax ? static_cast<uint32_t>(fx) : p->gmax;
    p->gy = fy < p->gmax ? static_cast<uint32_t>(fy) : p->gmax;
}

__device__ __forceinline__ uint32_t cell_coord(double x, double x0, double h, uint32_t g) {
    const double f = floor((x - x0) / h);
    return f < 0.0 ? 0u : f >= static_cast<double>(g) ? g - 1u : static_cast<uint32_t>(f);
}

__global__ void __launch_bounds__(kThreads)
    occ_cell_count_kernel(const double* __restrict__ geo, uint32_t n, const OccPar* __restrict__ p,
                          uint32_t* __restrict__ cell_of, uint32_t* __restrict__ cnt) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    uint32_t c = 0u;
    if (!p->off) {
        const double* g = geo + size_t(kGeo) * i;
        c = cell_coord(g[1], p->v0, p->h, p->gy) * p->gx + cell_coord(g[0], p->u0, p->h, p->gx);
        atomicAdd(cnt + c, 1u);
    }
    cell_of[i] = c;
}

__global__ void __launch_bounds__(kThreads)
    occ_cell_fill_kernel(const uint32_t* __restrict__ cell_of, uint32_t n, const OccPar* __restrict__ p,
                         const uint32_t* __restrict__ start, uint32_t* __restrict__ cur,
                         uint32_t* __restrict__ items) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n || p->off) return;
    const uint32_t c = cell_of[i];
    const uint32_t k = start[c] + atomicAdd(cur + c, 1u);
    if (k < n) items[k] = i;
}

// Bound on the pair passes' work: sum over cells of pop(cell) x pop(3x3).
__global__ void __launch_bounds__(kThreads)
    occ_work_kernel(const uint32_t* __restrict__ start, uint32_t nc, OccPar* __restrict__ p) {
    const uint32_t c = blockIdx.x * kThreads + threadIdx.x;
    unsigned long long w = 0ull;
    if (!p->off && c < p->gx * p->gy && c < nc) {
        const uint32_t gx = p->gx, gy = p->gy;
        const uint32_t cx = c % gx, cy = c / gx;
        const unsigned long long pop = start[c + 1u] - start[c];
        if (pop) {
            unsigned long long nb = 0ull;
            for (uint32_t y = cy ? cy - 1u : 0u; y <= min(cy + 1u, gy - 1u); ++y) {
                const uint32_t a = y * gx + (cx ? cx - 1u : 0u), b = y * gx + min(cx + 1u, gx - 1u);
                nb += start[b + 1u] - start[a];
            }
            w = pop * nb;
        }
    }
    for (int d = 32; d > 0; d >>= 1) w += __shfl_xor(w, d, 64);
    if ((threadIdx.x & 63u) == 0u && w) atomicAdd(&p->tot.work, w);
}

__global__ void occ_decide_kernel(OccPar* p, unsigned long long budget) {
    if (p->tot.work > budget) {
        p->off = 1u;
        p->tot.skipped = 1u;
    }
}

// The pair rule (see the head of this file).
__device__ __forceinline__ bool occ_pair(const double* __restrict__ gi, const double* __restrict__ gj,
                                         double delta) {
    const double du = gi[0] - gj[0], dv = gi[1] - gj[1];
    const double reach = gi[3] + gj[4];
    return du * du + dv * dv <= reach * reach &&
           gj[2] + gj[5] * (1.0 + kOccBehindR) + gi[3] + delta >= gi[2];
}
// Sphere i in its own list: an origin made from a hit on i lies at least
// kShadowEps minus the rounding of the hit point (camera inside the gate,
// kOccCamGate) outside it, heading away
// (n.L > 0), so isect cannot accept i when that rounding is small against
// kShadowEps; otherwise i is kept.
__device__ __forceinline__ bool occ_self(const double* __restrict__ gi, double M) {
    return !(kOccSelfM * (1.0 / 16777216.0) * (gi[5] + M) <= 0.75 * static_cast<double>(kShadowEps));
}

// visit(j) for every candidate j of sphere i, in no particular order
template <typename F>
__device__ __forceinline__ void occ_candidates(uint32_t i, const double* __restrict__ geo,
                                               const OccPar* __restrict__ p,
                                               const uint32_t* __restrict__ cell_of,
                                               const uint32_t* __restrict__ start,
                                               const uint32_t* __restrict__ items, F&& visit) {
    const uint32_t gx = p->gx, gy = p->gy;
    const uint32_t c = cell_of[i], cx = c % gx, cy = c / gx;
    const double* gi = geo + size_t(kGeo) * i;
    const double delta = p->delta;
    for (uint32_t y = cy ? cy - 1u : 0u; y <= min(cy + 1u, gy - 1u); ++y) {
        const uint32_t a = start[y * gx + (cx ? cx - 1u : 0u)];
        const uint32_t b = start[y * gx + min(cx + 1u, gx - 1u) + 1u];
        for (uint32_t k = a; k < b; ++k) {
            const uint32_t j = items[k];
            if (j == i ? occ_self(gi, p->M) : occ_pair(gi, geo + size_t(kGeo) * j, delta)) visit(j);
        }
    }
}

__global__ void __launch_bounds__(kThreads)
    occ_pair_count_kernel(const double* __restrict__ geo, uint32_t n, OccPar* __restrict__ p,
                          const uint32_t* __restrict__ cell_of, const uint32_t* __restrict__ start,
                          const uint32_t* __restrict__ items, uint32_t* __restrict__ len,
                          uint2* __restrict__ hdr) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    uint32_t cnt = 0u, capped = 0u;
    if (i < n) {
        if (!p->off) {
            occ_candidates(i, geo, p, cell_of, start, items, [&](uint32_t) { ++cnt; });
            capped = cnt > p->cap ? 1u : 0u;
        }
        len[i] = capped ? 0u : cnt;
        hdr[i] = make_uint2(0u, capped ? kOccWalk : cnt);
    }
    unsigned long long s = cnt;
    for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d, 64);
    const uint32_t nc = static_cast<uint32_t>(__popcll(__ballot(capped != 0u)));
    if ((threadIdx.x & 63u) == 0u) {
        if (s) atomicAdd(&p->tot.cand, s);
        if (nc) atomicAdd(&p->tot.n_capped, nc);
    }
}

__global__ void occ_total_kernel(OccPar* p, const uint32_t* total) { p->tot.entries = *total; }

// The lists: sphere i's candidates at [off_i, off_i + len_i), sorted by
// (w_j - r_j, j) in place, then their sphere records.
__global__ void __launch_bounds__(kThreads)
    occ_fill_kernel(const float4* __restrict__ spheres, const double* __restrict__ geo, uint32_t n,
                    const OccPar* __restrict__ p, const uint32_t* __restrict__ cell_of,
                    const uint32_t* __restrict__ start, const uint32_t* __restrict__ items,
                    const uint32_t* __restrict__ off, uint32_t entries, uint2* __restrict__ hdr,
                    uint32_t* __restrict__ occ_idx, double* __restrict__ keys,
                    float4* __restrict__ occ_sp) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t o = off[i];
    uint2 h = hdr[i];
    h.x = o;
    // (a list that would not fit the counted total cannot happen; it walks)
    if (h.y != kOccWalk && (h.y > entries || o > entries - h.y)) h.y = kOccWalk;
    hdr[i] = h;
    if (h.y == kOccWalk || h.y == 0u) return;
    const uint32_t m = h.y;
    uint32_t k = 0u;
    occ_candidates(i, geo, p, cell_of, start, items, [&](uint32_t j) {
        if (k < m) {
            const double* gj = geo + size_t(kGeo) * j;
            const double key = gj[2] - gj[5];
            // insertion into the sorted prefix [0, k)
            uint32_t q = k;
            while (q > 0u) {
                const double kq = keys[o + q - 1u];
                const uint32_t jq = occ_idx[o + q - 1u];
                if (kq < key || (kq == key && jq < j)) break;
                keys[o + q] = kq;
                occ_idx[o + q] = jq;
                --q;
            }
            keys[o + q] = key;
            occ_idx[o + q] = j;
            ++k;
        }
    });
    for (uint32_t q = 0; q < m; ++q) occ_sp[o + q] = spheres[occ_idx[o + q]];
}

// Per leaf reference the header of its sphere (gaps and the tail: no list).
__global__ void __launch_bounds__(kThreads)
    occ_refs_kernel(const uint32_t* __restrict__ prim_idx, uint32_t n_refs, uint32_t n_total,
                    const uint2* __restrict__ hdr, uint32_t n, uint2* __restrict__ out) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n_total) return;
    uint2 h = make_uint2(0u, 0u);
    if (i < n_refs) {
        const uint32_t k = prim_idx[i];
        if (k < n) h = hdr[k];
    }
    out[i] = h;
}

// ---- exclusive scan of uint32 in place (three launches) ---------------------
__global__ void __launch_bounds__(kThreads)
    scan_sums_kernel(const uint32_t* __restrict__ data, uint32_t n, uint32_t* __restrict__ part) {
    __shared__ uint32_t ws[kThreads / 64];
    const uint32_t base = blockIdx.x * kScanBlock + threadIdx.x * kScanItems;
    uint32_t s = 0u;
    for (uint32_t k = 0; k < kScanItems; ++k)
        if (base + k < n) s += data[base + k];
    for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d, 64);
    if ((threadIdx.x & 63u) == 0u) ws[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint32_t t = 0u;
        for (uint32_t w = 0; w < kThreads / 64; ++w) t += ws[w];
        part[blockIdx.x] = t;
    }
}
// one wave: part[0 .. nb) -> exclusive prefix, part[nb] = total
__global__ void __launch_bounds__(64) scan_parts_kernel(uint32_t* __restrict__ part, uint32_t nb) {
    uint32_t carry = 0u;
    const uint32_t lane = threadIdx.x;
    for (uint32_t b = 0; b < nb; b += 64u) {
        const uint32_t v = b + lane < nb ? part[b + lane] : 0u;
        uint32_t incl = v;
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t o = __shfl_up(incl, static_cast<unsigned>(d), 64);
            if (static_cast<int>(lane) >= d) incl += o;
        }
        if (b + lane < nb) part[b + lane] = carry + incl - v;
        carry += __shfl(incl, 63, 64);
    }
    if (lane == 0u) part[nb] = carry;
}
__global__ void __launch_bounds__(kThreads)
    scan_apply_kernel(uint32_t* __restrict__ data, uint32_t n, const uint32_t* __restrict__ part) {
    __shared__ uint32_t ws[kThreads / 64];
    const uint32_t base = blockIdx.x * kScanBlock + threadIdx.x * kScanItems;
    uint32_t v[kScanItems], s = 0u;
    for (uint32_t k = 0; k < kScanItems; ++k) {
        v[k] = base + k < n ? data[base + k] : 0u;
        s += v[k];
    }
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t incl = s;
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(incl, static_cast<unsigned>(d), 64);
        if (static_cast<int>(lane) >= d) incl += o;
    }
    if (lane == 63u) ws[wave] = incl;
    __syncthreads();
    uint32_t pre = part[blockIdx.x];
    for (uint32_t w = 0; w < wave; ++w) pre += ws[w];
    uint32_t run = pre + incl - s;
    for (uint32_t k = 0; k < kScanItems; ++k) {
        if (base + k < n) data[base + k] = run;
        run += v[k];
    }
}

inline uint32_t blocks_for(size_t n, uint32_t per) { return static_cast<uint32_t>((n + per - 1) / per); }

}  // namespace

template <typename T>
hipError_t OccluderLists::reserve(T*& p, size_t& cap, size_t n) {
    if (p && cap >= n) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    if (n == 0) n = 1;
    const hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), n * sizeof(T));
    if (e != hipSuccess) {
        p = nullptr;
        return e;
    }
    cap = n;
    return hipSuccess;
}

void OccluderLists::release() {
    void* all[] = {geo_, cell_of_, cells_, items_, len_, part_, hdr_, par_, occ_sp_, occ_idx_, keys_, prim_occ_};
    for (void* q : all)
        if (q) (void)hipFree(q);
    geo_ = nullptr, cell_of_ = nullptr, cells_ = nullptr, items_ = nullptr, len_ = nullptr;
    part_ = nullptr, hdr_ = nullptr, par_ = nullptr, occ_sp_ = nullptr, occ_idx_ = nullptr;
    keys_ = nullptr, prim_occ_ = nullptr;
    geo_cap_ = cell_of_cap_ = cells_cap_ = items_cap_ = len_cap_ = part_cap_ = hdr_cap_ = 0;
    occ_sp_cap_ = occ_idx_cap_ = keys_cap_ = prim_occ_cap_ = 0;
    on_ = false;
    n_ = 0;
}

// exclusive scan of data[0 .. n) in place; part_[blocks] = the total
hipError_t OccluderLists::scan(uint32_t* data, uint32_t n, hipStream_t st) {
    const uint32_t nb = blocks_for(n, kScanBlock);
    hipError_t e = reserve(part_, part_cap_, size_t(nb) + 1u);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(scan_sums_kernel, dim3(nb), dim3(kThreads), 0, st, data, n, part_);
    hipLaunchKernelGGL(scan_parts_kernel, dim3(1), dim3(64), 0, st, part_, nb);
    hipLaunchKernelGGL(scan_apply_kernel, dim3(nb), dim3(kThreads), 0, st, data, n, part_);
    return hipGetLastError();
}

hipError_t OccluderLists::count(const float4* spheres, uint32_t n, const float L[3], const float e[6],
                                double delta, double M, uint32_t cap, hipStream_t st) {
    on_ = false;
    tot_ = Totals{};
    spheres_ = spheres;
    n_ = n;
    cap_ = cap;
    if (n == 0) {
        tot_.skipped = 1u;
        return hipSuccess;
    }
    // about one cell a sphere, at most 2048 x 2048
    uint32_t g = static_cast<uint32_t>(sqrt(static_cast<double>(n)));
    gmax_ = g < 1u ? 1u : g > 2048u ? 2048u : g;
    const size_t nc = size_t(gmax_) * gmax_;
    hipError_t err;
    if (!par_) {
        OccPar* q = nullptr;
        if ((err = hipMalloc(reinterpret_cast<void**>(&q), sizeof(OccPar))) != hipSuccess) return err;
        par_ = q;
    }
    if ((err = reserve(geo_, geo_cap_, size_t(kGeo) * n)) != hipSuccess) return err;
    if ((err = reserve(cell_of_, cell_of_cap_, n)) != hipSuccess) return err;
    if ((err = reserve(cells_, cells_cap_, 2u * nc + 2u)) != hipSuccess) return err;
    if ((err = reserve(items_, items_cap_, n)) != hipSuccess) return err;
    if ((err = reserve(len_, len_cap_, n)) != hipSuccess) return err;
    if ((err = reserve(hdr_, hdr_cap_, n)) != hipSuccess) return err;
    OccPar* par = static_cast<OccPar*>(par_);
    uint32_t* start = cells_;             // nc + 1 words (start[nc] = n after the scan)
    uint32_t* cur = cells_ + nc + 1u;     // nc words
    const uint32_t nbs = blocks_for(n, kThreads);
    hipLaunchKernelGGL(occ_init_kernel, dim3(1), dim3(1), 0, st, par, delta, M, L[0], L[1], L[2], e[0],
                       e[1], e[2], e[3], e[4], e[5], gmax_, cap);
    if ((err = hipMemsetAsync(cells_, 0, (2u * nc + 2u) * sizeof(uint32_t), st)) != hipSuccess) return err;
    hipLaunchKernelGGL(occ_prep_kernel, dim3(nbs), dim3(kThreads), 0, st, spheres, n, par, geo_);
    hipLaunchKernelGGL(occ_grid_kernel, dim3(1), dim3(1), 0, st, par);
    hipLaunchKernelGGL(occ_cell_count_kernel, dim3(nbs), dim3(kThreads), 0, st, geo_, n, par, cell_of_, start);
    if ((err = scan(start, static_cast<uint32_t>(nc + 1u), st)) != hipSuccess) return err;
    hipLaunchKernelGGL(occ_cell_fill_kernel, dim3(nbs), dim3(kThreads), 0, st, cell_of_, n, par, start, cur,
                       items_);
    hipLaunchKernelGGL(occ_work_kernel, dim3(blocks_for(nc, kThreads)), dim3(kThreads), 0, st, start,
                       static_cast<uint32_t>(nc), par);
    hipLaunchKernelGGL(occ_decide_kernel, dim3(1), dim3(1), 0, st, par,
                       kOccWorkPerSphere * static_cast<unsigned long long>(n));
    hipLaunchKernelGGL(occ_pair_count_kernel, dim3(nbs), dim3(kThreads), 0, st, geo_, n, par, cell_of_,
                       start, items_, len_, hdr_);
    if ((err = scan(len_, n, st)) != hipSuccess) return err;
    hipLaunchKernelGGL(occ_total_kernel, dim3(1), dim3(1), 0, st, par, part_ + blocks_for(n, kScanBlock));
    if ((err = hipGetLastError()) != hipSuccess) return err;
    // the totals: read by the caller's wait
    return hipMemcpyAsync(&tot_, &par->tot, sizeof(tot_), hipMemcpyDeviceToHost, st);
}

hipError_t OccluderLists::fill(const uint32_t* prim_idx, uint32_t n_refs, double mean_max,
                               hipStream_t st) {
    on_ = false;
    if (n_ == 0 || tot_.skipped || tot_.n_bad) return hipSuccess;
    const double mean = static_cast<double>(tot_.cand) / n_;
    const unsigned long long bytes = static_cast<unsigned long long>(tot_.entries) * (16u + 4u + 8u) +
                                     (static_cast<unsigned long long>(n_refs) + kPrimPad) * 8u;
    if (mean > mean_max || bytes > kOccMaxBytes) return hipSuccess;
    hipError_t err;
    const uint32_t m = tot_.entries;
    if ((err = reserve(occ_sp_, occ_sp_cap_, size_t(m) + 1u)) != hipSuccess) return err;
    if ((err = reserve(occ_idx_, occ_idx_cap_, size_t(m) + 1u)) != hipSuccess) return err;
    if ((err = reserve(keys_, keys_cap_, size_t(m) + 1u)) != hipSuccess) return err;
    if ((err = reserve(prim_occ_, prim_occ_cap_, size_t(n_refs) + kPrimPad)) != hipSuccess) return err;
    OccPar* par = static_cast<OccPar*>(par_);
    hipLaunchKernelGGL(occ_fill_kernel, dim3(blocks_for(n_, kThreads)), dim3(kThreads), 0, st, spheres_,
                       geo_, n_, par, cell_of_, cells_, items_, len_, m, hdr_, occ_idx_, keys_, occ_sp_);
    hipLaunchKernelGGL(occ_refs_kernel, dim3(blocks_for(size_t(n_refs) + kPrimPad, kThreads)),
                       dim3(kThreads), 0, st, prim_idx, n_refs, n_refs + kPrimPad, hdr_, n_, prim_occ_);
    if ((err = hipGetLastError()) != hipSuccess) return err;
    on_ = true;
    return hipSuccess;
}

}  // namespace rtamd
