// rt_scene.cpp — the scene of a renderer: upload, the octree build
// (build_scene and its steps) and the exports.
#include <stdexcept>

#include "rt_host.h"

using namespace rtamd;

namespace {

// Leaf records of a breadth-first tree: a record's kind is in
// its parent's leaf mask, and children come after their parent, so one
// forward pass over the records finds them all.  Returned in record order.
std::vector<uint32_t> leaf_records(const std::vector<uint2>& nodes) {
    std::vector<uint8_t> internal(nodes.size(), 0);
    std::vector<uint32_t> leaves;
    if (!nodes.empty()) internal[0] = 1;  // (callers skip a root leaf)
    for (size_t i = 0; i < nodes.size(); ++i) {
        if (!internal[i]) continue;
        const uint32_t valid = nodes[i].y & 0xFFu, leafm = (nodes[i].y >> 8) & 0xFFu;
        uint32_t k = nodes[i].x;
        for (uint32_t c = 0; c < 8; ++c) {
            if (!((valid >> c) & 1u)) continue;
            if ((leafm >> c) & 1u) leaves.push_back(k);
            else internal[k] = 1;
            ++k;
        }
    }
    std::sort(leaves.begin(), leaves.end(), [&](uint32_t a, uint32_t b) { return nodes[a].x < nodes[b].x; });
    return leaves;
}

// Line-packed leaf lists: the builders store the leaf
// lists back to back, so a leaf of n spheres (16 B each) straddles a 128-byte
// cache line whenever it does not fit in the rest of one: 1.44-1.57 lines per
// leaf on C3 / C5 / C5d against 1.05-1.12 when no leaf that fits a line
// crosses one.  This relays the lists out so that it never does: a leaf whose
// footprint (n, plus the slot past its end that a two-sphere chunk reads when
// n is odd) fits in 8 slots starts in the current line if it fits there, else
// at the next line; a longer leaf starts at a line.  The gaps hold what the
// kPrimPad tail holds (zero spheres, or the test-only pad-fill spheres);
// leaf records point at the new offsets; images and counters are unchanged
// (the layout is not part of the spec).  The arrays grow by ~1.28x.
int pack_leaf_lines(rt_renderer* r, SceneArgs& sc, rt_scene_info& in, const float4& pad) {
    const size_t nn = in.n_nodes, np = in.n_prim_refs;
    std::vector<uint2> nodes(nn);
    RT_HIP(r, hipMemcpy(nodes.data(), sc.nodes, nn * sizeof(uint2), hipMemcpyDeviceToHost));
    const std::vector<uint32_t> leaves = leaf_records(nodes);
    std::vector<uint32_t> nf(leaves.size());
    uint64_t off = 0;
    for (size_t i = 0; i < leaves.size(); ++i) {
        const uint32_t n = nodes[leaves[i]].y, f = n + (n & 1u), w = static_cast<uint32_t>(off & 7u);
        if (w && (f > 8u || w + f > 8u)) off += 8u - w;
        nf[i] = static_cast<uint32_t>(off);
        off += n;
    }
    if (off + kPrimPad >= (uint64_t(1) << 32)) return RT_OK;  // (keep the compact layout)
    const uint32_t slots = static_cast<uint32_t>(off);
    std::vector<float4> sp(np), spn(slots, pad);
    std::vector<uint32_t> ix(np), ixn(slots, 0u);
    if (np) {
        RT_HIP(r, hipMemcpy(sp.data(), sc.prim_sp, np * sizeof(float4), hipMemcpyDeviceToHost));
        RT_HIP(r, hipMemcpy(ix.data(), sc.prim_idx, np * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    for (size_t i = 0; i < leaves.size(); ++i) {
        uint2& rec = nodes[leaves[i]];
        std::copy(sp.begin() + rec.x, sp.begin() + rec.x + rec.y, spn.begin() + nf[i]);
        std::copy(ix.begin() + rec.x, ix.begin() + rec.x + rec.y, ixn.begin() + nf[i]);
        rec.x = nf[i];
    }
    int st;
    if ((st = ensure(r, r->d_prim_sp, (size_t)slots + kPrimPad))) return st;
    if ((st = ensure(r, r->d_prim_idx, slots))) return st;
    if (slots) {
        RT_HIP(r, hipMemcpy(r->d_prim_sp.p, spn.data(), slots * sizeof(float4), hipMemcpyHostToDevice));
        RT_HIP(r, hipMemcpy(r->d_prim_idx.p, ixn.data(), slots * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    RT_HIP(r, hipMemcpy(const_cast<uint2*>(sc.nodes), nodes.data(), nn * sizeof(uint2),
                        hipMemcpyHostToDevice));
    sc.prim_sp = r->d_prim_sp.p;
    sc.prim_idx = r->d_prim_idx.p;
    r->prim_slots = slots;
    r->leaf_packed = true;
    return RT_OK;
}

// build_scene's steps.  They share r->sc and r->info: the depth limit in
// force is info.max_depth, the root box the builder used info.root_min / max.

// The device builder's tree (the default).  *err is the build's own status:
// anything but hipSuccess leaves no tree, and host_tree decides what follows.
int device_tree(rt_renderer* r, uint32_t cap, hipError_t* err) {
    const rt_octree_params& p = r->oct;
    SceneArgs& sc = r->sc;
    rt_scene_info& in = r->info;
    GpuBuildResult res;
    hipError_t e = r->gpu_build.build(r->d_spheres.p, r->n_spheres, p.min, p.max, in.max_depth, cap,
                                      r->stream, &res);
    if (res.n_invalid)
        return fail(r, RT_E_INVALID, "scene has spheres with radius <= 0 or non-finite values");
    // (test only: kOptDeviceBuildRefuse makes the device build report
    // running out of HBM, the one case that falls back to the host)
    if ((r->cfg.flags >> RT_FLAG_OPT_SHIFT) & kOptDeviceBuildRefuse) e = hipErrorOutOfMemory;
    if (res.ref_overflow) {
        // The device builder's 32-bit per-level slots overflowed: that
        // level holds >= 2^29 references (octree_build.hip), which the
        // host builder would need >= 2^29 x ~64 B = 32 GiB for (index,
        // sphere record, per-level lists) and would grind through for
        // minutes.  Always refused, at once; the
        // host fallback covers only the device build running out of HBM.
        (void)hipGetLastError();
        return fail(r, RT_E_NOMEM,
                    "scene too large for the octree: the device builder overflowed at " +
                        std::to_string(res.ref_overflow) +
                        " references (a host build would need about " +
                        std::to_string((res.ref_overflow * 64ull) >> 30) +
                        " GiB); lower max_depth or raise leaf_capacity");
    }
    *err = e;
    if (e != hipSuccess) return RT_OK;
    sc.nodes = r->gpu_build.nodes();
    sc.prim_sp = r->gpu_build.prim_sp();
    sc.prim_idx = r->gpu_build.prim_idx();
    sc.root = res.root;
    sc.root_is_leaf = res.root_is_leaf ? 1u : 0u;
    in.n_nodes = res.n_nodes;
    in.n_leaves = res.n_leaves;
    in.n_prim_refs = res.n_prims;
    in.depth_reached = res.depth_reached;
    in.builder = RT_BUILDER_DEVICE;
    memcpy(in.root_min, res.rmin, sizeof(in.root_min));
    memcpy(in.root_max, res.rmax, sizeof(in.root_max));
    return RT_OK;
}

// The host builder's tree, uploaded: when it was asked for
// (RT_FLAG_HOST_BUILD), or when the device build (status `dev`) ran out of
// HBM; any other device failure is the call's.
int host_tree(rt_renderer* r, uint32_t cap, bool asked, hipError_t dev) {
    if (!asked) {
        if (dev == hipSuccess) return RT_OK;  // the device tree stands
        if (dev != hipErrorOutOfMemory) return hip_fail(r, dev, "device octree build");
        // HBM cannot hold the device build's working set: build the
        // identical tree on the host instead (rt_scene_info.builder then
        // reports RT_BUILDER_HOST); build_octree refuses past 2^31
        // references and reports host allocation failure as RT_E_NOMEM
        (void)hipGetLastError();
    }
    const rt_octree_params& p = r->oct;
    const uint32_t n = r->n_spheres;
    if (!r->host_copy) {
        r->spheres.resize(4u * n);
        if (n)
            RT_HIP(r, hipMemcpy(r->spheres.data(), r->d_spheres.p, n * sizeof(float4),
                                hipMemcpyDeviceToHost));
        r->host_copy = true;
    }
    BuiltOctree tree;
    try {
        build_octree(r->spheres.data(), n, p.min, p.max, r->info.max_depth, cap, tree);
    } catch (const std::length_error& ex) {  // past the 32-bit record fields
        return fail(r, RT_E_INVALID, std::string("scene too large for the octree: ") + ex.what() +
                                         "; lower max_depth or raise leaf_capacity");
    } catch (const std::exception& ex) {  // bad_alloc: never through the C-ABI
        return fail(r, RT_E_NOMEM, std::string("host octree build: ") + ex.what());
    }
    const size_t nn = tree.nodes.size(), np = tree.prim_idx.size();
    int st;
    if ((st = ensure(r, r->d_nodes, nn))) return st;
    if ((st = ensure(r, r->d_prim_sp, np + kPrimPad))) return st;  // scalar-read padding
    if ((st = ensure(r, r->d_prim_idx, np))) return st;
    RT_HIP(r, hipMemcpy(r->d_nodes.p, tree.nodes.data(), nn * sizeof(uint2), hipMemcpyHostToDevice));
    if (np) {
        RT_HIP(r, hipMemcpy(r->d_prim_sp.p, tree.prim_sp.data(), np * sizeof(float4),
                            hipMemcpyHostToDevice));
        RT_HIP(r, hipMemcpy(r->d_prim_idx.p, tree.prim_idx.data(), np * sizeof(uint32_t),
                            hipMemcpyHostToDevice));
    }
    SceneArgs& sc = r->sc;
    rt_scene_info& in = r->info;
    sc.nodes = r->d_nodes.p;
    sc.prim_sp = r->d_prim_sp.p;
    sc.prim_idx = r->d_prim_idx.p;
    sc.root = make_uint2(tree.nodes[0].x, tree.nodes[0].y);
    sc.root_is_leaf = tree.root_is_leaf ? 1u : 0u;
    in.n_nodes = static_cast<uint32_t>(nn);
    in.n_leaves = tree.n_leaves;
    in.n_prim_refs = static_cast<uint32_t>(np);
    in.depth_reached = tree.depth_reached;
    in.builder = RT_BUILDER_HOST;
    memcpy(in.root_min, tree.rmin, sizeof(in.root_min));
    memcpy(in.root_max, tree.rmax, sizeof(in.root_max));
    return RT_OK;
}

// The kPrimPad tail after the last leaf list is read by the leaf loads (a
// chunk's slot past the end of the LAST leaf) and joins the leaf screen
// unmasked; its tests are skipped, so only time could depend on it.  Neither
// builder writes it: fill it here so that nothing a frame does depends on
// what the allocation held before.  Zero spheres (r = 0) by default; the
// test-only fill modes put spheres there that pass the screen (NaN, or one
// covering the root box) to prove the images and counters do not depend on
// the tail.  The line-packed layout's gaps hold the same (RT_LEAF_PACK=1, a
// test hook; off by default: measured no faster).
int pad_and_pack(rt_renderer* r) {
    SceneArgs& sc = r->sc;
    const float *rmin = r->info.root_min, *rmax = r->info.root_max;
    const uint32_t mode = (r->cfg.flags >> RT_FLAG_PAD_FILL_SHIFT) & 3u;
    float4 p1 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (mode == 1) {
        p1 = make_float4(NAN, NAN, NAN, NAN);
    } else if (mode == 2) {
        const float c = 0.5f * (rmin[0] + rmax[0]);
        p1 = make_float4(c, 0.5f * (rmin[1] + rmax[1]), 0.5f * (rmin[2] + rmax[2]),
                         4.0f * (rmax[0] - rmin[0] + rmax[1] - rmin[1] + rmax[2] - rmin[2]));
    }
    float4 pad[kPrimPad];
    for (uint32_t i = 0; i < kPrimPad; ++i) pad[i] = p1;
    r->prim_slots = r->info.n_prim_refs;
    r->leaf_packed = false;
    int st;
    if (!sc.root_is_leaf && r->leaf_pack && (st = pack_leaf_lines(r, sc, r->info, p1))) return st;
    float4* tail = const_cast<float4*>(sc.prim_sp) + r->prim_slots;
    RT_HIP(r, hipMemcpyAsync(tail, pad, sizeof(pad), hipMemcpyHostToDevice, r->stream));
    RT_HIP(r, hipStreamSynchronize(r->stream));
    return RT_OK;
}

// depth-K cell table over the tree (flags bits 28..31: 0 auto, 15 off, else K)
int cell_table_over_tree(rt_renderer* r) {
    SceneArgs& sc = r->sc;
    const uint32_t f = (r->cfg.flags >> RT_FLAG_CELL_TABLE_SHIFT) & 0xFu;
    const uint32_t k_req = f == 0 ? kCellTableAuto : f == 15 ? kCellTableOff : f;
    hipError_t e = r->cell_table.build(sc.nodes, sc.root, sc.root_is_leaf != 0, r->info.max_depth,
                                       r->info.depth_reached, k_req, r->stream);
    if (e != hipSuccess) return hip_fail(r, e, "cell table build");
    sc.tab = r->cell_table.table();
    sc.tab_k = r->cell_table.k();
    r->info.cell_table_depth = sc.tab_k;
    return RT_OK;
}

// the rest of the kernels' scene arguments and of rt_scene_info; the scene is current from here
void finish_scene(rt_renderer* r, double build_ms) {
    SceneArgs& sc = r->sc;
    rt_scene_info& in = r->info;
    const uint32_t depth = in.max_depth;
    sc.spheres = r->d_spheres.p;
    sc.albedo = r->d_albedo.p;
    sc.max_depth = depth;
    sc.stack_depth = std::max(1u, std::min(depth, in.depth_reached));
    // LDS leaf staging on every scene; RT_LDS_STAGE=0, a test
    // hook, turns it off (the on/off parity test)
    sc.lds_max = r->lds_stage ? kLeafBuf : 0u;
    sc.G = static_cast<float>(1u << depth);
    for (int i = 0; i < 3; ++i) {
        sc.rmin[i] = in.root_min[i];
        sc.scale[i] = sc.G / (in.root_max[i] - in.root_min[i]);
    }
    in.n_spheres = r->n_spheres;
    in.node_bytes = sizeof(uint2);
    in.prim_bytes = sizeof(float4) + sizeof(uint32_t);
    in.build_ms = build_ms;
    ++r->scene_gen;  // the derived records (DerivedRecords) are remade at the next frame
    r->occ.off();    // and the occluder lists with the light-plane records
    r->occ_timed = false;
    r->has_scene = true;
}

int check_octree_params(rt_renderer* r, const rt_octree_params* oct, const char* who) {
    if (!oct) return RT_OK;
    for (int i = 0; i < 3; ++i)
        if (!(oct->max[i] > oct->min[i]))
            return fail(r, RT_E_INVALID, std::string(who) + ": empty octree root box");
    if (oct->max_depth > kMaxDepth) return fail(r, RT_E_INVALID, std::string(who) + ": max_depth > 16");
    if (oct->max_depth == 0 && !(oct->resolution > 0.0f))
        return fail(r, RT_E_INVALID, std::string(who) + ": need max_depth or resolution > 0");
    return RT_OK;
}

}  // namespace

// Build the octree of the device sphere list (d_spheres) and point the
// kernel's scene arguments at it.  The device builder is the default; the
// host builder (RT_FLAG_HOST_BUILD) yields the identical tree.
int rtamd::build_scene(rt_renderer* r) {
    const rt_octree_params& p = r->oct;
    const uint32_t depth = p.max_depth ? p.max_depth : depth_for_resolution(p.min, p.max, p.resolution);
    const uint32_t cap = p.leaf_capacity ? p.leaf_capacity : 8;
    int st;
    if ((st = set_device(r))) return st;
    // buffers of the previous tree may still be read by frames in flight on
    // any stream: the rebuild waits for the device
    RT_HIP(r, hipDeviceSynchronize());
    r->has_scene = false;
    r->frames_accum = 0;
    const double upload_ms = r->info.upload_ms;
    r->info = rt_scene_info();
    r->info.upload_ms = upload_ms;
    r->info.max_depth = std::min(depth, kMaxDepth);
    const auto t0 = std::chrono::steady_clock::now();
    const bool host = (r->cfg.flags & RT_FLAG_HOST_BUILD) != 0;
    hipError_t dev = hipSuccess;
    if (!host && (st = device_tree(r, cap, &dev))) return st;
    if ((st = host_tree(r, cap, host, dev))) return st;
    if ((st = pad_and_pack(r))) return st;
    if ((st = cell_table_over_tree(r))) return st;
    const auto t1 = std::chrono::steady_clock::now();
    finish_scene(r, std::chrono::duration<double, std::milli>(t1 - t0).count());
    return RT_OK;
}

extern "C" {

int rt_set_scene(rt_renderer* r, const float* spheres, const uint32_t* albedo, uint32_t n,
                 const rt_octree_params* oct) {
    if (!r) return fail(r, RT_E_INVALID, "rt_set_scene: null handle");
    if (n && !spheres) return fail(r, RT_E_INVALID, "rt_set_scene: null spheres");
    int st;
    if ((st = check_octree_params(r, oct, "rt_set_scene"))) return st;
    for (uint32_t i = 0; i < n; ++i) {
        const float* s = spheres + 4u * i;
        if (!(s[3] > 0.0f) || !isfinite(s[0]) || !isfinite(s[1]) || !isfinite(s[2]) ||
            !isfinite(s[3]))
            return fail(r, RT_E_INVALID,
                        "rt_set_scene: sphere with radius <= 0 or non-finite values");
    }
    if (oct) r->oct = *oct;
    if ((st = set_device(r))) return st;
    RT_HIP(r, hipDeviceSynchronize());
    auto t0 = std::chrono::steady_clock::now();
    r->spheres.assign(spheres, spheres + 4u * n);
    r->host_copy = true;
    r->n_spheres = n;
    std::vector<uint32_t> alb(n);
    for (uint32_t i = 0; i < n; ++i) alb[i] = albedo ? albedo[i] : 0xFFCCCCCCu;
    if ((st = ensure(r, r->d_spheres, n))) return st;
    if ((st = ensure(r, r->d_albedo, n))) return st;
    if (n) {
        RT_HIP(r, hipMemcpy(r->d_spheres.p, spheres, n * sizeof(float4), hipMemcpyHostToDevice));
        RT_HIP(r, hipMemcpy(r->d_albedo.p, alb.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    r->info.upload_ms =
        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if ((st = build_scene(r))) return st;
    return for_peers(r, [&](rt_renderer* p) { return rt_set_scene(p, spheres, albedo, n, oct); });
}

int rt_set_scene_device(rt_renderer* r, const void* dev_spheres, const void* dev_albedo,
                        uint32_t n, const rt_octree_params* oct, void* stream) {
    if (!r) return fail(r, RT_E_INVALID, "rt_set_scene_device: null handle");
    if (n && !dev_spheres) return fail(r, RT_E_INVALID, "rt_set_scene_device: null spheres");
    int st;
    if ((st = check_octree_params(r, oct, "rt_set_scene_device"))) return st;
    if ((st = set_device(r))) return st;
    if (stream) RT_HIP(r, hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    const float4* src = static_cast<const float4*>(dev_spheres);
    if (n) {
        SphereBounds sb;
        hipError_t e = r->gpu_build.bounds(src, n, r->stream, &sb);
        if (e != hipSuccess) return hip_fail(r, e, "rt_set_scene_device: validation");
        if (sb.n_invalid)
            return fail(r, RT_E_INVALID,
                        "rt_set_scene_device: sphere with radius <= 0 or non-finite values");
    }
    if (oct) r->oct = *oct;
    RT_HIP(r, hipDeviceSynchronize());
    auto t0 = std::chrono::steady_clock::now();
    if ((st = ensure(r, r->d_spheres, n))) return st;
    if ((st = ensure(r, r->d_albedo, n))) return st;
    if (n) {
        RT_HIP(r, hipMemcpyAsync(r->d_spheres.p, src, n * sizeof(float4), hipMemcpyDeviceToDevice,
                                 r->stream));
        if (dev_albedo)
            RT_HIP(r, hipMemcpyAsync(r->d_albedo.p, dev_albedo, n * sizeof(uint32_t),
                                     hipMemcpyDeviceToDevice, r->stream));
        else
            RT_HIP(r, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(r->d_albedo.p),
                                        0xFFCCCCCCu, n, r->stream));
        RT_HIP(r, hipStreamSynchronize(r->stream));
    }
    r->n_spheres = n;
    r->spheres.clear();
    r->host_copy = false;
    r->info.upload_ms =
        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if ((st = build_scene(r))) return st;
    // a multi-device handle: the validated list (now in d_spheres / d_albedo
    // on devices[0]) is broadcast to the other devices, which build their trees
    return r->multi ? multi_set_scene_device(r, n, oct) : RT_OK;
}

int rt_set_octree(rt_renderer* r, const float mn[3], const float mx[3], float resolution) {
    if (!r || !mn || !mx) return fail(r, RT_E_INVALID, "rt_set_octree: null argument");
    rt_octree_params p = r->oct;
    for (int i = 0; i < 3; ++i) {
        p.min[i] = mn[i];
        p.max[i] = mx[i];
        if (!(mx[i] > mn[i])) return fail(r, RT_E_INVALID, "rt_set_octree: empty box");
    }
    if (!(resolution > 0.0f)) return fail(r, RT_E_INVALID, "rt_set_octree: resolution <= 0");
    p.resolution = resolution;
    p.max_depth = 0;
    r->oct = p;
    int st;
    if (r->has_scene && (st = build_scene(r))) return st;
    return for_peers(r, [&](rt_renderer* q) { return rt_set_octree(q, mn, mx, resolution); });
}

int rt_get_scene_info(const rt_renderer* r, rt_scene_info* info) {
    if (!r || !info) return RT_E_INVALID;
    if (!r->has_scene) return RT_E_NOSCENE;
    *info = r->info;
    return RT_OK;
}

int rt_export_occluders(rt_renderer* r, uint32_t* offsets_out, uint32_t* counts_out,
                        uint32_t* indices_out, uint32_t* prim_occ_out) {
    if (!r) return fail(r, RT_E_INVALID, "rt_export_occluders: null handle");
    if (!r->has_scene) return fail(r, RT_E_NOSCENE, "rt_export_occluders: no scene");
    if (!r->occluders_current())
        return fail(r, RT_E_STATE, "rt_export_occluders: the scene has no occluder lists "
                                   "(they are made by the first frame after a scene change)");
    if (prim_occ_out && r->leaf_packed)
        return fail(r, RT_E_STATE, "rt_export_occluders: no per-reference export of a line-packed layout");
    int st;
    if ((st = set_device(r))) return st;
    RT_HIP(r, hipDeviceSynchronize());
    const uint32_t n = r->occ.n(), m = r->occ.totals().entries;
    std::vector<uint2> hdr(n);
    if (n) RT_HIP(r, hipMemcpy(hdr.data(), r->occ.headers(), n * sizeof(uint2), hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < n; ++i) {
        if (offsets_out) offsets_out[i] = hdr[i].x;
        if (counts_out) counts_out[i] = hdr[i].y;
    }
    if (indices_out && m)
        RT_HIP(r, hipMemcpy(indices_out, r->occ.occ_idx(), m * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (prim_occ_out && r->info.n_prim_refs)
        RT_HIP(r, hipMemcpy(prim_occ_out, r->occ.prim_occ(), r->info.n_prim_refs * sizeof(uint2),
                            hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_export_octree(rt_renderer* r, uint32_t* nodes_out, float* prim_sp_out,
                     uint32_t* prim_idx_out) {
    if (!r) return fail(r, RT_E_INVALID, "rt_export_octree: null handle");
    if (!r->has_scene) return fail(r, RT_E_NOSCENE, "rt_export_octree: no scene");
    int st;
    if ((st = set_device(r))) return st;
    RT_HIP(r, hipDeviceSynchronize());
    const size_t nn = r->info.n_nodes, np = r->info.n_prim_refs;
    if (r->leaf_packed) {
        // the builders' record-for-record tree: the line-packed lists
        // (pack_leaf_lines) put back to back again, in the same order
        std::vector<uint2> nodes(nn);
        RT_HIP(r, hipMemcpy(nodes.data(), r->sc.nodes, nn * sizeof(uint2), hipMemcpyDeviceToHost));
        std::vector<float4> sp(r->prim_slots);
        std::vector<uint32_t> ix(r->prim_slots);
        if (r->prim_slots) {
            RT_HIP(r, hipMemcpy(sp.data(), r->sc.prim_sp, sp.size() * sizeof(float4), hipMemcpyDeviceToHost));
            RT_HIP(r, hipMemcpy(ix.data(), r->sc.prim_idx, ix.size() * sizeof(uint32_t),
                                hipMemcpyDeviceToHost));
        }
        uint32_t off = 0;
        for (uint32_t i : leaf_records(nodes)) {
            uint2& rec = nodes[i];
            if (prim_sp_out)
                memcpy(prim_sp_out + 4u * size_t(off), sp.data() + rec.x, rec.y * sizeof(float4));
            if (prim_idx_out) memcpy(prim_idx_out + off, ix.data() + rec.x, rec.y * sizeof(uint32_t));
            rec.x = off;
            off += rec.y;
        }
        if (nodes_out) memcpy(nodes_out, nodes.data(), nn * sizeof(uint2));
        return RT_OK;
    }
    if (nodes_out)
        RT_HIP(r, hipMemcpy(nodes_out, r->sc.nodes, nn * sizeof(uint2), hipMemcpyDeviceToHost));
    if (prim_sp_out && np)
        RT_HIP(r, hipMemcpy(prim_sp_out, r->sc.prim_sp, np * sizeof(float4), hipMemcpyDeviceToHost));
    if (prim_idx_out && np)
        RT_HIP(r, hipMemcpy(prim_idx_out, r->sc.prim_idx, np * sizeof(uint32_t),
                            hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_save_spheres(const char* path, const float* spheres, const uint32_t* albedo, uint32_t n) {
    if (!path || (n && !spheres)) return fail(nullptr, RT_E_INVALID, "rt_save_spheres: null argument");
    std::string err;
    if (!save_sphere_file(path, spheres, albedo, n, &err)) return fail(nullptr, RT_E_INVALID, err);
    return RT_OK;
}

int rt_load_spheres(const char* path, float* spheres_out, uint32_t* albedo_out, uint32_t capacity,
                    uint32_t* n_out) {
    if (!path || !n_out) return fail(nullptr, RT_E_INVALID, "rt_load_spheres: null argument");
    std::string err;
    if (!load_sphere_file(path, spheres_out, albedo_out, capacity, n_out, &err))
        return fail(nullptr, RT_E_INVALID, err);
    return RT_OK;
}

int rt_generate_spheres(uint32_t n, uint32_t seed, float* spheres_out, uint32_t* albedo_out) {
    if (n && !spheres_out) return fail(nullptr, RT_E_INVALID, "rt_generate_spheres: null output");
    generate_spheres(n, seed, spheres_out, albedo_out);
    return RT_OK;
}

}  // extern "C"
