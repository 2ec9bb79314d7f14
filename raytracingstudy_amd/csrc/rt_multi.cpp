// rt_multi.cpp — the multi-device handle (rt_create_multi; SURVEY 8b B2 "device ids", 8e E1)
//
// One process drives n devices.  Frame j uses slot f = j mod 2:
//   device k, its renderer's stream : [wait sent[f][k]]  render its tiles -> slab[f][k]
//                                      record rendered[f][k]
//   device k, comm stream cs[k]     : wait rendered[f][k]; send slab[f][k] to device 0
//                                      record sent[f][k]
//   device 0, comm stream cs[0]     : [wait unpacked[f]]; receive slab k into
//                                      recv[f] + k * slab; record recvd[f]
//   device 0, output stream hs      : record out_ready; cs[0] waits it and recvd[f], unpacks
//                                      the n slabs in ONE launch into the frame; hs waits
//                                      unpacked[f]
// so frame j+1's tiles render while frame j's slabs travel and unpack, and a
// slab or receive buffer is rewritten only after its previous frame let go of
// it.  Transport: RCCL (grouped ncclSend / ncclRecv over one ncclCommInitAll
// communicator, device 0 receiving from itself too) or peer copies
// (hipMemcpyPeerAsync: distinct devices over xGMI, or the same device in a
// rehearsal of the n-way plan on one GPU).
#include <dlfcn.h>
#include <rccl/rccl.h>  // types only: the functions are resolved at run time (rccl_api)

#include <mutex>

#include "rt_host.h"

using namespace rtamd;

namespace {

// RCCL resolved at run time: librt_amd.so does not link it, so a process that
// already holds one (torch's) shares it, and single-device use never loads it.
struct RcclApi {
    bool ok = false;
    std::string why;
    ncclResult_t (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Broadcast)(const void*, void*, size_t, ncclDataType_t, int, ncclComm_t,
                              hipStream_t) = nullptr;
    const char* (*ErrorString)(ncclResult_t) = nullptr;
};

RcclApi& rccl_api() {
    static RcclApi api;
    static std::once_flag once;
    std::call_once(once, [] {
        void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
        if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_LOCAL);
        if (!h) {
            api.why = std::string("librccl.so.1 not loadable: ") + dlerror();
            return;
        }
        bool all = true;
        auto sym = [&](const char* n) {
            void* p = dlsym(h, n);
            if (!p) all = false;
            return p;
        };
        api.CommInitAll = reinterpret_cast<decltype(api.CommInitAll)>(sym("ncclCommInitAll"));
        api.CommDestroy = reinterpret_cast<decltype(api.CommDestroy)>(sym("ncclCommDestroy"));
        api.GroupStart = reinterpret_cast<decltype(api.GroupStart)>(sym("ncclGroupStart"));
        api.GroupEnd = reinterpret_cast<decltype(api.GroupEnd)>(sym("ncclGroupEnd"));
        api.Send = reinterpret_cast<decltype(api.Send)>(sym("ncclSend"));
        api.Recv = reinterpret_cast<decltype(api.Recv)>(sym("ncclRecv"));
        api.Broadcast = reinterpret_cast<decltype(api.Broadcast)>(sym("ncclBroadcast"));
        api.ErrorString = reinterpret_cast<decltype(api.ErrorString)>(sym("ncclGetErrorString"));
        api.ok = all;
        if (!all) api.why = "librccl.so.1 lacks a required symbol";
    });
    return api;
}

int nccl_fail(rt_renderer* r, ncclResult_t e, const char* what) {
    const char* m = rccl_api().ErrorString ? rccl_api().ErrorString(e) : "?";
    return fail(r, RT_E_HIP, std::string(what) + ": RCCL error " + std::to_string((int)e) + " (" + m + ")");
}

#define RT_NCCL(r, call)                                         \
    do {                                                         \
        ncclResult_t e_ = (call);                                \
        if (e_ != ncclSuccess) return nccl_fail((r), e_, #call); \
    } while (0)

// (Re)plan the tiles and the buffers for the handle's current size: tile t to
// device t mod n (interleaved, so a centred scene balances), slabs
// of S = ceil(T / n) tiles, the gathered slabs unpacked with padding slots
// skipped.  Waits for in-flight frames before it frees anything.
int multi_plan(rt_renderer* r) {
    MultiState& m = *r->multi;
    if (m.W == r->W && m.H == r->H && m.recv[0]) return RT_OK;
    int st;
    if ((st = multi_wait(r))) return st;
    const uint32_t n = static_cast<uint32_t>(m.devs.size()), ts = MultiState::kTs;
    const uint32_t T = ((r->W + ts - 1) / ts) * ((r->H + ts - 1) / ts);
    m.S = (T + n - 1) / n;
    m.slab_bytes = (size_t)m.S * ts * ts * 4;
    m.ids.assign(n, {});
    for (uint32_t t = 0; t < T; ++t) m.ids[t % n].push_back(t);
    m.all_ids.assign((size_t)n * m.S, RT_TILE_SKIP);
    for (uint32_t k = 0; k < n; ++k)
        std::copy(m.ids[k].begin(), m.ids[k].end(), m.all_ids.begin() + (size_t)k * m.S);
    for (int f = 0; f < MultiState::F; ++f) {
        for (uint32_t k = 0; k < n; ++k) {
            RT_HIP(r, hipSetDevice(m.devs[k]));
            if (m.slab[f][k]) (void)hipFree(m.slab[f][k]);
            m.slab[f][k] = nullptr;
            hipError_t e = m.fault == MultiState::kSlab && k == m.fault_k
                               ? hipErrorOutOfMemory  // RT_TEST_FAULT=slab:k
                               : hipMalloc(&m.slab[f][k], m.slab_bytes);
            if (e != hipSuccess) {
                m.slab[f][k] = nullptr;
                return hip_fail(r, e, ("tile slab allocation" + peer_name(m, k)).c_str());
            }
        }
        RT_HIP(r, hipSetDevice(m.devs[0]));
        if (m.recv[f]) (void)hipFree(m.recv[f]);
        m.recv[f] = nullptr;
        RT_HIP(r, hipMalloc(&m.recv[f], m.slab_bytes * n));
        m.used[f] = false;
    }
    RT_HIP(r, hipSetDevice(m.devs[0]));
    if (m.d_all_ids) (void)hipFree(m.d_all_ids);
    m.d_all_ids = nullptr;
    RT_HIP(r, hipMalloc(reinterpret_cast<void**>(&m.d_all_ids), m.all_ids.size() * sizeof(uint32_t)));
    RT_HIP(r, hipMemcpy(m.d_all_ids, m.all_ids.data(), m.all_ids.size() * sizeof(uint32_t),
                        hipMemcpyHostToDevice));
    m.W = r->W;
    m.H = r->H;
    return RT_OK;
}

// ---- rt_create_multi's steps ----

// The arguments, and the transport RT_TRANSPORT_AUTO stands for.
int check_create_multi(const rt_config* cfg, const int32_t* devices, uint32_t n_devices, uint32_t* transport) {
    if (n_devices == 0 || n_devices > RT_MAX_DEVICES)
        return fail(nullptr, RT_E_INVALID, "rt_create_multi: n_devices must be 1..16");
    if (*transport > RT_TRANSPORT_PEER) return fail(nullptr, RT_E_INVALID, "rt_create_multi: unknown transport");
    const int ndev = rt_device_count();
    bool distinct = true;
    for (uint32_t i = 0; i < n_devices; ++i) {
        if (devices[i] < 0 || devices[i] >= ndev)
            return fail(nullptr, RT_E_INVALID, "rt_create_multi: device ordinal out of range");
        for (uint32_t j = 0; j < i; ++j)
            if (devices[j] == devices[i]) distinct = false;
    }
    if (*transport == RT_TRANSPORT_RCCL && !distinct)
        return fail(nullptr, RT_E_INVALID,
                    "rt_create_multi: RCCL needs distinct devices (a repeated ordinal is a "
                    "peer-copy rehearsal)");
    if (*transport == RT_TRANSPORT_AUTO) *transport = distinct && rccl_api().ok ? RT_TRANSPORT_RCCL : RT_TRANSPORT_PEER;
    if (*transport == RT_TRANSPORT_RCCL && !rccl_api().ok)
        return fail(nullptr, RT_E_INVALID, "rt_create_multi: " + rccl_api().why);
    // the handle renders through packed tile slabs, which carry RGBA8 only
    if (cfg->flags & RT_FLAG_RADIANCE)
        return fail(nullptr, RT_E_INVALID,
                    "rt_create_multi: RT_FLAG_RADIANCE is not supported on a multi-device handle");
    return RT_OK;
}

// The empty state of a handle over `devices`, with the test-only fault
// injection read once (MultiState::Fault, RT_FLAG_TEST_HOOKS); null: out of memory.
MultiState* new_multi_state(const rt_config* cfg, const int32_t* devices, uint32_t n_devices,
                            uint32_t transport) {
    MultiState* m = new (std::nothrow) MultiState();
    if (!m) return nullptr;
    if (const char* fe = test_env(cfg->flags, "RT_TEST_FAULT")) {
        const std::string f(fe);
        const size_t c = f.find(':');
        const std::string kind = f.substr(0, c);
        m->fault_k = c == std::string::npos ? 0u : static_cast<uint32_t>(strtoul(f.c_str() + c + 1, nullptr, 10));
        m->fault = kind == "create" ? MultiState::kCreate : kind == "comm" ? MultiState::kComm
                 : kind == "slab" ? MultiState::kSlab : kind == "queue" ? MultiState::kQueue
                 : MultiState::kNone;
    }
    m->transport = transport;
    m->devs.assign(devices, devices + n_devices);
    m->peers.assign(n_devices, nullptr);
    m->cs.assign(n_devices, nullptr);
    for (int f = 0; f < MultiState::F; ++f) {
        m->slab[f].assign(n_devices, nullptr);
        m->rendered[f].assign(n_devices, nullptr);
        m->sent[f].assign(n_devices, nullptr);
        m->t_start[f].assign(n_devices, nullptr);
        m->t_end[f].assign(n_devices, nullptr);
    }
    return m;
}

// Every device's comm stream and per-slot events (peer access for the
// peer-copy transport), then devices[0]'s output stream and events.
int multi_streams_and_events(rt_renderer* r) {
    MultiState* m = r->multi;
    const std::vector<int>& devices = m->devs;
    for (size_t k = 0; k < devices.size(); ++k) {
        hipError_t e = hipSetDevice(devices[k]);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&m->cs[k], hipStreamNonBlocking);
        for (int f = 0; f < MultiState::F && e == hipSuccess; ++f) {
            e = hipEventCreateWithFlags(&m->rendered[f][k], hipEventDisableTiming);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&m->sent[f][k], hipEventDisableTiming);
            // t_start / t_end time device k's render (rt_get_multi_timing)
            if (e == hipSuccess) e = hipEventCreate(&m->t_start[f][k]);
            if (e == hipSuccess) e = hipEventCreate(&m->t_end[f][k]);
        }
        if (e != hipSuccess)
            return hip_fail(r, e, ("rt_create_multi: streams/events" + peer_name(*m, k)).c_str());
        if (k && m->transport == RT_TRANSPORT_PEER && devices[k] != devices[0]) {
            int can = 0;
            if (hipDeviceCanAccessPeer(&can, devices[0], devices[k]) == hipSuccess && can) {
                (void)hipSetDevice(devices[0]);
                (void)hipDeviceEnablePeerAccess(devices[k], 0);  // already enabled is fine
                (void)hipGetLastError();
            }
        }
    }
    hipError_t e = hipSetDevice(devices[0]);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&m->out, hipStreamNonBlocking);
    for (int f = 0; f < MultiState::F && e == hipSuccess; ++f) {
        e = hipEventCreateWithFlags(&m->recvd[f], hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&m->unpacked[f], hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreate(&m->t_unpacked[f]);
    }
    if (e == hipSuccess) e = hipEventCreateWithFlags(&m->out_ready, hipEventDisableTiming);
    return e == hipSuccess ? RT_OK : hip_fail(r, e, "rt_create_multi: events");
}

// The RCCL transport's communicators, one per device.
int multi_communicators(rt_renderer* r) {
    MultiState* m = r->multi;
    const int n = static_cast<int>(m->devs.size());
    m->comms.assign(m->devs.size(), nullptr);
    const ncclResult_t e = m->fault == MultiState::kComm
                               ? ncclInternalError  // RT_TEST_FAULT=comm
                               : rccl_api().CommInitAll(m->comms.data(), n, m->devs.data());
    if (e == ncclSuccess) return RT_OK;
    m->comms.clear();
    std::string devs;
    for (int k = 0; k < n; ++k) devs += (k ? "," : "") + std::to_string(m->devs[k]);
    return nccl_fail(r, e, ("ncclCommInitAll over devices [" + devs + "]").c_str());
}

}  // namespace

namespace rtamd {

// Wait for all of the handle's queued work: every device's render and comm
// streams, devices[0]'s output stream and the unpacks.
int multi_wait(rt_renderer* r) {
    MultiState& m = *r->multi;
    for (size_t k = 0; k < m.devs.size(); ++k) {
        RT_HIP(r, hipSetDevice(m.devs[k]));
        if (k < m.cs.size() && m.cs[k]) RT_HIP(r, hipStreamSynchronize(m.cs[k]));
        // (a creation that failed part-way leaves later peers unmade)
        rt_renderer* p = m.peers[k];
        if (!p) continue;
        RT_HIP(r, hipStreamSynchronize(p->stream));
        if (p->pending) RT_HIP(r, hipEventSynchronize(p->done));
    }
    RT_HIP(r, hipSetDevice(m.devs[0]));
    if (m.out) RT_HIP(r, hipStreamSynchronize(m.out));
    for (int f = 0; f < MultiState::F; ++f)
        if (m.unpacked[f]) RT_HIP(r, hipEventSynchronize(m.unpacked[f]));
    return RT_OK;
}

// Every device's failure word (queue_report): a device whose frame the wave
// queue's bounded wait marked incomplete had its slab gathered and unpacked
// incomplete, so the handle reports RT_E_HIP naming that device, as a
// single-device renderer does for itself.  A host read, no sync.
int multi_queue_report(rt_renderer* r) {
    MultiState& m = *r->multi;
    for (size_t k = 0; k < m.peers.size(); ++k) {
        rt_renderer* p = m.peers[k];
        if (!p) continue;
        if (const int st = queue_report(p)) return fail(r, st, p->err + peer_name(m, k));
    }
    return RT_OK;
}

// multi_wait, then every device's failure word.
int multi_synchronize(rt_renderer* r) {
    int st;
    if ((st = multi_wait(r))) return st;
    if ((st = multi_queue_report(r))) return st;
    return set_device(r);
}

int multi_render(rt_renderer* r, uint32_t* out, hipStream_t hs, rt_stats* stats) {
    MultiState& m = *r->multi;
    int st;
    if (r->cfg.mode == RT_MODE_SCENE && !r->has_scene)
        return fail(r, RT_E_NOSCENE, "RT_MODE_SCENE render without rt_set_scene");
    if (m.broken)
        return fail(r, RT_E_STATE, "rt_render: a resize failed on one of the devices: resize again");
    if ((st = multi_plan(r))) return st;
    if (!hs) hs = m.out;
    const uint32_t n = static_cast<uint32_t>(m.devs.size()), ts = MultiState::kTs;
    const int f = static_cast<int>(m.frame % MultiState::F);
    const auto t0 = std::chrono::steady_clock::now();
    const bool timed = m.timing;
    m.timed[f] = false;
    rt_stats sum{};
    // 1. every device renders its tiles into its slab of slot f
    for (uint32_t k = 0; k < n; ++k) {
        rt_renderer* p = m.peers[k];
        RT_HIP(r, hipSetDevice(m.devs[k]));
        if (m.used[f]) RT_HIP(r, hipStreamWaitEvent(p->stream, m.sent[f][k], 0));
        if (timed) RT_HIP(r, hipEventRecord(m.t_start[f][k], p->stream));
        rt_stats sk{};
        st = render_tiles_one(p, m.ids[k].data(), static_cast<uint32_t>(m.ids[k].size()), ts,
                              m.slab[f][k], p->stream, stats ? &sk : nullptr);
        if (st) {
            r->err = p->err + peer_name(m, k);
            return st;
        }
        if (stats) {
            sum.primary_rays += sk.primary_rays;
            sum.shadow_rays += sk.shadow_rays;
            sum.nodes_visited += sk.nodes_visited;
            sum.prims_tested += sk.prims_tested;
            sum.samples_per_pixel = sk.samples_per_pixel;
        }
        if (timed) RT_HIP(r, hipEventRecord(m.t_end[f][k], p->stream));
        RT_HIP(r, hipEventRecord(m.rendered[f][k], p->stream));
        RT_HIP(r, hipStreamWaitEvent(m.cs[k], m.rendered[f][k], 0));
    }
    // 2. the slabs to devices[0]: recv[f] + k * slab
    RT_HIP(r, hipSetDevice(m.devs[0]));
    if (m.used[f]) RT_HIP(r, hipStreamWaitEvent(m.cs[0], m.unpacked[f], 0));
    char* rb = static_cast<char*>(m.recv[f]);
    if (m.transport == RT_TRANSPORT_RCCL) {
        RcclApi& api = rccl_api();
        RT_NCCL(r, api.GroupStart());
        for (uint32_t k = 0; k < n; ++k) {
            ncclResult_t e = api.Send(m.slab[f][k], m.slab_bytes, ncclUint8, 0, m.comms[k], m.cs[k]);
            if (e == ncclSuccess)
                e = api.Recv(rb + k * m.slab_bytes, m.slab_bytes, ncclUint8, static_cast<int>(k),
                             m.comms[0], m.cs[0]);
            if (e != ncclSuccess) {
                (void)api.GroupEnd();
                return nccl_fail(r, e, "ncclSend/ncclRecv");
            }
        }
        RT_NCCL(r, api.GroupEnd());
        for (uint32_t k = 0; k < n; ++k) {
            RT_HIP(r, hipSetDevice(m.devs[k]));
            RT_HIP(r, hipEventRecord(m.sent[f][k], m.cs[k]));
        }
    } else {
        for (uint32_t k = 0; k < n; ++k) {
            RT_HIP(r, hipSetDevice(m.devs[k]));
            // the copy writes devices[0]'s receive buffer from device k's stream:
            // after frame j-2's unpack has read it
            if (k && m.used[f]) RT_HIP(r, hipStreamWaitEvent(m.cs[k], m.unpacked[f], 0));
            RT_HIP(r, hipMemcpyPeerAsync(rb + k * m.slab_bytes, m.devs[0], m.slab[f][k], m.devs[k],
                                         m.slab_bytes, m.cs[k]));
            RT_HIP(r, hipEventRecord(m.sent[f][k], m.cs[k]));
        }
        RT_HIP(r, hipSetDevice(m.devs[0]));
        for (uint32_t k = 1; k < n; ++k) RT_HIP(r, hipStreamWaitEvent(m.cs[0], m.sent[f][k], 0));
    }
    // 3. one unpack of all slabs on devices[0], after the output stream's
    //    earlier work (a mapped display buffer is ready) and the slabs' arrival
    RT_HIP(r, hipSetDevice(m.devs[0]));
    RT_HIP(r, hipEventRecord(m.recvd[f], m.cs[0]));
    // (RT_FLAG_TEST_POISON: the frame's pixels all come from the unpack)
    if (r->cfg.flags & RT_FLAG_TEST_POISON)
        RT_HIP(r, hipMemsetAsync(out, 0xAB, (size_t)r->W * r->H * 4, hs));
    RT_HIP(r, hipEventRecord(m.out_ready, hs));
    RT_HIP(r, hipStreamWaitEvent(m.cs[0], m.out_ready, 0));
    hipError_t e = launch_unpack(static_cast<const uint32_t*>(m.recv[f]), m.d_all_ids, n * m.S, ts,
                                 (r->W + ts - 1) / ts, r->W, r->H, out, m.cs[0]);
    if (e != hipSuccess) return hip_fail(r, e, "multi-device unpack");
    if (timed) RT_HIP(r, hipEventRecord(m.t_unpacked[f], m.cs[0]));
    RT_HIP(r, hipEventRecord(m.unpacked[f], m.cs[0]));
    RT_HIP(r, hipStreamWaitEvent(hs, m.unpacked[f], 0));
    m.used[f] = true;
    m.timed[f] = timed;
    ++m.frame;
    if (stats) {
        RT_HIP(r, hipStreamSynchronize(hs));
        sum.ms = static_cast<float>(
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        if (r->cfg.mode != RT_MODE_SCENE) sum.primary_rays = (uint64_t)r->W * r->H;
        *stats = sum;
    }
    return RT_OK;
}

int multi_set_scene_device(rt_renderer* r, uint32_t n, const rt_octree_params* oct) {
    MultiState& m = *r->multi;
    const uint32_t nd = static_cast<uint32_t>(m.devs.size());
    if (nd < 2) return RT_OK;
    // each other device receives the list into a scratch pair, then builds
    std::vector<void*> sp(nd, nullptr), al(nd, nullptr);
    int st = RT_OK;
    auto release = [&] {
        for (uint32_t k = 1; k < nd; ++k) {
            (void)hipSetDevice(m.devs[k]);
            if (sp[k]) (void)hipFree(sp[k]);
            if (al[k]) (void)hipFree(al[k]);
        }
        (void)hipSetDevice(m.devs[0]);
    };
    const size_t nb = std::max<size_t>(1, (size_t)n) * sizeof(float4);
    const size_t ab = std::max<size_t>(1, (size_t)n) * sizeof(uint32_t);
    for (uint32_t k = 1; k < nd && !st; ++k) {
        hipError_t e = hipSetDevice(m.devs[k]);
        if (e == hipSuccess) e = hipMalloc(&sp[k], nb);
        if (e == hipSuccess) e = hipMalloc(&al[k], ab);
        if (e != hipSuccess) st = hip_fail(r, e, "rt_set_scene_device: broadcast buffers");
    }
    if (!st && n) {
        if (m.transport == RT_TRANSPORT_RCCL) {
            // ncclBroadcast from devices[0]: spheres as 4n floats, albedo as n words
            RcclApi& api = rccl_api();
            ncclResult_t e = api.GroupStart();
            for (uint32_t k = 0; k < nd && e == ncclSuccess; ++k) {
                void* dst = k ? sp[k] : r->d_spheres.p;
                e = api.Broadcast(r->d_spheres.p, dst, (size_t)n * 4, ncclFloat32, 0, m.comms[k], m.cs[k]);
                if (e == ncclSuccess)
                    e = api.Broadcast(r->d_albedo.p, k ? al[k] : r->d_albedo.p, n, ncclUint32, 0,
                                      m.comms[k], m.cs[k]);
            }
            const ncclResult_t e2 = api.GroupEnd();
            if (e == ncclSuccess) e = e2;
            if (e != ncclSuccess) st = nccl_fail(r, e, "ncclBroadcast");
        } else {
            for (uint32_t k = 1; k < nd && !st; ++k) {
                hipError_t e = hipSetDevice(m.devs[k]);
                if (e == hipSuccess)
                    e = hipMemcpyPeerAsync(sp[k], m.devs[k], r->d_spheres.p, m.devs[0], nb, m.cs[k]);
                if (e == hipSuccess)
                    e = hipMemcpyPeerAsync(al[k], m.devs[k], r->d_albedo.p, m.devs[0], ab, m.cs[k]);
                if (e != hipSuccess) st = hip_fail(r, e, "rt_set_scene_device: peer copy");
            }
        }
    }
    for (uint32_t k = 1; k < nd && !st; ++k) {
        st = rt_set_scene_device(m.peers[k], sp[k], al[k], n, oct, m.cs[k]);
        if (st) r->err = m.peers[k]->err + " (device " + std::to_string(m.devs[k]) + ")";
    }
    release();
    return st;
}

void multi_destroy(rt_renderer* r) {
    MultiState* m = r->multi;
    (void)multi_wait(r);
    r->multi = nullptr;
    const size_t n = m->devs.size();
    for (size_t k = 0; k < n; ++k) {
        (void)hipSetDevice(m->devs[k]);
        for (int f = 0; f < MultiState::F; ++f) {
            if (k < m->slab[f].size() && m->slab[f][k]) (void)hipFree(m->slab[f][k]);
            for (auto* ev : {&m->rendered[f], &m->sent[f], &m->t_start[f], &m->t_end[f]})
                if (k < ev->size() && (*ev)[k]) (void)hipEventDestroy((*ev)[k]);
        }
        if (k < m->comms.size() && m->comms[k]) (void)rccl_api().CommDestroy(m->comms[k]);
        if (k < m->cs.size() && m->cs[k]) (void)hipStreamDestroy(m->cs[k]);
        if (k && m->peers[k]) rt_destroy(m->peers[k]);
    }
    (void)hipSetDevice(m->devs[0]);
    for (int f = 0; f < MultiState::F; ++f) {
        if (m->recv[f]) (void)hipFree(m->recv[f]);
        if (m->recvd[f]) (void)hipEventDestroy(m->recvd[f]);
        if (m->unpacked[f]) (void)hipEventDestroy(m->unpacked[f]);
        if (m->t_unpacked[f]) (void)hipEventDestroy(m->t_unpacked[f]);
    }
    if (m->out) (void)hipStreamDestroy(m->out);
    if (m->out_ready) (void)hipEventDestroy(m->out_ready);
    if (m->d_all_ids) (void)hipFree(m->d_all_ids);
    delete m;
}

}  // namespace rtamd

extern "C" {

int rt_create_multi(const rt_config* cfg, const int32_t* devices, uint32_t n_devices,
                    uint32_t transport, rt_renderer** out) {
    if (!cfg || !devices || !out) return fail(nullptr, RT_E_INVALID, "rt_create_multi: null argument");
    *out = nullptr;
    int st;
    if ((st = check_create_multi(cfg, devices, n_devices, &transport))) return st;
    rt_config c0 = *cfg;
    c0.device = devices[0];
    rt_renderer* r = nullptr;
    if ((st = rt_create(&c0, &r))) return st;
    MultiState* m = new_multi_state(cfg, devices, n_devices, transport);
    if (!m) {
        rt_destroy(r);
        return fail(nullptr, RT_E_NOMEM, "rt_create_multi: out of host memory");
    }
    r->multi = m;
    m->peers[0] = r;
    auto bail = [&](int code) {
        g_last_error = r->err.empty() ? g_last_error : r->err;
        rt_destroy(r);  // frees the multi state and the peers made so far
        return code;
    };
    for (uint32_t k = 1; k < n_devices; ++k) {
        rt_config ck = *cfg;
        ck.device = devices[k];
        st = m->fault == MultiState::kCreate && k == m->fault_k
                 ? fail(nullptr, RT_E_NOMEM, "rt_create: injected failure (RT_TEST_FAULT)")
                 : rt_create(&ck, &m->peers[k]);
        if (st) {
            r->err = "rt_create_multi: " + g_last_error + peer_name(*m, k);
            return bail(st);
        }
    }
    // RT_TEST_FAULT=queue:k: peer k's plain frames report themselves failed
    // (rt_create honoured a "queue:0" on every peer: only peer k keeps it)
    for (uint32_t k = 0; k < n_devices; ++k)
        m->peers[k]->test_fault_queue = m->fault == MultiState::kQueue && k == m->fault_k;
    if ((st = multi_streams_and_events(r))) return bail(st);
    if (transport == RT_TRANSPORT_RCCL && (st = multi_communicators(r))) return bail(st);
    // the tile plan and its slabs for the configured size, now: an allocation
    // failure surfaces here, not at the first frame (a resize re-plans)
    if ((st = multi_plan(r))) return bail(st);
    (void)hipSetDevice(devices[0]);
    *out = r;
    return RT_OK;
}

int rt_get_multi_timing(rt_renderer* r, rt_multi_timing* t) {
    if (!r || !t) return fail(r, RT_E_INVALID, "rt_get_multi_timing: null argument");
    if (!r->multi) return fail(r, RT_E_STATE, "rt_get_multi_timing: not a multi-device handle");
    MultiState& m = *r->multi;
    // from now on frames record their timing events
    const bool was_on = m.timing;
    m.timing = true;
    if (!m.frame) return fail(r, RT_E_STATE, "rt_get_multi_timing: no frame rendered yet");
    const int f = static_cast<int>((m.frame - 1) % MultiState::F);
    if (!m.timed[f])
        return fail(r, RT_E_STATE,
                    was_on ? "rt_get_multi_timing: the last frame was not timed"
                           : "rt_get_multi_timing: timing starts with the next frame (frames "
                             "record timing events once it has been asked for)");
    int st;
    if ((st = multi_wait(r))) return st;
    memset(t, 0, sizeof(*t));
    t->n_devices = static_cast<uint32_t>(m.devs.size());
    t->frame = m.frame - 1;
    for (size_t k = 0; k < m.devs.size(); ++k) {
        RT_HIP(r, hipSetDevice(m.devs[k]));
        RT_HIP(r, hipEventElapsedTime(&t->render_ms[k], m.t_start[f][k], m.t_end[f][k]));
    }
    RT_HIP(r, hipSetDevice(m.devs[0]));
    RT_HIP(r, hipEventElapsedTime(&t->deliver_ms, m.t_end[f][0], m.t_unpacked[f]));
    return RT_OK;
}

int rt_get_multi_info(const rt_renderer* r, rt_multi_info* info) {
    if (!r || !info) return RT_E_INVALID;
    memset(info, 0, sizeof(*info));
    info->tile_size = MultiState::kTs;
    if (!r->multi) {
        info->n_devices = 1;
        info->devices[0] = r->device;
        return RT_OK;
    }
    const MultiState& m = *r->multi;
    info->n_devices = static_cast<uint32_t>(m.devs.size());
    for (size_t k = 0; k < m.devs.size(); ++k) info->devices[k] = m.devs[k];
    info->transport = m.transport;
    const uint32_t ts = MultiState::kTs, n = info->n_devices;
    info->slab_tiles = (((r->W + ts - 1) / ts) * ((r->H + ts - 1) / ts) + n - 1) / n;
    info->frames_in_flight = MultiState::F;
    info->frames = m.frame;
    return RT_OK;
}

}  // extern "C"
