#!/usr/bin/env python3
"""One-bounce diffuse layer time (rt_render_indirect) on a config's scene, beside
rt_render_ao at the same settings, the stages of the viewer's chain, and the
composition a caller had before it.

    python tools/indirect_bench.py [--config c3] [--rays 1,4,16] [--comp-rays 4] [--reps 10]
                                   [--warmup 2] [--passes 3] [--comp-reps 2] [--chunk-log2 24]

Per setting (rays a pixel x radius: 2 x and 8 x the scene's mean sphere radius,
and +inf), timed with HIP events on one stream, --passes rounds alternating:
  indirect     rt_render_indirect, both outputs: the median of --reps launches after --warmup
  ao           rt_render_ao, both outputs, the same way
  composition  (--comp-rays only) what a caller composes without the call, in this
               order: rt_render_gbuffer (hits), then per chunk of rows a torch
               program that builds the bounce rays' rt_ray records (tools/ao_bench.py
               torch_rays), rt_trace_rays(NEAREST), torch shading of the hits and
               the lit hits' shadow records, rt_trace_rays(ANY), and a torch sum
               per pixel: --comp-reps runs after one
How many of the layer's words the composition gets the same is reported, not
required: torch rounds a division or a square root on its own in places and sums
in another order.  Beside them, in the same process: the G-buffer (three
outputs), the config's own plain frame, rt_add_layer, and the whole
moving-camera chain per frame (G-buffer, indirect at 4 rays and 8 mean radii with
salt = the frame number, rt_reproject_layer and rt_filter_layer at channels = 4,
the frame, rt_add_layer).  Prints one JSON line.  Needs a GPU: there is no fallback.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import raytracingstudy_amd as rt  # noqa: E402
from tools import query_bench_common as qb  # noqa: E402
from tools.ao_bench import torch_rays  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--rays", default="1,4,16")
    ap.add_argument("--comp-rays", default="4")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--comp-reps", type=int, default=2)
    ap.add_argument("--chunk-log2", type=int, default=24, help="most rays of one composition chunk")
    args = ap.parse_args()
    import torch

    import ao_ref as ar
    import indirect_ref as ir
    if rt.device_count() == 0:
        sys.exit("indirect_bench: no HIP device visible (times are measured on the GPU only)")
    r, sp, info, pose = qb.scene_renderer(args.config)
    _, al = rt.configs.scene_spheres(rt.CONFIGS[args.config], rt.SEED)
    W, H = r.width, r.height
    n = W * H
    pose_np, K = r.camera()
    mean_r = float(sp[:, 3].astype(np.float64).mean())
    radii = {"2x_mean_r": 2.0 * mean_r, "8x_mean_r": 8.0 * mean_r, "inf": float("inf")}
    ray_counts = [int(v) for v in args.rays.split(",")]
    comp_rays = [int(v) for v in args.comp_rays.split(",") if v]
    stream = torch.cuda.Stream()
    sp_ = stream.cuda_stream
    dev = torch.device("cuda")
    L = ir.light_toward(ir.LIGHT)
    amb = float(ir.AMBIENT)
    d_sp = torch.from_numpy(sp).to(dev)
    d_al = torch.from_numpy(np.ascontiguousarray(al, np.uint32).astype(np.int64)).to(dev)
    d_L = torch.from_numpy(L).to(dev)
    d_layer = torch.empty((H, W, 4), dtype=torch.float32, device=dev)
    d_occ = torch.empty((H, W), dtype=torch.int32, device=dev)
    d_ao = torch.empty((H, W), dtype=torch.float32, device=dev)
    d_hits = torch.empty((n, 2), dtype=torch.int32, device=dev)
    d_comp = torch.zeros((n, 4), dtype=torch.float32, device=dev)
    d_dirs = torch.from_numpy(qb.camera_rays(n, W, H, pose_np, K)[:, 4:7].copy()).to(dev)
    d_o = torch.from_numpy(pose_np[3, :3].copy()).to(dev)
    # the chain's two buffer sets: {hits, normals, albedo, this frame's layer, the carried mean, its count}
    sets = [dict(hits=torch.empty((n, 2), dtype=torch.int32, device=dev),
                 nrm=torch.empty((n, 4), dtype=torch.float32, device=dev),
                 alb=torch.empty(n, dtype=torch.int32, device=dev),
                 cur=torch.empty((n, 4), dtype=torch.float32, device=dev),
                 out=torch.empty((n, 4), dtype=torch.float32, device=dev),
                 count=torch.empty(n, dtype=torch.float32, device=dev)) for _ in range(2)]
    d_flt = torch.empty((n, 4), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()

    def plain_frame():
        r.render(stream=sp_)
    for _ in range(5):
        plain_frame()
    frame_ms = [qb.event_ms(plain_frame, stream) for _ in range(20)]
    r.synchronize()

    def indirect(rays, radius, stats=False):
        return r.render_indirect_device(rays, radius, d_layer.data_ptr(), d_occ.data_ptr(), 0, 1.0, stream=sp_,
                                        stats=stats)

    def ao(rays, radius):
        return r.render_ao_device(rays, radius, d_ao.data_ptr(), d_occ.data_ptr(), 0, stream=sp_)

    def gbuffer():
        s = sets[0]
        r.render_gbuffer_device(s["hits"].data_ptr(), s["nrm"].data_ptr(), s["alb"].data_ptr(), stream=sp_)

    def add_layer():
        r.add_layer_device(d_layer.data_ptr(), 1.0, sets[0]["alb"].data_ptr(), stream=sp_)

    def trace(recs, kind):
        out = torch.empty((recs.shape[0], 2), dtype=torch.int32, device=dev)
        r.trace_rays_device(recs.data_ptr(), recs.shape[0], out.data_ptr(), kind, stream=sp_)
        return out

    def composition(rays, radius):
        key = int(ar.key(0)[0])
        with torch.cuda.stream(stream):
            r.render_gbuffer_device(d_hits.data_ptr(), stream=sp_)
            d_comp.zero_()
            d_comp[:, 3] = 1.0
            rows = max(1, (1 << args.chunk_log2) // (rays * W))
            for y0 in range(0, H, rows):
                a, b = y0 * W, min(H, y0 + rows) * W
                hits = d_hits[a:b]
                pix = torch.nonzero(hits[:, 1] != -1).reshape(-1)
                if pix.numel() == 0:
                    continue
                pid = pix + a
                t = hits[pix, 0].view(torch.float32)
                rec = d_sp[hits[pix, 1].to(torch.int64)]
                recs = torch_rays(torch, ar, key, pid, d_o, t, d_dirs[pid], rec, rays, radius)
                out = trace(recs, "nearest")
                hit = out[:, 1] != -1
                d = recs[:, 4:7]
                col = torch.stack([torch.full_like(d[:, 1], 200.0 / 255.0), d[:, 1].clamp(0.0, 1.0),
                                   d[:, 2].clamp(0.0, 1.0)], dim=1)
                at = torch.nonzero(hit).reshape(-1)
                if at.numel():
                    s = out[at, 1].to(torch.int64)
                    rec2 = d_sp[s]
                    q = recs[at, :3] + out[at, 0].view(torch.float32)[:, None] * d[at]
                    m = (q - rec2[:, :3]) * (1.0 / rec2[:, 3])[:, None]
                    ndl = (m[:, 0] * d_L[0] + m[:, 1] * d_L[1]) + m[:, 2] * d_L[2]
                    lam = ndl.clamp(min=0.0)
                    lit = torch.nonzero(ndl > 0).reshape(-1)
                    if lit.numel():
                        srec = torch.zeros((lit.numel(), 8), dtype=torch.float32, device=dev)
                        srec[:, :3] = q[lit] + m[lit] * float(ar.SHADOW_EPS)
                        srec[:, 4:7] = d_L
                        srec[:, 7] = float("inf")
                        sh = trace(srec, "any")
                        lam[lit] = torch.where(sh[:, 1] != -1, torch.zeros_like(lam[lit]), lam[lit])
                    f = amb + (1.0 - amb) * lam
                    word = d_al[s]
                    col[at] = torch.stack([((word >> (8 * k)) & 0xFF).to(torch.float32) * (1.0 / 255.0) * f
                                           for k in range(3)], dim=1)
                d_comp[pid, :3] = col.view(-1, rays, 3).sum(dim=1) * (1.0 / rays)
                d_comp[pid, 3] = (rays - hit.view(-1, rays).sum(dim=1)).to(torch.float32) * (1.0 / rays)

    # the viewer's loop on a moving camera, per frame, two buffer sets swapped
    chain_state = dict(k=0, hist=None)

    def chain_frame():
        k = chain_state["k"]
        s = sets[k & 1]
        p = pose_np.copy()
        p[3, :3] += np.float32(0.002) * np.float32(k % 8) * np.array([1.0, -0.5, 0.25], np.float32)
        r.setPosition(p)
        r.render_gbuffer_device(s["hits"].data_ptr(), s["nrm"].data_ptr(), s["alb"].data_ptr(), stream=sp_)
        r.render_indirect_device(4, radii["8x_mean_r"], s["cur"].data_ptr(), None, k, 1.0, stream=sp_)
        r.reproject_layer_device(s["hits"].data_ptr(), s["cur"].data_ptr(), s["out"].data_ptr(), s["count"].data_ptr(),
                                 chain_state["hist"], 4, stream=sp_)
        r.filter_layer_device(s["out"].data_ptr(), d_flt.data_ptr(), s["hits"].data_ptr(), s["nrm"].data_ptr(), 3, 4,
                              stream=sp_)
        r.render(stream=sp_)
        r.add_layer_device(d_flt.data_ptr(), 1.0, s["alb"].data_ptr(), stream=sp_)
        chain_state["hist"] = dict(hits=s["hits"].data_ptr(), layer=s["out"].data_ptr(), count=s["count"].data_ptr(),
                                   pose=p.reshape(16), K=np.asarray(K, np.float32).reshape(9))
        chain_state["k"] = k + 1

    out = {"config": args.config, "width": W, "height": H, "reps": args.reps, "warmup": args.warmup,
           "passes": args.passes, "comp_reps": args.comp_reps, "scene": qb.scene_summary(info),
           "mean_radius": round(mean_r, 6),
           "frame": {"spp": rt.CONFIGS[args.config].spp, "what": "plain frames, HIP events on the stream",
                     **qb.ms_row(frame_ms)},
           "not_measured": "other scenes and cameras; the shadow walks' share of the kernel's time; a per-counter "
                           "profile of the kernel"}
    for name, fn in (("gbuffer", gbuffer), ("add_layer", add_layer), ("chain_frame", chain_frame)):
        rounds = []
        for _ in range(args.passes):
            for _ in range(args.warmup):
                fn()
            rounds.append(qb.ms_row([qb.event_ms(fn, stream) for _ in range(args.reps)]))
        out[name] = {"rounds": rounds, "ms": round(float(np.median([p["ms_median"] for p in rounds])), 4)}
    out["chain_frame"]["what"] = ("set_pose, G-buffer (3 outputs), indirect 4 rays at 8 mean radii, reproject and "
                                  "3-pass filter at channels 4, the plain frame, add_layer")
    r.setPosition(pose_np)
    r.synchronize()
    hit_px = d_hit_pixels(r, sets, sp_, torch)
    out["hit_pixels"] = hit_px
    for rays in ray_counts:
        for rname, radius in radii.items():
            comp = rays in comp_rays
            row = {"rays": rays, "radius": radius if np.isfinite(radius) else "inf", "indirect_passes": [],
                   "ao_passes": [], "composition_passes": []}
            for _ in range(args.passes):
                for _ in range(args.warmup):
                    indirect(rays, radius)
                row["indirect_passes"].append(
                    qb.ms_row([qb.event_ms(lambda: indirect(rays, radius), stream) for _ in range(args.reps)]))
                for _ in range(args.warmup):
                    ao(rays, radius)
                row["ao_passes"].append(
                    qb.ms_row([qb.event_ms(lambda: ao(rays, radius), stream) for _ in range(args.reps)]))
                if comp:
                    composition(rays, radius)
                    cms = [qb.event_ms(lambda: composition(rays, radius), stream) for _ in range(args.comp_reps)]
                    row["composition_passes"].append(qb.ms_row(cms, 3))
            st = indirect(rays, radius, stats=True)
            r.synchronize()
            stream.synchronize()
            med = float(np.median([p["ms_median"] for p in row["indirect_passes"]]))
            amed = float(np.median([p["ms_median"] for p in row["ao_passes"]]))
            cast = int(st.shadow_rays)
            bounce = rays * hit_px
            row.update(indirect_ms=round(med, 4), ao_ms=round(amed, 4), indirect_over_ao=round(med / amed, 2),
                       indirect_over_frame=round(med / out["frame"]["ms_median"], 2),
                       rays_cast=cast, bounce_rays=bounce, shadow_rays=cast - bounce,
                       Mrays_s=round((cast + st.primary_rays) / med / 1e3, 1),
                       nodes_per_ray=round(st.nodes_visited / max(1, cast + st.primary_rays), 3),
                       tests_per_ray=round(st.prims_tested / max(1, cast + st.primary_rays), 3),
                       hit_fraction=round(float(d_occ.sum().item()) / max(1, bounce), 4), pixels=n)
            if comp:
                cmed = float(np.median([p["ms_median"] for p in row["composition_passes"]]))
                same = (d_comp.view(torch.int32) == d_layer.view(n, 4).view(torch.int32))
                row.update(composition_ms=round(cmed, 3), composition_over_indirect=round(cmed / med, 2),
                           fused_below_composition_each_round=[
                               a["ms_median"] < b["ms_median"]
                               for a, b in zip(row["indirect_passes"], row["composition_passes"])],
                           composition_same_words=int(same.sum().item()), words=4 * n,
                           composition_same_w=int(same[:, 3].sum().item()))
            else:
                del row["composition_passes"]
            out[f"rays{rays}_{rname}"] = row
            print(f"indirect_bench: rays {rays} radius {rname}: indirect {med:.3f} ms, ao {amed:.3f} ms"
                  + (f", composition {row['composition_ms']:.1f} ms" if comp else ""), file=sys.stderr, flush=True)
    print(json.dumps(out))
    r.close()


def d_hit_pixels(r, sets, stream_ptr, torch):
    """The frame's hit pixels under the handle's current camera (the G-buffer's count)."""
    s = sets[0]
    r.render_gbuffer_device(s["hits"].data_ptr(), stream=stream_ptr)
    r.synchronize()
    torch.cuda.synchronize()
    return int((s["hits"][:, 1] != -1).sum().item())


if __name__ == "__main__":
    main()
