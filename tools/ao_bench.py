#!/usr/bin/env python3
"""Ambient-occlusion layer time (rt_render_ao) on a config's scene, beside the
composition a caller had before it.

    python tools/ao_bench.py [--config c3] [--rays 4,16,64] [--reps 10] [--warmup 2]
                             [--passes 3] [--comp-reps 2] [--chunk-log2 24] [--crop 64]

Per setting (rays a pixel x radius: 2 x and 8 x the scene's mean sphere radius,
and +inf), timed with HIP events on one stream, --passes times alternating:
  ao           rt_render_ao, both outputs: the median of --reps launches after --warmup
  composition  rt_render_gbuffer (hits), then per chunk of rows a torch program
               that compacts the hit pixels and builds their rt_ray records on
               the device (DESIGN.md 5.15's arithmetic in torch operations: the
               hash in int64 under a 32-bit mask, f32 elementwise operations),
               rt_trace_rays(ANY) and a count per pixel: --comp-reps runs after one
Checked, not timed: on a --crop x --crop window in the image's middle, the rays
built on the host by tests/ao_ref.py's arithmetic from the G-buffer's hits and
traced by rt_trace_rays(ANY) must name render_ao's occluded counts (the tool
fails otherwise).  How many of the frame's pixels the composition counts the
same is reported, not required: torch rounds a division or a square root on
its own in places, and a direction one ulp off can flip a grazing ray.  The
config's own plain frame (events on the stream, as bench.py times it) and its
counting frame are reported beside them.  Prints one JSON line.  Needs a GPU: there is no fallback.
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

M32 = 0xFFFFFFFF


def _mix32(x):
    """mix32 on int64 tensors holding 32-bit words (a product's low 32 bits survive int64's wrap)."""
    x = x ^ (x >> 16)
    x = (x * 0x7FEB352D) & M32
    x = x ^ (x >> 15)
    x = (x * 0x846CA68B) & M32
    return x ^ (x >> 16)


def torch_rays(torch, ar, key, pid, o, t, d, rec, rays, radius):
    """(m * rays, 8) rt_ray records of the hit pixels pid (m,) int64: origin
    o + t d (m, 3), sphere records rec (m, 4); ao_ref.directions in torch."""
    p = o[None, :] + t[:, None] * d
    n = (p - rec[:, :3]) * (1.0 / rec[:, 3])[:, None]
    org = p + n * float(ar.SHADOW_EPS)
    m = pid.shape[0]
    hp = _mix32(pid ^ key)[:, None].expand(m, rays).reshape(-1)
    i = torch.arange(rays, device=pid.device, dtype=torch.int64)[None, :].expand(m, rays).reshape(-1)
    nn = n[:, None, :].expand(m, rays, 3).reshape(-1, 3)
    out = nn.clone()
    open_ = torch.ones(m * rays, dtype=torch.bool, device=pid.device)
    lo = float(ar.MIN_LEN2)
    for attempt in range(ar.TRIES):
        hb = _mix32(hp ^ ((i << 3) | attempt))
        c = torch.stack([2.0 * ((_mix32(hb ^ a) >> 8).to(torch.float32) * (1.0 / 16777216.0)) - 1.0
                         for a in ar.AXIS_WORDS], dim=1)
        q = (c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]
        take = open_ & (q >= lo) & (q <= 1.0)
        w = nn + c / torch.sqrt(q)[:, None]
        q2 = (w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2]
        ok = take & (q2 >= lo)
        out = torch.where(ok[:, None], w / torch.sqrt(q2)[:, None], out)
        open_ = open_ & ~take
    recs = torch.zeros((m * rays, 8), dtype=torch.float32, device=pid.device)
    recs[:, :3] = org[:, None, :].expand(m, rays, 3).reshape(-1, 3)
    recs[:, 4:7] = out
    recs[:, 7] = radius
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--rays", default="4,16,64")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--comp-reps", type=int, default=2)
    ap.add_argument("--chunk-log2", type=int, default=24, help="most rays of one composition chunk")
    ap.add_argument("--crop", type=int, default=64)
    args = ap.parse_args()
    import torch

    import ao_ref as ar
    if rt.device_count() == 0:
        sys.exit("ao_bench: no HIP device visible (times are measured on the GPU only)")
    r, sp, info, pose = qb.scene_renderer(args.config)
    W, H = r.width, r.height
    pose_np, K = r.camera()
    mean_r = float(sp[:, 3].astype(np.float64).mean())
    radii = {"2x_mean_r": 2.0 * mean_r, "8x_mean_r": 8.0 * mean_r, "inf": float("inf")}
    ray_counts = [int(v) for v in args.rays.split(",")]
    stream = torch.cuda.Stream()
    dev = torch.device("cuda")
    d_sp = torch.from_numpy(sp).to(dev)
    d_ao = torch.empty((H, W), dtype=torch.float32, device=dev)
    d_occ = torch.empty((H, W), dtype=torch.int32, device=dev)
    d_hits = torch.empty((H * W, 2), dtype=torch.int32, device=dev)
    d_count = torch.zeros(H * W, dtype=torch.int32, device=dev)
    # every pixel's camera ray, once: the composition's caller knows its camera
    d_dirs = torch.from_numpy(qb.camera_rays(W * H, W, H, pose_np, K)[:, 4:7].copy()).to(dev)
    d_o = torch.from_numpy(pose_np[3, :3].copy()).to(dev)
    torch.cuda.synchronize()

    # the config's own frame, for scale: the plain frame a viewer renders, between HIP events on
    # the stream as bench.py times it, after warm frames; and the counting frame (rt_render with
    # stats plans another instance), named as such
    def plain_frame():
        r.render(stream=stream.cuda_stream)
    for _ in range(5):
        plain_frame()
    frame_ms = [qb.event_ms(plain_frame, stream) for _ in range(20)]
    stats_frame_ms = [float(r.render(stats=True).ms) for _ in range(3)]
    r.synchronize()

    def ao(rays, radius, stats=False):
        return r.render_ao_device(rays, radius, d_ao.data_ptr(), d_occ.data_ptr(), 0, stream=stream.cuda_stream,
                                  stats=stats)

    def composition(rays, radius):
        key = int(ar.key(0)[0])
        with torch.cuda.stream(stream):
            r.render_gbuffer_device(d_hits.data_ptr(), stream=stream.cuda_stream)
            d_count.zero_()
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
                out = torch.empty((recs.shape[0], 2), dtype=torch.int32, device=dev)
                r.trace_rays_device(recs.data_ptr(), recs.shape[0], out.data_ptr(), "any",
                                    stream=stream.cuda_stream)
                d_count[pid] = (out[:, 1] != -1).view(-1, rays).sum(dim=1, dtype=torch.int32)
                # (recs and out are the caching allocator's: reused by the next chunk on this stream)

    c = min(args.crop, W, H)
    x0, y0 = (W - c) // 2, (H - c) // 2
    # the crop's pixel-centre directions: Camera::getRay in f32 on the host (the same operations as the device's)
    crop_dirs = qb.camera_rays(W * H, W, H, pose_np, K)[:, 4:7].reshape(H, W, 3)[y0:y0 + c, x0:x0 + c].copy()

    def crop_check(rays, radius):
        """render_ao's counts on the crop against rays built on the host (ao_ref) from the G-buffer's hits."""
        hits = d_hits.cpu().numpy().reshape(H, W, 2)[y0:y0 + c, x0:x0 + c]
        g = dict(sphere=np.ascontiguousarray(hits[..., 1]).view(np.uint32),
                 t=np.ascontiguousarray(hits[..., 0]).view(np.float32),
                 dirs=crop_dirs)
        pid = (np.arange(y0, y0 + c)[:, None] * W + np.arange(x0, x0 + c)[None, :]).astype(np.uint32)
        pixel, recs, _ = ar.rays_of(g, pose_np, sp, rays, radius, 0, pid=pid)
        want = np.zeros(c * c, np.int64)
        if len(pixel):
            _, sphere = r.trace_rays(recs.reshape(-1, 8), "any")
            want[pixel] = (sphere != ar.NO_HIT).reshape(-1, rays).sum(axis=1)
        got = d_occ.cpu().numpy()[y0:y0 + c, x0:x0 + c].reshape(-1)
        return dict(pixels=c * c, hit=int(len(pixel)), same=int((got == want).sum()))

    out = {"config": args.config, "width": W, "height": H, "reps": args.reps, "warmup": args.warmup,
           "passes": args.passes, "comp_reps": args.comp_reps, "scene": qb.scene_summary(info),
           "mean_radius": round(mean_r, 6), "frame": {"spp": rt.CONFIGS[args.config].spp, "what": "plain frames, HIP events on the stream",
                     **qb.ms_row(frame_ms)},
           "stats_frame": {"what": "the counting frame (rt_render with stats), its own device time",
                           **qb.ms_row(stats_frame_ms)},
           "not_measured": "other scenes and cameras; a per-counter profile of the kernel"}
    for rays in ray_counts:
        for rname, radius in radii.items():
            row = {"rays": rays, "radius": radius if np.isfinite(radius) else "inf", "ao_passes": [],
                   "composition_passes": []}
            for _ in range(args.passes):
                for _ in range(args.warmup):
                    ao(rays, radius)
                ms = [qb.event_ms(lambda: ao(rays, radius), stream) for _ in range(args.reps)]
                row["ao_passes"].append(qb.ms_row(ms))
                composition(rays, radius)
                cms = [qb.event_ms(lambda: composition(rays, radius), stream) for _ in range(args.comp_reps)]
                row["composition_passes"].append(qb.ms_row(cms, 3))
            st = ao(rays, radius, stats=True)
            r.synchronize()
            stream.synchronize()
            med = float(np.median([p["ms_median"] for p in row["ao_passes"]]))
            cmed = float(np.median([p["ms_median"] for p in row["composition_passes"]]))
            row.update(ao_ms=round(med, 4), composition_ms=round(cmed, 3),
                       composition_over_ao=round(cmed / med, 2), ao_rays=int(st.shadow_rays),
                       Mrays_s=round((st.shadow_rays + st.primary_rays) / med / 1e3, 1),
                       ao_Mrays_s=round(st.shadow_rays / med / 1e3, 1),
                       nodes_per_ray=round(st.nodes_visited / max(1, st.shadow_rays + st.primary_rays), 3),
                       tests_per_ray=round(st.prims_tested / max(1, st.shadow_rays + st.primary_rays), 3),
                       occluded_fraction=round(float(d_occ.sum().item()) / max(1, st.shadow_rays), 4),
                       composition_same_count=int((d_count == d_occ.reshape(-1)).sum().item()),
                       pixels=W * H, crop=crop_check(rays, radius))
            out[f"rays{rays}_{rname}"] = row
            if row["crop"]["same"] != row["crop"]["pixels"]:
                print(json.dumps(out))
                sys.exit(f"ao_bench: rays {rays} radius {rname}: render_ao and the host-built rays differ on the crop")
            print(f"ao_bench: rays {rays} radius {rname}: ao {med:.3f} ms, composition {cmed:.1f} ms",
                  file=sys.stderr, flush=True)
    print(json.dumps(out))
    r.close()


if __name__ == "__main__":
    main()
