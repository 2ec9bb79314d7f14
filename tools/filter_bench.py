#!/usr/bin/env python3
"""Layer-filter time (rt_filter_layer, rt_apply_layer) on a config's scene, beside
what a viewer chooses between: casting more AO rays.

    python tools/filter_bench.py [--config c3] [--reps 10] [--warmup 2] [--rounds 3]
                                 [--torch-reps 3] [--kernel-stats CSV] [--loop N]

Timed with HIP events on one stream, --rounds times alternating over the cases,
each case the median of --reps launches after --warmup; a case's figure is the
median of its rounds' medians:
  filter       rt_filter_layer alone at passes 1, 3 and 5, channels 1 (the frame's
               4-ray AO layer) and 4 (a seeded random float4 layer)
  chain        rt_render_gbuffer (hits, normals) + rt_render_ao (4 rays) +
               rt_filter_layer (3 passes) + rt_apply_layer into the internal
               framebuffer, on the stream, and each of its steps alone
  ao           the unfiltered layer at 4, 16 and 64 rays, in the same process: the
               filter is for beating more rays, so filter(3) is set against the
               time that separates the 4-ray from the 16-ray layer
  torch        the same output computed by a torch program on the same GPU, 25
               shifted tensors a pass (the composition a caller had before);
               whether its values agree is reported, not required
The AO radius is 2 x the scene's mean sphere radius (tools/ao_bench.py's short one).
--loop N: only N filter(3) launches on one channel, for a kernel trace taken in a
run of its own; --kernel-stats CSV: that trace's per-kernel table, from which the
guide-packing kernel's share of the call is recorded.  Prints one JSON line.
Needs a GPU: there is no fallback.
"""
from __future__ import annotations

import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import raytracingstudy_amd as rt  # noqa: E402
from tools import query_bench_common as qb  # noqa: E402

KTAP = (0.375, 0.25, 0.0625)
DEFAULTS = dict(depth_sigma=0.05, normal_power=5)


def torch_filter(torch, v, hit, t, n, passes, depth_sigma, normal_power):
    """rt_filter_layer's specification in torch operations: v (H, W, C), hit (H, W)
    bool, t (H, W), n (H, W, 3), all on the device."""
    pad2 = torch.nn.functional.pad
    H, W, _ = v.shape
    iz = 1.0 / (depth_sigma * t)
    for s in range(passes):
        step = 1 << s
        p = 2 * step
        grow = lambda a: pad2(a.permute(2, 0, 1), (p, p, p, p)).permute(1, 2, 0)  # noqa: E731
        vg, ng = grow(v), grow(n)
        tg = grow(t[..., None])[..., 0]
        hg = grow(hit[..., None].to(torch.float32))[..., 0] > 0
        sw = torch.zeros_like(t)
        sv = torch.zeros_like(v)
        for j in range(-2, 3):
            for i in range(-2, 3):
                y0, x0 = p + j * step, p + i * step
                nq, tq = ng[y0:y0 + H, x0:x0 + W], tg[y0:y0 + H, x0:x0 + W]
                on = hit & hg[y0:y0 + H, x0:x0 + W]
                dn = (n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2]
                wn = torch.clamp_min(dn, 0.0)
                for _ in range(normal_power):
                    wn = wn * wn
                e = (tq - t) * iz
                w = torch.where(on, (KTAP[abs(i)] * KTAP[abs(j)] * wn) * (1.0 / (1.0 + e * e)), torch.zeros_like(t))
                sw = sw + w
                sv = sv + torch.where(on[..., None], w[..., None] * vg[y0:y0 + H, x0:x0 + W], torch.zeros_like(v))
        v = torch.where((hit & (sw > 0))[..., None], sv / sw[..., None], v)
    return v


def pack_share(path):
    """The guide-packing kernel's share of the filter kernels' time in a rocprofv3
    kernel-stats table (--kernel-trace --stats of a --loop run)."""
    rows = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            if "filter_" in row["Name"]:
                key = "pack" if "filter_pack" in row["Name"] else "pass"
                ent = rows.setdefault(key, {"calls": 0, "total_ns": 0})
                ent["calls"] += int(row["Calls"])
                ent["total_ns"] += int(float(row["TotalDurationNs"]))
    if set(rows) != {"pack", "pass"}:
        sys.exit(f"filter_bench: {path} holds no filter kernels")
    total = rows["pack"]["total_ns"] + rows["pass"]["total_ns"]
    return {"what": "rocprofv3 --kernel-trace --stats of `filter_bench.py --loop`: 3 passes, 1 channel",
            "pack_calls": rows["pack"]["calls"], "pass_calls": rows["pass"]["calls"],
            "pack_us_per_call": round(rows["pack"]["total_ns"] / rows["pack"]["calls"] / 1e3, 2),
            "pass_us_per_launch": round(rows["pass"]["total_ns"] / rows["pass"]["calls"] / 1e3, 2),
            "pack_share_of_kernel_time": round(rows["pack"]["total_ns"] / total, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--loop", type=int, default=0)
    args = ap.parse_args()
    import torch

    if rt.device_count() == 0:
        sys.exit("filter_bench: no HIP device visible (times are measured on the GPU only)")
    r, sp, info, _ = qb.scene_renderer(args.config)
    W, H = r.width, r.height
    radius = 2.0 * float(sp[:, 3].astype(np.float64).mean())
    stream = torch.cuda.Stream()
    s_ptr = stream.cuda_stream
    dev = torch.device("cuda")
    d_hits = torch.empty((H, W, 2), dtype=torch.int32, device=dev)
    d_nrm = torch.empty((H, W, 4), dtype=torch.float32, device=dev)
    d_ao = torch.empty((H, W), dtype=torch.float32, device=dev)
    d_flt = torch.empty((H, W), dtype=torch.float32, device=dev)
    d_in4 = torch.from_numpy(np.random.default_rng(30).random((H, W, 4)).astype(np.float32)).to(dev)
    d_out4 = torch.empty_like(d_in4)
    torch.cuda.synchronize()

    def gbuffer():
        r.render_gbuffer_device(d_hits.data_ptr(), d_nrm.data_ptr(), stream=s_ptr)

    def ao(rays):
        r.render_ao_device(rays, radius, d_ao.data_ptr(), stream=s_ptr)

    def flt(passes, channels=1):
        src, dst = (d_ao, d_flt) if channels == 1 else (d_in4, d_out4)
        r.filter_layer_device(src.data_ptr(), dst.data_ptr(), d_hits.data_ptr(), d_nrm.data_ptr(), passes, channels,
                              stream=s_ptr, **DEFAULTS)

    def apply():
        r.apply_layer_device(d_flt.data_ptr(), 0.25, stream=s_ptr)

    def chain():
        gbuffer()
        ao(4)
        flt(3)
        apply()

    r.render(stream=s_ptr)      # a frame in the internal framebuffer for the multiply
    gbuffer()
    ao(4)
    if args.loop:
        for _ in range(args.loop):
            flt(3)
        stream.synchronize()
        r.synchronize()
        r.close()
        return

    cases = {f"filter_p{p}_c{c}": (lambda p=p, c=c: flt(p, c)) for c in (1, 4) for p in (1, 3, 5)}
    cases.update(gbuffer=gbuffer, apply=apply, chain_gbuffer_ao4_filter3_apply=chain,
                 frame=lambda: r.render(stream=s_ptr))
    cases.update({f"ao{n}": (lambda n=n: ao(n)) for n in (4, 16, 64)})
    rounds = {k: [] for k in cases}
    for _ in range(args.rounds):
        for name, fn in cases.items():
            for _ in range(args.warmup):
                fn()
            rounds[name].append(qb.ms_row([qb.event_ms(fn, stream) for _ in range(args.reps)]))
    ao(4)       # the layer the filter cases and the torch program read is the 4-ray one again
    stream.synchronize()
    out = {"config": args.config, "width": W, "height": H, "reps": args.reps, "warmup": args.warmup,
           "rounds": args.rounds, "scene": qb.scene_summary(info), "ao_radius": round(radius, 6),
           "filter_params": DEFAULTS, "cases": {}}
    med = {}
    for name, rows in rounds.items():
        med[name] = float(np.median([x["ms_median"] for x in rows]))
        out["cases"][name] = {"ms": round(med[name], 4), "rounds": rows}
    more_rays = med["ao16"] - med["ao4"]
    out["filter3_against_more_rays"] = {
        "filter3_ms": round(med["filter_p3_c1"], 4), "gbuffer_ms": round(med["gbuffer"], 4),
        "ao4_ms": round(med["ao4"], 4), "ao16_ms": round(med["ao16"], 4), "ao64_ms": round(med["ao64"], 4),
        "ao16_minus_ao4_ms": round(more_rays, 4),
        "filter3_over_ao16_minus_ao4": round(med["filter_p3_c1"] / more_rays, 3),
        "filter3_plus_gbuffer_over_ao16_minus_ao4": round((med["filter_p3_c1"] + med["gbuffer"]) / more_rays, 3),
        "chain_ms": round(med["chain_gbuffer_ao4_filter3_apply"], 4),
        "chain_over_ao16": round(med["chain_gbuffer_ao4_filter3_apply"] / med["ao16"], 3),
        "chain_over_frame": round(med["chain_gbuffer_ao4_filter3_apply"] / med["frame"], 3)}

    # the torch program: the same output from 25 shifted tensors a pass
    hit = d_hits[..., 1] != -1
    t = d_hits[..., 0].contiguous().view(torch.float32)
    n3 = d_nrm[..., :3].contiguous()
    out["torch"] = {}
    for channels, passes in ((1, 3), (4, 3)):
        src = d_ao[..., None] if channels == 1 else d_in4
        with torch.cuda.stream(stream):
            ref = torch_filter(torch, src, hit, t, n3, passes, **DEFAULTS)      # warm
            ms = [qb.event_ms(lambda: torch_filter(torch, src, hit, t, n3, passes, **DEFAULTS), stream)
                  for _ in range(args.torch_reps)]
            flt(passes, channels)
        stream.synchronize()
        r.synchronize()
        got = (d_flt[..., None] if channels == 1 else d_out4)
        name = f"filter_p{passes}_c{channels}"
        diff = (got - ref).abs()
        out["torch"][name] = {**qb.ms_row(ms, 3), "torch_over_filter": round(float(np.median(ms)) / med[name], 1),
                              "elements": int(got.numel()),
                              "same_bits": int((got.view(torch.int32) == ref.view(torch.int32)).sum().item()),
                              "max_abs_diff": float(diff.max().item())}
    if args.kernel_stats:
        out["pack_kernel"] = pack_share(args.kernel_stats)
    out["not_measured"] = "other scenes, sizes and cameras; a per-counter profile of the kernels"
    print(json.dumps(out))
    r.close()


if __name__ == "__main__":
    main()
