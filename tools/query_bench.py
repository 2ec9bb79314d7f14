#!/usr/bin/env python3
"""Ray-query throughput (rt_trace_rays) on a config's scene, coherent and incoherent rays.

    python tools/query_bench.py [--config c3] [--log2-rays 22] [--reps 20] [--warmup 3]
                                [--multi K[,K...]]

Two ray sets of 2^k rays each, nearest and any-hit, timed with HIP events around
the launch on a stream (median of --reps launches after --warmup):
  coherent    the config's own frame: pixel-centre camera rays in row-major
              order (repeated from the first pixel when the frame has fewer)
  incoherent  origins just off random spheres' surfaces, uniformly random
              directions (neighbouring lanes share nothing)
Prints one JSON line: Mrays/s, hit fraction and the walk's work per ray (from
one stats launch) for each set and kind.  With --multi, also the ordered
multi-hit query (rt_trace_rays_multi) for each K on the same two ray sets in
the same process, next to the nearest query: ms, Mrays/s, the mean count per
ray, nodes and tests per ray, and the ratios to one and to K nearest launches.
Needs a GPU: there is no fallback.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import raytracingstudy_amd as rt  # noqa: E402
from tools import query_bench_common as qb  # noqa: E402


def surface_rays(n: int, sp: np.ndarray, seed: int) -> np.ndarray:
    g = np.random.default_rng(seed)

    def unit(m):
        x = g.normal(size=(m, 3))
        return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)

    k = g.integers(0, len(sp), n)
    rays = np.zeros((n, 8), np.float32)
    rays[:, :3] = sp[k, :3] + np.float32(1.001) * sp[k, 3:4] * unit(n)
    rays[:, 3] = 1e-5
    rays[:, 4:7] = unit(n)
    rays[:, 7] = np.inf
    return rays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--log2-rays", type=int, default=22)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--multi", default="", metavar="K[,K...]",
                    help="also time rt_trace_rays_multi for these k (1 .. 16)")
    args = ap.parse_args()
    multi_ks = [int(x) for x in args.multi.split(",") if x]
    if any(k < 1 or k > rt._lib.RT_MULTIHIT_MAX for k in multi_ks):
        sys.exit(f"query_bench: --multi takes k in 1 .. {rt._lib.RT_MULTIHIT_MAX}")
    import torch
    if rt.device_count() == 0:
        sys.exit("query_bench: no HIP device visible (rates are measured on the GPU only)")
    n = 1 << args.log2_rays
    r, sp, info, pose = qb.scene_renderer(args.config)
    _, K = r.camera()
    sets = {"coherent": qb.camera_rays(n, r.width, r.height, pose, K),
            "incoherent": surface_rays(n, sp, 12345)}
    stream = torch.cuda.Stream()
    d_hits = torch.empty((n, 2), dtype=torch.int32, device="cuda")
    out = {"config": args.config, "rays": n, "reps": args.reps, "warmup": args.warmup,
           "scene": qb.scene_summary(info)}

    def timed(launch):
        for _ in range(args.warmup):
            launch()
        return [qb.event_ms(launch, stream) for _ in range(args.reps)]

    d_mhits = d_counts = None
    if multi_ks:
        d_mhits = torch.empty((n, max(multi_ks), 2), dtype=torch.int32, device="cuda")
        d_counts = torch.empty((n,), dtype=torch.int32, device="cuda")
    for name, rays in sets.items():
        d_rays = torch.from_numpy(rays).cuda()
        torch.cuda.synchronize()
        for kind in ("nearest", "any"):
            def launch():
                r.trace_rays_device(d_rays.data_ptr(), n, d_hits.data_ptr(), kind,
                                    stream=stream.cuda_stream)
            ms = timed(launch)
            st = r.trace_rays_device(d_rays.data_ptr(), n, d_hits.data_ptr(), kind,
                                     stream=stream.cuda_stream, stats=True)
            hit = float((d_hits[:, 1] != -1).float().mean().item())
            med = float(np.median(ms))
            out[f"{name}_{kind}"] = {
                **qb.ms_row(ms),
                "Mrays_s": round(n / med / 1e3, 1), "hit_fraction": round(hit, 4),
                "nodes_per_ray": round(st.nodes_visited / n, 3),
                "prims_per_ray": round(st.prims_tested / n, 3),
                "stats_launch_ms": round(float(st.ms), 4)}
        near = out[f"{name}_nearest"]["ms_median"]
        for k in multi_ks:
            def launch_multi():
                r.trace_rays_multi_device(d_rays.data_ptr(), n, k, d_mhits.data_ptr(),
                                          d_counts.data_ptr(), stream=stream.cuda_stream)
            ms = timed(launch_multi)
            st = r.trace_rays_multi_device(d_rays.data_ptr(), n, k, d_mhits.data_ptr(),
                                           d_counts.data_ptr(), stream=stream.cuda_stream, stats=True)
            med = float(np.median(ms))
            out[f"{name}_multi{k}"] = {
                **qb.ms_row(ms),
                "Mrays_s": round(n / med / 1e3, 1),
                "mean_count": round(float(d_counts.float().mean().item()), 4),
                "nodes_per_ray": round(st.nodes_visited / n, 3),
                "prims_per_ray": round(st.prims_tested / n, 3),
                "stats_launch_ms": round(float(st.ms), 4),
                "vs_nearest": round(med / near, 4),
                "vs_k_nearest_launches": round(med / (k * near), 4)}
    print(json.dumps(out))
    r.close()


if __name__ == "__main__":
    main()
