#!/usr/bin/env python3
"""G-buffer pass time (rt_render_gbuffer) on a config's scene, next to
rt_trace_rays on the same pixel-centre rays.

    python tools/gbuffer_bench.py [--config c3] [--reps 20] [--warmup 3] [--passes 2]

Three rows at the config's frame size, each timed with HIP events around the
launch on a stream (median of --reps launches after --warmup):
  gbuffer_all    hits, normals and albedo
  gbuffer_hits   the hits buffer alone
  trace_rays     rt_trace_rays, nearest, on the frame's W*H pixel-centre rays
                 in row-major order (32 B read and 8 B written per ray)
The rows alternate launch by launch inside a pass, and the whole measurement
runs --passes times in this process: the difference between a row's medians
is the noise a difference between rows has to exceed.  Prints one JSON line
with every pass's median / min / max per row, the hit fraction, the walk's
work per ray (one stats launch) and whether the two paths' hits agree (the
rays are restated in numpy, so a last-bit difference in a direction can move
a grazing hit).  Needs a GPU: there is no fallback.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--passes", type=int, default=2)
    args = ap.parse_args()
    import torch
    if rt.device_count() == 0:
        sys.exit("gbuffer_bench: no HIP device visible (times are measured on the GPU only)")
    r, _, info, pose = qb.scene_renderer(args.config)
    w, h = r.width, r.height
    n = w * h
    _, K = r.camera()
    stream = torch.cuda.Stream()
    d_rays = torch.from_numpy(qb.camera_rays(n, w, h, pose, K)).cuda()
    d_hits = torch.empty((n, 2), dtype=torch.int32, device="cuda")
    d_qhits = torch.empty((n, 2), dtype=torch.int32, device="cuda")
    d_nrm = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    d_alb = torch.empty((n,), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    s = stream.cuda_stream
    rows = {
        "gbuffer_all": lambda: r.render_gbuffer_device(d_hits.data_ptr(), d_nrm.data_ptr(),
                                                       d_alb.data_ptr(), stream=s),
        "gbuffer_hits": lambda: r.render_gbuffer_device(d_hits.data_ptr(), stream=s),
        "trace_rays": lambda: r.trace_rays_device(d_rays.data_ptr(), n, d_qhits.data_ptr(), "nearest",
                                                  stream=s),
    }
    out = {"config": args.config, "width": w, "height": h, "rays": n, "reps": args.reps,
           "warmup": args.warmup,
           "scene": qb.scene_summary(info), "passes": []}
    for _ in range(args.passes):
        for _ in range(args.warmup):
            for launch in rows.values():
                launch()
        ms = {k: [] for k in rows}
        for _ in range(args.reps):
            for k, launch in rows.items():
                ms[k].append(qb.event_ms(launch, stream))
        out["passes"].append({k: {**qb.ms_row(v), "Mrays_s": round(n / float(np.median(v)) / 1e3, 1)}
                              for k, v in ms.items()})
    st = r.render_gbuffer_device(d_hits.data_ptr(), stream=s, stats=True)
    sq = r.trace_rays_device(d_rays.data_ptr(), n, d_qhits.data_ptr(), "nearest", stream=s, stats=True)
    stream.synchronize()
    out["hit_fraction"] = round(float((d_hits[:, 1] != -1).float().mean().item()), 4)
    out["hits_equal_fraction"] = round(float((d_hits == d_qhits).all(dim=1).float().mean().item()), 6)
    out["nodes_per_ray"] = round(st.nodes_visited / n, 3)
    out["prims_per_ray"] = round(st.prims_tested / n, 3)
    out["trace_rays_nodes_per_ray"] = round(sq.nodes_visited / n, 3)
    out["stats_launch_ms"] = {"gbuffer_hits": round(float(st.ms), 4), "trace_rays": round(float(sq.ms), 4)}
    print(json.dumps(out))
    r.close()


if __name__ == "__main__":
    main()
