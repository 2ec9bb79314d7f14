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
from raytracingstudy_amd.camera import scene_pose  # noqa: E402
from tools.query_bench import camera_rays  # noqa: E402


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
    cfg = rt.CONFIGS[args.config]
    w, h = cfg.width, cfg.height
    n = w * h
    sp, al = rt.configs.scene_spheres(cfg, rt.SEED)
    r = rt.KernelRenderer(w, h, mode="scene", spp=cfg.spp)
    r.resize(w, h)
    pose = scene_pose()
    r.setPosition(pose)
    info = r.set_scene(sp, al, max_depth=cfg.max_depth, leaf_capacity=cfg.leaf_capacity)
    _, K = r.camera()
    stream = torch.cuda.Stream()
    d_rays = torch.from_numpy(camera_rays(n, w, h, pose, K)).cuda()
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
           "scene": {k: info[k] for k in ("n_spheres", "n_nodes", "n_prim_refs", "depth_reached",
                                          "cell_table_depth")},
           "passes": []}
    for _ in range(args.passes):
        for _ in range(args.warmup):
            for launch in rows.values():
                launch()
        ms = {k: [] for k in rows}
        for _ in range(args.reps):
            for k, launch in rows.items():
                e0 = torch.cuda.Event(enable_timing=True)
                e1 = torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                launch()
                e1.record(stream)
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1))
        out["passes"].append({k: {"ms_median": round(float(np.median(v)), 4), "ms_min": round(min(v), 4),
                                  "ms_max": round(max(v), 4),
                                  "Mrays_s": round(n / float(np.median(v)) / 1e3, 1)}
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
