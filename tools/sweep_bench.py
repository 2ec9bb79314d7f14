#!/usr/bin/env python3
"""Swept-sphere query throughput (rt_sweep_spheres) on a config's scene.

    python tools/sweep_bench.py [--config c3] [--log2-casts 22] [--reps 20] [--warmup 3]
                                [--passes 2] [--torch-casts 16384] [--torch-chunk 1024]

query_bench.py's two ray sets as the casts (coherent: the config's camera
rays; incoherent: origins just off random spheres' surfaces, random
directions), each at R = 0, R = the scene's mean radius and R = 4 x the mean
radius, timed with HIP events around the launch on a stream: the median of
--reps launches after --warmup, the whole table --passes times back to back.
Beside each line:
  walk    at R = 0, the same rays through rt_trace_rays nearest in the same
          process: the price of the box-guided descent against the walk (the
          two answer the same, which is checked)
  torch   what a caller does without the query: a chunked brute force on the
          same GPU (the test's operations in f32, torch's own rounding: no
          fused multiply-add), on --torch-casts casts of the set, with the two
          rates' ratio and how many of those casts name the same sphere.  Torch
          rounds differently, so agreement is reported, not required.
Prints one JSON line.  Needs a GPU: there is no fallback.
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
from tools.query_bench import surface_rays  # noqa: E402


def torch_sweep(torch, d_sp, d_rays, radius, chunk):
    """(t (n,), sphere (n,) int32, -1: a miss) from a chunked brute force."""
    inf = float("inf")
    t_out, i_out = [], []
    for a in range(0, d_rays.shape[0], chunk):
        r = d_rays[a:a + chunk]
        o, tmin, d, tmax = r[:, None, 0:3], r[:, None, 3], r[:, None, 4:7], r[:, None, 7]
        oc = o - d_sp[None, :, :3]
        b = (oc * d).sum(2)
        q = oc - b[:, :, None] * d
        s = d_sp[None, :, 3] + radius
        h = s * s - (q * q).sum(2)
        sq = torch.sqrt(h.clamp(min=0.0))
        near = -b - sq
        t = torch.where(near > tmin, near, -b + sq)
        ok = (h >= 0.0) & (t > tmin) & (t < tmax)
        val, idx = torch.where(ok, t, inf).min(dim=1)
        hit = val < inf
        t_out.append(torch.where(hit, val, r[:, 7]))
        i_out.append(torch.where(hit, idx.to(torch.int32), -1))
    return torch.cat(t_out), torch.cat(i_out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--log2-casts", type=int, default=22)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--torch-casts", type=int, default=16384)
    ap.add_argument("--torch-chunk", type=int, default=1024)
    args = ap.parse_args()
    import torch
    if rt.device_count() == 0:
        sys.exit("sweep_bench: no HIP device visible (rates are measured on the GPU only)")
    n = 1 << args.log2_casts
    r, sp, info, pose = qb.scene_renderer(args.config)
    _, K = r.camera()
    mean_r = float(sp[:, 3].mean())
    sets = {"coherent": qb.camera_rays(n, r.width, r.height, pose, K),
            "incoherent": surface_rays(n, sp, 12345)}
    radii = {"r0": 0.0, "mean_r": mean_r, "4x_mean_r": 4.0 * mean_r}
    stream = torch.cuda.Stream()
    cur = torch.cuda.current_stream()
    d_sp = torch.from_numpy(sp).cuda()
    d_hits = torch.empty((n, 2), dtype=torch.int32, device="cuda")
    d_walk = torch.empty((n, 2), dtype=torch.int32, device="cuda")
    t_n = min(args.torch_casts, n)
    out = {"config": args.config, "casts": n, "reps": args.reps, "warmup": args.warmup, "passes": args.passes,
           "scene": qb.scene_summary(info), "mean_radius": round(mean_r, 6), "cell_table_entry": "not built"}

    def timed(launch, reps=args.reps, on=stream):
        for _ in range(args.warmup):
            launch()
        return [qb.event_ms(launch, on) for _ in range(reps)]

    for p in range(args.passes):
        for name, rays in sets.items():
            d_rays = torch.from_numpy(rays).cuda()
            torch.cuda.synchronize()
            for rname, R in radii.items():
                def launch(stats=False):
                    return r.sweep_spheres_device(d_rays.data_ptr(), n, d_hits.data_ptr(), R,
                                                  stream=stream.cuda_stream, stats=stats)
                ms = timed(launch)
                med = float(np.median(ms))
                row = out.setdefault(f"{name}_{rname}", {"radius": round(R, 6), "passes": []})
                row["passes"].append({**qb.ms_row(ms), "Mcasts_s": round(n / med / 1e3, 1)})
                if p + 1 < args.passes:
                    continue
                st = launch(stats=True)
                r.synchronize()
                row.update({"hit_fraction": round(float((d_hits[:, 1] != -1).float().mean().item()), 4),
                            "nodes_per_cast": round(st.nodes_visited / n, 3),
                            "tests_per_cast": round(st.prims_tested / n, 3),
                            "stats_launch_ms": round(float(st.ms), 4)})
                if R == 0.0:
                    def walk():
                        r.trace_rays_device(d_rays.data_ptr(), n, d_walk.data_ptr(), "nearest",
                                            stream=stream.cuda_stream)
                    wms = timed(walk)
                    r.synchronize()
                    row["walk"] = {**qb.ms_row(wms), "Mrays_s": round(n / float(np.median(wms)) / 1e3, 1),
                                   "sweep_over_walk": round(med / float(np.median(wms)), 3),
                                   "same_answer": bool(torch.equal(d_hits, d_walk))}
                tms = timed(lambda: torch_sweep(torch, d_sp, d_rays[:t_n].view(t_n, 8), R, args.torch_chunk),
                            reps=3, on=cur)
                tt, ti = torch_sweep(torch, d_sp, d_rays[:t_n].view(t_n, 8), R, args.torch_chunk)
                torch.cuda.synchronize()
                trate = t_n / float(np.median(tms)) * 1e3
                row["torch"] = {"casts": t_n, "chunk": args.torch_chunk, **qb.ms_row(tms, 3),
                                "Mcasts_s": round(trate / 1e6, 4),
                                "same_sphere": int((ti == d_hits[:t_n, 1]).sum().item())}
                row["speedup_vs_torch"] = round(n / med * 1e3 / trate, 1)
            del d_rays
    print(json.dumps(out))
    r.close()


if __name__ == "__main__":
    main()
