#!/usr/bin/env python3
"""Sphere-overlap query throughput (rt_query_overlaps) on a config's scene.

    python tools/overlap_bench.py [--config c3] [--log2-probes 20] [--k 16] [--rounds 10]
                                  [--warmup 2] [--torch-probes 16384] [--torch-chunk 2048]

Three probe sets, timed with HIP events around the launch on a stream:
  contacts  the scene's own spheres as the probes with skip_self (all contacts
            of the scene)
  points    2^k random points in the root box (radius 0: containment)
  mean_r    2^k probes at random points with the scene's mean radius
The rounds alternate the cases (contacts, points, mean_r, then again), after
--warmup rounds that are not recorded; each case reports the median, the
minimum and the maximum of its rounds, probes/s from the median, the mean set
size and the descent's work per probe (from one stats launch).
Beside them, what a caller does without the query: a chunked torch distance
matrix on the same GPU (the same f32 predicate, the k smallest indices by a
top-k over masked indices, the count by a sum), timed on --torch-probes probes
of each set in the same alternating rounds and reported as probes/s, with the
ratio of the two rates.  Prints one JSON line.  Needs a GPU: there is no fallback.
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


def torch_overlaps(torch, d_sp, d_pr, k, chunk, skip_self):
    """The k smallest touching sphere indices and the set size per probe, from a
    chunked distance matrix: the predicate's operations in f32, in its order."""
    n_s = d_sp.shape[0]
    ar = torch.arange(n_s, device=d_sp.device, dtype=torch.int32)
    big = torch.iinfo(torch.int32).max
    idx_out, total_out = [], []
    for a in range(0, d_pr.shape[0], chunk):
        p = d_pr[a:a + chunk]
        dx = p[:, None, 0] - d_sp[None, :, 0]
        dy = p[:, None, 1] - d_sp[None, :, 1]
        dz = p[:, None, 2] - d_sp[None, :, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        s = p[:, None, 3] + d_sp[None, :, 3]
        hit = d2 <= s * s
        if skip_self:
            i = torch.arange(a, min(a + p.shape[0], n_s), device=d_sp.device)
            hit[i - a, i] = False
        total_out.append(hit.sum(1, dtype=torch.int32))
        idx_out.append(torch.where(hit, ar[None, :], big).topk(k, dim=1, largest=False, sorted=True).values)
    return torch.cat(idx_out), torch.cat(total_out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--log2-probes", type=int, default=20)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--torch-probes", type=int, default=16384)
    ap.add_argument("--torch-chunk", type=int, default=2048)
    args = ap.parse_args()
    if not 1 <= args.k <= rt._lib.RT_OVERLAP_MAX:
        sys.exit(f"overlap_bench: --k takes 1 .. {rt._lib.RT_OVERLAP_MAX}")
    import torch
    if rt.device_count() == 0:
        sys.exit("overlap_bench: no HIP device visible (rates are measured on the GPU only)")
    k = args.k
    n = 1 << args.log2_probes
    r, sp, info, _ = qb.scene_renderer(args.config)
    g = np.random.default_rng(12345)
    mean_r = float(sp[:, 3].mean())
    points = qb.root_box_probes(g, info, n, 0.0)
    balls = qb.root_box_probes(g, info, n, mean_r)  # a second draw: other centres than points'
    cases = {"contacts": (sp, True), "points": (points, False), "mean_r": (balls, False)}
    stream = torch.cuda.Stream()
    d_sp = torch.from_numpy(sp).cuda()
    dev = {name: torch.from_numpy(p).cuda() for name, (p, _) in cases.items()}
    n_max = max(len(p) for p, _ in cases.values())
    d_idx = torch.empty((n_max, k), dtype=torch.int32, device="cuda")
    d_cnt = torch.empty((n_max,), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def launch(name, stats=False):
        p, skip = cases[name]
        return r.query_overlaps_device(dev[name].data_ptr(), len(p), k, d_idx.data_ptr(), d_cnt.data_ptr(),
                                       skip_self=skip, stream=stream.cuda_stream, stats=stats)

    ms = {name: [] for name in cases}
    tms = {name: [] for name in cases}
    tn = {name: min(args.torch_probes, len(cases[name][0])) for name in cases}
    cur = torch.cuda.current_stream()
    for rnd in range(args.warmup + args.rounds):
        for name in cases:
            t = qb.event_ms(lambda: launch(name), stream)
            tt = qb.event_ms(lambda: torch_overlaps(torch, d_sp, dev[name][:tn[name]], k, args.torch_chunk,
                                                    cases[name][1]), cur)
            if rnd >= args.warmup:
                ms[name].append(t)
                tms[name].append(tt)
    out = {"config": args.config, "k": k, "rounds": args.rounds, "warmup": args.warmup,
           "scene": qb.scene_summary(info),
           "mean_radius": round(mean_r, 6), "cell_table_entry": "not built"}
    for name, (p, skip) in cases.items():
        m = len(p)
        st = launch(name, stats=True)
        r.synchronize()
        words = d_cnt[:m].cpu().numpy().view(np.uint32)
        # the two paths agree on the probes the baseline ran
        ti, tt = torch_overlaps(torch, d_sp, dev[name][:tn[name]], k, args.torch_chunk, skip)
        same = bool(torch.equal(torch.where(ti == torch.iinfo(torch.int32).max, -1, ti), d_idx[:tn[name]])
                    and torch.equal(torch.clamp(tt, max=k), (d_cnt[:tn[name]] & 0x7FFFFFFF)))
        med, tmed = float(np.median(ms[name])), float(np.median(tms[name]))
        rate, trate = m / med * 1e3, tn[name] / tmed * 1e3
        out[name] = {
            "probes": m, "skip_self": skip, **qb.ms_row(ms[name]),
            "Mprobes_s": round(rate / 1e6, 3),
            "mean_count": round(float((words & 0x7FFFFFFF).mean()), 4),
            "more_fraction": round(float((words >> 31).mean()), 6),
            "nodes_per_probe": round(st.nodes_visited / m, 3),
            "prims_per_probe": round(st.prims_tested / m, 3),
            "stats_launch_ms": round(float(st.ms), 4),
            "torch": {"probes": tn[name], "chunk": args.torch_chunk, **qb.ms_row(tms[name], 3),
                      "Mprobes_s": round(trate / 1e6, 4), "same_answer": same},
            "speedup_vs_torch": round(rate / trate, 1)}
    print(json.dumps(out))
    r.close()


if __name__ == "__main__":
    main()
