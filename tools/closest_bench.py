#!/usr/bin/env python3
"""Closest-sphere query throughput (rt_query_closest) on a config's scene.

    python tools/closest_bench.py [--config c3] [--log2-probes 20] [--ks 1,16] [--rounds 10]
                                  [--warmup 2] [--torch-probes 16384] [--torch-chunk 2048]

Three probe sets, each at every k of --ks, timed with HIP events around the
launch on a stream:
  neighbours  the scene's own centres as the probes with skip_self, unbounded
              (each sphere's k nearest neighbours)
  points      2^n random points in the root box, unbounded (R = +inf)
  mean_r      the same kind of points with R = the scene's mean radius
The rounds alternate the cases, after --warmup rounds that are not recorded;
each case reports the median, the minimum and the maximum of its rounds,
probes/s from the median, the mean count and the descent's work per probe (from
one stats launch).  Beside them, what a caller does without the query: a
chunked torch distance matrix on the same GPU (the key's operations in f32, in
its order, a top-k of the keys within R), timed on --torch-probes probes of
each set in the same alternating rounds, with the ratio of the two rates and
whether the two paths answered the same (distances and counts everywhere, the
sphere indices on the rows without equal distances: top-k does not order ties
by index).  A second reference row: rt_query_overlaps on mean_r's probes.
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


def torch_closest(torch, d_sp, d_pr, k, chunk, skip_self):
    """(dist (n, k), sphere (n, k), count (n,)) from a chunked distance matrix;
    a free slot holds {the probe's radius, -1}."""
    n_s = d_sp.shape[0]
    inf = float("inf")
    dist_out, idx_out, count_out = [], [], []
    for a in range(0, d_pr.shape[0], chunk):
        p = d_pr[a:a + chunk]
        dx = p[:, None, 0] - d_sp[None, :, 0]
        dy = p[:, None, 1] - d_sp[None, :, 1]
        dz = p[:, None, 2] - d_sp[None, :, 2]
        key = torch.sqrt((dx * dx + dy * dy) + dz * dz) - d_sp[None, :, 3]
        member = key <= p[:, 3:4]
        if skip_self:
            i = torch.arange(a, min(a + p.shape[0], n_s), device=d_sp.device)
            member[i - a, i] = False
        count = member.sum(1, dtype=torch.int32).clamp(max=k)
        val, idx = torch.where(member, key, inf).topk(k, dim=1, largest=False, sorted=True)
        free = torch.arange(k, device=d_sp.device)[None, :] >= count[:, None]
        dist_out.append(torch.where(free, p[:, 3:4].expand(-1, k), val))
        idx_out.append(torch.where(free, -1, idx.to(torch.int32)))
        count_out.append(count)
    return torch.cat(dist_out), torch.cat(idx_out), torch.cat(count_out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--log2-probes", type=int, default=20)
    ap.add_argument("--ks", default="1,16")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--torch-probes", type=int, default=16384)
    ap.add_argument("--torch-chunk", type=int, default=2048)
    args = ap.parse_args()
    ks = [int(t) for t in args.ks.split(",")]
    if not all(1 <= k <= rt._lib.RT_CLOSEST_MAX for k in ks):
        sys.exit(f"closest_bench: --ks takes 1 .. {rt._lib.RT_CLOSEST_MAX}")
    import torch
    if rt.device_count() == 0:
        sys.exit("closest_bench: no HIP device visible (rates are measured on the GPU only)")
    n = 1 << args.log2_probes
    r, sp, info, _ = qb.scene_renderer(args.config)
    g = np.random.default_rng(12345)
    mean_r = float(sp[:, 3].mean())
    own = sp.copy()
    own[:, 3] = np.inf
    points = qb.root_box_probes(g, info, n, np.inf)
    balls = points.copy()  # the same centres: one draw
    balls[:, 3] = mean_r
    sets = {"neighbours": (own, True), "points": (points, False), "mean_r": (balls, False)}
    cases = [(name, k) for name in sets for k in ks]
    stream = torch.cuda.Stream()
    d_sp = torch.from_numpy(sp).cuda()
    dev = {name: torch.from_numpy(p).cuda() for name, (p, _) in sets.items()}
    n_max, k_max = max(len(p) for p, _ in sets.values()), max(ks)
    d_near = torch.empty((n_max * k_max, 2), dtype=torch.int32, device="cuda")
    d_cnt = torch.empty((n_max,), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def launch(name, k, stats=False):
        p, skip = sets[name]
        return r.query_closest_device(dev[name].data_ptr(), len(p), k, d_near.data_ptr(), d_cnt.data_ptr(),
                                      skip_self=skip, stream=stream.cuda_stream, stats=stats)

    def launch_overlap(k, stats=False):
        return r.query_overlaps_device(dev["mean_r"].data_ptr(), n, k, d_near.data_ptr(), d_cnt.data_ptr(),
                                       stream=stream.cuda_stream, stats=stats)

    ms = {c: [] for c in cases}
    tms = {c: [] for c in cases}
    oms = {k: [] for k in ks}
    tn = {name: min(args.torch_probes, len(sets[name][0])) for name in sets}
    cur = torch.cuda.current_stream()
    for rnd in range(args.warmup + args.rounds):
        for name, k in cases:
            t = qb.event_ms(lambda: launch(name, k), stream)
            tt = qb.event_ms(lambda: torch_closest(torch, d_sp, dev[name][:tn[name]], k, args.torch_chunk,
                                                   sets[name][1]), cur)
            if rnd >= args.warmup:
                ms[name, k].append(t)
                tms[name, k].append(tt)
        for k in ks:
            t = qb.event_ms(lambda: launch_overlap(k), stream)
            if rnd >= args.warmup:
                oms[k].append(t)
    out = {"config": args.config, "ks": ks, "rounds": args.rounds, "warmup": args.warmup,
           "scene": qb.scene_summary(info),
           "mean_radius": round(mean_r, 6), "cell_table_entry": "not built"}
    for name, k in cases:
        p, skip = sets[name]
        m, t_n = len(p), tn[name]
        st = launch(name, k, stats=True)
        r.synchronize()
        near = d_near[:m * k].view(m, k, 2)
        count = d_cnt[:m].clone()
        td, ti, tc = torch_closest(torch, d_sp, dev[name][:t_n], k, args.torch_chunk, skip)
        dist = near[:t_n, :, 0].contiguous().view(torch.float32)
        untied = ~((dist[:, 1:] == dist[:, :-1]) & (near[:t_n, 1:, 1] != -1)).any(dim=1)
        same = bool(torch.equal(td, dist) and torch.equal(tc, count[:t_n])
                    and torch.equal(ti[untied], near[:t_n, :, 1][untied]))
        med, tmed = float(np.median(ms[name, k])), float(np.median(tms[name, k]))
        rate, trate = m / med * 1e3, t_n / tmed * 1e3
        out[f"{name}_k{k}"] = {
            "probes": m, "k": k, "skip_self": skip, "radius": "inf" if name != "mean_r" else round(mean_r, 6),
            **qb.ms_row(ms[name, k]),
            "Mprobes_s": round(rate / 1e6, 3),
            "mean_count": round(float(count.float().mean()), 4),
            "nodes_per_probe": round(st.nodes_visited / m, 3),
            "tests_per_probe": round(st.prims_tested / m, 3),
            "stats_launch_ms": round(float(st.ms), 4),
            "torch": {"probes": t_n, "chunk": args.torch_chunk, **qb.ms_row(tms[name, k], 3),
                      "Mprobes_s": round(trate / 1e6, 4), "same_answer": same,
                      "rows_without_ties": int(untied.sum())},
            "speedup_vs_torch": round(rate / trate, 1)}
    for k in ks:
        st = launch_overlap(k, stats=True)
        r.synchronize()
        med = float(np.median(oms[k]))
        out[f"overlaps_mean_r_k{k}"] = {
            "probes": n, "k": k, **qb.ms_row(oms[k]), "Mprobes_s": round(n / med * 1e3 / 1e6, 3),
            "nodes_per_probe": round(st.nodes_visited / n, 3), "tests_per_probe": round(st.prims_tested / n, 3)}
    print(json.dumps(out))
    r.close()


if __name__ == "__main__":
    main()
