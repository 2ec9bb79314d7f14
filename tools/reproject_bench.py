#!/usr/bin/env python3
"""Layer-reprojection time (rt_reproject_layer) on a config's scene, beside the
calls a viewer runs around it.

    python tools/reproject_bench.py [--config c3] [--reps 10] [--warmup 2] [--rounds 3]
                                    [--torch-reps 3]

Timed with HIP events on one stream, --rounds times alternating over the cases,
each case the median of --reps launches after --warmup; a case's figure is the
median of its rounds' medians:
  reproject    rt_reproject_layer alone, channels 1 (the frame's 4-ray AO layer) and
               4 (a seeded random float4 layer), with the camera at rest (the
               history is the same camera's) and moving (the history is a camera's
               shifted by 0.004 in x), and with no history (the copy)
  beside it    rt_render_gbuffer (hits, normals), rt_render_ao (4 rays),
               rt_filter_layer (3 passes) and rt_apply_layer, in the same process
  chain        the whole moving-camera frame: rt_set_pose, G-buffer, 4-ray AO with
               salt = the frame number, rt_reproject_layer against the previous
               frame's buffers, rt_filter_layer on the accumulated layer,
               rt_apply_layer; the two sets of buffers swap each frame
  torch        the same output computed by a torch program on the same GPU (index
               arithmetic and gathers); whether its words agree is reported, not
               required
The AO radius is 2 x the scene's mean sphere radius (tools/ao_bench.py's short one).
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

PARAMS = dict(max_count=32.0, depth_tol=0.05)
SHIFT = 0.004


def torch_reproject(torch, cur, hits, pose, K, hist, max_count, depth_tol):
    """rt_reproject_layer's specification in torch operations: cur (H, W, C), hits
    (H, W, 2) int32, pose (16,) and K (9,) python floats of the current camera;
    hist = (hits, layer (H, W, C), count (H, W), pose, K) -> (out, count)."""
    H, W, _ = cur.shape
    f32 = torch.float32
    ys, xs = torch.meshgrid(torch.arange(H, device=cur.device, dtype=f32), torch.arange(W, device=cur.device, dtype=f32),
                            indexing="ij")
    dx, dy = (xs - K[2]) / K[0], (ys - K[5]) / K[4]
    wv = [pose[k] * dx + pose[4 + k] * dy + pose[8 + k] * 1.0 for k in range(3)]
    ln = torch.sqrt(wv[0] * wv[0] + wv[1] * wv[1] + wv[2] * wv[2])
    t = hits[..., 0].contiguous().view(f32)
    s = hits[..., 1]
    h_hits, h_layer, h_count, hp, hk = hist
    q = [(pose[12 + k] + t * (wv[k] / ln)) - hp[12 + k] for k in range(3)]
    cx, cy, cz = ((hp[4 * k] * q[0] + hp[4 * k + 1] * q[1]) + hp[4 * k + 2] * q[2] for k in range(3))
    dist = torch.sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2])
    live = (s != -1) & (cz > 0)
    u, v = (cx / cz) * hk[0] + hk[2], (cy / cz) * hk[4] + hk[5]
    u0, v0 = torch.floor(u), torch.floor(v)
    a, b = u - u0, v - v0
    ht = h_hits[..., 0].contiguous().view(f32).reshape(-1)
    hs = h_hits[..., 1].reshape(-1)
    hl, hc = h_layer.reshape(H * W, -1), h_count.reshape(-1)
    zero = torch.zeros_like(t)
    sw, sc, sv = zero, zero, torch.zeros_like(cur)
    for j in range(2):
        fv = v0 + float(j)
        for i in range(2):
            fu = u0 + float(i)
            on = live & (fu >= 0) & (fu <= W - 1) & (fv >= 0) & (fv <= H - 1)
            idx = torch.where(on, fv, zero).long() * W + torch.where(on, fu, zero).long()
            tq = ht[idx]
            on = on & (hs[idx] == s) & ((dist - tq).abs() <= depth_tol * tq)
            w = (a if i else 1.0 - a) * (b if j else 1.0 - b)
            sw = sw + torch.where(on, w, zero)
            sv = sv + torch.where(on[..., None], w[..., None] * hl[idx], torch.zeros_like(cur))
            sc = sc + torch.where(on, w * hc[idx], zero)
    took = live & (sw > 0)
    n = torch.fmin(sc / sw + 1.0, torch.full_like(sw, max_count))   # fminf: a NaN count restarts at the cap
    hv = sv / sw[..., None]
    out = torch.where(took[..., None], hv + (cur - hv) * (1.0 / n)[..., None], cur)
    return out, torch.where(took, n, torch.ones_like(n))


class FrameSet:
    """One camera's {hits, normals, 4-ray AO layer, float4 layer} and, for when it
    serves as a history, counts and the accumulated layers of a first call."""

    def __init__(self, torch, r, pose, K, radius, salt, stream):
        H, W = r.height, r.width
        dev = torch.device("cuda")
        self.pose, self.K = np.asarray(pose, np.float32).reshape(16), np.asarray(K, np.float32).reshape(9)
        self.hits = torch.empty((H, W, 2), dtype=torch.int32, device=dev)
        self.nrm = torch.empty((H, W, 4), dtype=torch.float32, device=dev)
        self.ao = torch.empty((H, W), dtype=torch.float32, device=dev)
        self.v4 = torch.from_numpy(np.random.default_rng(31 + salt).random((H, W, 4)).astype(np.float32)).to(dev)
        self.acc1, self.acc4 = torch.empty_like(self.ao), torch.empty_like(self.v4)
        self.count = torch.empty_like(self.ao)
        torch.cuda.synchronize()
        r.setPosition(self.pose)
        r.render_gbuffer_device(self.hits.data_ptr(), self.nrm.data_ptr(), stream=stream)
        r.render_ao_device(4, radius, self.ao.data_ptr(), salt=salt, stream=stream)

    def history(self, channels):
        layer = self.acc1 if channels == 1 else self.acc4
        return dict(hits=self.hits.data_ptr(), layer=layer.data_ptr(), count=self.count.data_ptr(), pose=self.pose,
                    K=self.K)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--torch-reps", type=int, default=3)
    args = ap.parse_args()
    import torch

    if rt.device_count() == 0:
        sys.exit("reproject_bench: no HIP device visible (times are measured on the GPU only)")
    r, sp, info, pose0 = qb.scene_renderer(args.config)
    W, H = r.width, r.height
    radius = 2.0 * float(sp[:, 3].astype(np.float64).mean())
    stream = torch.cuda.Stream()
    s_ptr = stream.cuda_stream
    K = r.camera()[1].reshape(9)
    pose0 = np.asarray(pose0, np.float32)
    pose1 = pose0.copy()
    pose1[3, 0] += np.float32(SHIFT)
    # the history (pose0) carries the mean of a few frames: accumulate it once, at rest
    prev = FrameSet(torch, r, pose0, K, radius, 0, s_ptr)
    rest = FrameSet(torch, r, pose0, K, radius, 1, s_ptr)
    moved = FrameSet(torch, r, pose1, K, radius, 1, s_ptr)
    for channels, src, dst in ((1, prev.ao, prev.acc1), (4, prev.v4, prev.acc4)):
        r.reproject_layer_device(prev.hits.data_ptr(), src.data_ptr(), dst.data_ptr(), prev.count.data_ptr(), None,
                                 channels, stream=s_ptr, **PARAMS)
    out1, out4, cnt = torch.empty_like(prev.ao), torch.empty_like(prev.v4), torch.empty_like(prev.ao)
    d_flt = torch.empty_like(prev.ao)
    stream.synchronize()
    r.synchronize()

    def reproject(cur, hist, channels):
        src, dst = (cur.ao, out1) if channels == 1 else (cur.v4, out4)
        r.reproject_layer_device(cur.hits.data_ptr(), src.data_ptr(), dst.data_ptr(), cnt.data_ptr(),
                                 None if hist is None else hist.history(channels), channels, stream=s_ptr, **PARAMS)

    def at(cur, fn):
        def run():
            r.setPosition(cur.pose)
            fn()
        return run

    # the moving-camera chain: two buffer sets that swap, the camera alternating between the two poses
    sets = [prev, moved]
    state = {"k": 0}

    def chain():
        k = state["k"] = state["k"] + 1
        cur, hist = sets[k & 1], sets[(k & 1) ^ 1]
        r.setPosition(cur.pose)
        r.render_gbuffer_device(cur.hits.data_ptr(), cur.nrm.data_ptr(), stream=s_ptr)
        r.render_ao_device(4, radius, cur.ao.data_ptr(), salt=k, stream=s_ptr)
        r.reproject_layer_device(cur.hits.data_ptr(), cur.ao.data_ptr(), cur.acc1.data_ptr(), cur.count.data_ptr(),
                                 hist.history(1), 1, stream=s_ptr, **PARAMS)
        r.filter_layer_device(cur.acc1.data_ptr(), d_flt.data_ptr(), cur.hits.data_ptr(), cur.nrm.data_ptr(), 3, 1,
                              stream=s_ptr)
        r.apply_layer_device(d_flt.data_ptr(), 0.25, stream=s_ptr)

    r.render(stream=s_ptr)      # a frame in the internal framebuffer for the multiply
    cases = {}
    for c in (1, 4):
        cases[f"reproject_c{c}_rest"] = at(rest, lambda c=c: reproject(rest, prev, c))
        cases[f"reproject_c{c}_moving"] = at(moved, lambda c=c: reproject(moved, prev, c))
        cases[f"reproject_c{c}_no_history"] = at(moved, lambda c=c: reproject(moved, None, c))
    scratch = FrameSet(torch, r, pose1, K, radius, 2, s_ptr)    # what the single steps write
    cases.update(
        gbuffer=at(scratch, lambda: r.render_gbuffer_device(scratch.hits.data_ptr(), scratch.nrm.data_ptr(),
                                                            stream=s_ptr)),
        ao4=at(scratch, lambda: r.render_ao_device(4, radius, scratch.ao.data_ptr(), stream=s_ptr)),
        filter3=at(scratch, lambda: r.filter_layer_device(scratch.ao.data_ptr(), d_flt.data_ptr(),
                                                          scratch.hits.data_ptr(), scratch.nrm.data_ptr(), 3, 1,
                                                          stream=s_ptr)),
        apply=at(scratch, lambda: r.apply_layer_device(d_flt.data_ptr(), 0.25, stream=s_ptr)),
        frame=at(scratch, lambda: r.render(stream=s_ptr)))
    rounds = {k: [] for k in list(cases) + ["chain_moving"]}
    for _ in range(args.rounds):
        for name, fn in cases.items():
            for _ in range(args.warmup):
                fn()
            rounds[name].append(qb.ms_row([qb.event_ms(fn, stream) for _ in range(args.reps)]))
    # the chain last: it overwrites prev's and moved's accumulated layers
    for _ in range(args.rounds):
        for _ in range(args.warmup):
            chain()
        rounds["chain_moving"].append(qb.ms_row([qb.event_ms(chain, stream) for _ in range(args.reps)]))
    stream.synchronize()
    out = {"config": args.config, "width": W, "height": H, "reps": args.reps, "warmup": args.warmup,
           "rounds": args.rounds, "scene": qb.scene_summary(info), "ao_radius": round(radius, 6),
           "camera_shift_x": SHIFT, "params": PARAMS, "cases": {}}
    med = {}
    for name, rows in rounds.items():
        med[name] = float(np.median([x["ms_median"] for x in rows]))
        out["cases"][name] = {"ms": round(med[name], 4), "rounds": rows}
    steps = med["gbuffer"] + med["ao4"] + med["reproject_c1_moving"] + med["filter3"] + med["apply"]
    out["chain"] = {"chain_moving_ms": round(med["chain_moving"], 4), "sum_of_steps_ms": round(steps, 4),
                    "reproject_share_of_chain": round(med["reproject_c1_moving"] / med["chain_moving"], 4),
                    "chain_over_frame": round(med["chain_moving"] / med["frame"], 3)}

    # the torch program: the same output from index arithmetic and four gathers
    out["torch"] = {}
    r.setPosition(moved.pose)
    # (the chain rewrote the accumulated layers: whatever they hold now is the history of both programs)
    for channels in (1, 4):
        cur = moved.ao[..., None] if channels == 1 else moved.v4
        hist = (prev.hits, (prev.acc1[..., None] if channels == 1 else prev.acc4), prev.count,
                [float(x) for x in prev.pose], [float(x) for x in prev.K])
        a = (torch, cur, moved.hits, [float(x) for x in moved.pose], [float(x) for x in moved.K], hist,
             PARAMS["max_count"], PARAMS["depth_tol"])
        with torch.cuda.stream(stream):
            ref, ref_n = torch_reproject(*a)      # warm
            ms = [qb.event_ms(lambda: torch_reproject(*a), stream) for _ in range(args.torch_reps)]
            reproject(moved, prev, channels)
        stream.synchronize()
        r.synchronize()
        got = out1[..., None] if channels == 1 else out4
        name = f"reproject_c{channels}_moving"
        out["torch"][name] = {**qb.ms_row(ms, 3), "torch_over_reproject": round(float(np.median(ms)) / med[name], 1),
                              "elements": int(got.numel()) + int(cnt.numel()),
                              "same_bits": int((got.view(torch.int32) == ref.view(torch.int32)).sum().item())
                              + int((cnt.view(torch.int32) == ref_n.view(torch.int32)).sum().item()),
                              "max_abs_diff": float((got - ref).abs().max().item()),
                              "pixels_with_history": int((cnt > 1).sum().item())}
    out["not_measured"] = ("other scenes, sizes and camera motions; image quality on this scene; a per-counter "
                           "profile of the kernel")
    print(json.dumps(out))
    r.close()


if __name__ == "__main__":
    main()
