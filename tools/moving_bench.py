#!/usr/bin/env python3
"""Time plain frames of a config with a NEW camera pose every frame: what a
Displayer session pays.  bench.py renders one fixed pose, so everything keyed
on the pose (the camera-relative and image-plane screen records) is made once
and falls out of its headline; here every frame remakes it, and the
screen-space bins, which are never keyed on the pose, cost the same as there.

    python tools/moving_bench.py [--config c3] [--frames 60] [--fixed]
    RT_AMD_LIB=abl/librt_A.so python tools/moving_bench.py    # another build

The camera orbits the scene centre slowly (0.2 degrees a frame at the
SURVEY 8d distance, inside the occluder lists' camera gate).  Per frame: HIP
events around rt_render on one stream, the frames queued back to back.
--fixed: the same pose every frame, for the difference.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import raytracingstudy_amd as rt  # noqa: E402
from raytracingstudy_amd.camera import display_pose  # noqa: E402


def orbit_pose(k: int, step_deg: float = 0.2) -> np.ndarray:
    """Frame k's pose: on the circle of radius 1.56 about (0.64, 0.64, 0.64) in
    the y = 0.64 plane, facing the centre; k = 0 is scene_pose's position."""
    a = math.radians(step_deg * k)
    pos = (0.64 + 1.56 * math.sin(a), 0.64, 0.64 + 1.56 * math.cos(a))
    return display_pose(pos, yaw_deg=step_deg * k, pitch_deg=0.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--fixed", action="store_true")
    ap.add_argument("--no-bins", action="store_true")
    args = ap.parse_args()
    import torch
    cfg = rt.CONFIGS[args.config]
    sp, al = rt.configs.scene_spheres(cfg, rt.SEED)
    kw = {"bins": False} if args.no_bins else {}
    r = rt.KernelRenderer(cfg.width, cfg.height, mode="scene", spp=cfg.spp, **kw)
    r.resize(cfg.width, cfg.height)
    r.setPosition(orbit_pose(0))
    r.set_scene(sp, al, max_depth=cfg.max_depth, leaf_capacity=cfg.leaf_capacity)
    stream = torch.cuda.Stream()
    n = args.warmup + args.frames
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
    ev[0].record(stream)
    for k in range(n):
        r.setPosition(orbit_pose(0 if args.fixed else k))
        r.render(None, stream.cuda_stream)
        ev[k + 1].record(stream)
    ev[n].synchronize()
    ms = [ev[k].elapsed_time(ev[k + 1]) for k in range(args.warmup, n)]
    out = {"config": args.config, "pose": "fixed" if args.fixed else "moving", "frames": args.frames,
           "ms_median": round(float(np.median(ms)), 4), "ms_min": round(float(np.min(ms)), 4),
           "ms_max": round(float(np.max(ms)), 4)}
    if hasattr(r, "bin_info") and hasattr(r._lib, "rt_get_bin_info"):
        bi = r.bin_info()
        out["bins"] = {k: bi[k] for k in ("reason", "entries", "non_empty_bins", "longest",
                                           "overflowed_bins", "wide")}
    import hashlib
    out["last_image_sha1"] = hashlib.sha1(r.readback().tobytes()).hexdigest()[:12]
    print(json.dumps(out))
    r.close()


if __name__ == "__main__":
    main()
