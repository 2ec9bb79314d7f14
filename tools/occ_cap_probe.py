#!/usr/bin/env python3
"""The runs behind the occluder lists' cap C and mean threshold T (DESIGN.md
5.1 round 7): per config, in one process, a renderer that walks and renderers
on lists at caps 16 / 32 / 64 with the scene rule lifted (the test hooks
RT_TEST_OCC_CAP and RT_TEST_OCC_MEAN), 5 interleaved rounds of plain frames.

    python tools/occ_cap_probe.py c5d,c5,c3
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import raytracingstudy_amd as rt
from raytracingstudy_amd import _lib
from raytracingstudy_amd.camera import scene_pose
import torch  # noqa: E402

_lib.test_flags = _lib.RT_FLAG_TEST_HOOKS
stream = torch.cuda.Stream()
for name in sys.argv[1].split(","):
    cfg = rt.CONFIGS[name]
    sp, al = rt.configs.scene_spheres(cfg, rt.SEED)
    rs = {}
    for key, env in (("walk", None), ("cap16", "16"), ("cap32", "32"), ("cap64", "64")):
        if env:
            os.environ["RT_TEST_OCC_MEAN"] = "1e9"
            os.environ["RT_TEST_OCC_CAP"] = env
        r = rt.KernelRenderer(cfg.width, cfg.height, mode="scene", spp=cfg.spp, occluders=env is not None)
        r.resize(cfg.width, cfg.height); r.setPosition(scene_pose())
        r.set_scene(sp, al, max_depth=cfg.max_depth, leaf_capacity=cfg.leaf_capacity)
        r.render(stats=True)
        r.render()
        rs[key] = r
    times = {k: [] for k in rs}
    for _ in range(5):
        for k, r in rs.items():
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record(stream); r.render(None, stream.cuda_stream); e1.record(stream); e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    ref = rs["walk"].readback()
    out = {}
    for k, r in rs.items():
        info = r.scene_info()
        out[k] = {"ms_median": round(float(np.median(times[k])), 3), "ms_min": round(min(times[k]), 3),
                  "on": info["occluder_lists_on"], "entries": info["occluder_entries"],
                  "build_ms": round(info["occluder_build_ms"], 3),
                  "same_image": bool(np.array_equal(r.readback(), ref))}
        r.close()
    print(name, json.dumps(out), flush=True)
