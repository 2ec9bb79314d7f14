"""What query_bench.py, overlap_bench.py, closest_bench.py and gbuffer_bench.py
share: a config's scene in a renderer, a HIP-event timer, the rows and the scene
summary of their JSON lines, and their ray and probe sets.  Each tool keeps its
torch baseline, its case table, its order of launches and its JSON assembly.
"""
from __future__ import annotations

import numpy as np

import raytracingstudy_amd as rt
from raytracingstudy_amd.camera import scene_pose


def scene_renderer(config: str):
    """A renderer of the config's size with the config's scene at scene_pose():
    (renderer, spheres (n, 4) float32, scene info, pose)."""
    cfg = rt.CONFIGS[config]
    sp, al = rt.configs.scene_spheres(cfg, rt.SEED)
    sp = np.ascontiguousarray(sp, np.float32)
    r = rt.KernelRenderer(cfg.width, cfg.height, mode="scene", spp=cfg.spp)
    r.resize(cfg.width, cfg.height)
    pose = scene_pose()
    r.setPosition(pose)
    info = r.set_scene(sp, al, max_depth=cfg.max_depth, leaf_capacity=cfg.leaf_capacity)
    return r, sp, info, pose


def event_ms(fn, stream) -> float:
    """The ms between two HIP events recorded on `stream` around fn()."""
    import torch
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def ms_row(ms, digits: int = 4) -> dict:
    """Median, minimum and maximum of a case's times (4 digits: a query's, 3: a torch baseline's)."""
    return {"ms_median": round(float(np.median(ms)), digits), "ms_min": round(min(ms), digits),
            "ms_max": round(max(ms), digits)}


def scene_summary(info: dict) -> dict:
    return {k: info[k] for k in ("n_spheres", "n_nodes", "n_prim_refs", "depth_reached", "cell_table_depth")}


def camera_rays(n: int, w: int, h: int, pose: np.ndarray, K: np.ndarray) -> np.ndarray:
    """Camera::getRay (include/camera.h:24-41) at pixel centres, row-major, f32."""
    f = np.float32
    i = np.arange(n, dtype=np.int64) % (w * h)
    u, v = (i % w).astype(f), (i // w).astype(f)
    dx, dy = (u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1]
    d = np.stack([pose[0, c] * dx + pose[1, c] * dy + pose[2, c] for c in range(3)], 1).astype(f)
    d /= np.sqrt((d * d).sum(1, dtype=f))[:, None]
    rays = np.zeros((n, 8), f)
    rays[:, :3] = pose[3, :3]
    rays[:, 4:7] = d
    rays[:, 7] = np.inf
    return rays


def root_box_probes(g: np.random.Generator, info: dict, n: int, radius: float) -> np.ndarray:
    """(n, 4) float32 probes: centres uniform in the scene's root box (one draw
    of (n, 3) from g), every radius `radius`."""
    lo, hi = np.array(info["root_min"], np.float32), np.array(info["root_max"], np.float32)
    probes = np.zeros((n, 4), np.float32)
    probes[:, :3] = g.uniform(lo, hi, (n, 3))
    probes[:, 3] = radius
    return probes
