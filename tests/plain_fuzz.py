"""Seeded cases for the plain-frame paths (occluder lists, screen-space bins;
DESIGN.md 5.1 rounds 7 and 10) and their CPU model, shared by
test_plain_fuzz_cpu.py and test_gpu_plain_fuzz.py.

plain_case(seed): one scene, camera and render setting.  Against the
generator's scenes the distribution widens what the two features' slack terms
carry: radii over three decades inside one scene, centres across and outside
the root box, tree depths 1..8 and leaf capacities 1..16, cameras inside the
box, beside a sphere (it straddles the camera plane) and 5..500 box sizes away,
focal lengths scaled per axis, negated, and principal points off the image.

model(seed, dump, oracle): what the frame's bins must report, from
csrc/rt_bins_math.h run on the CPU (bins_native.py) and the oracle alone.
"""
import numpy as np

import raytracingstudy_amd as rt
from raytracingstudy_amd.camera import display_pose

from bins_native import BINNED, WIDE, frame_gate, rects
from bins_oracle import look_at_pose, primary_hits

SEEDS = 64
BIN = 8            # kBinSide
BIN_CAP = 64       # kBinCap
WIDE_CAP = 32      # kBinWideCap
SPPS = (1, 2, 3, 8, 64, 65, 130)        # 65 and 130: the sorted rounds
MODES = ("look", "inside", "beside", "far", "yaw")
_MODE_P = (0.4, 0.2, 0.2, 0.1, 0.1)


def plain_case(seed: int) -> dict:
    g = np.random.default_rng(7000 + seed)
    n = int(g.choice([1, 7, 50, 400, 3000], p=[0.05, 0.1, 0.2, 0.3, 0.35]))
    depth = int(g.integers(1, 9))     # (the oracle aborts on deeper trees over radii like these)
    leaf = int(g.integers(1, 17))
    ctr = g.uniform(-0.2, 1.48, (n, 3))
    target = g.uniform(0.3, 1.0, 3)
    cluster = bool(n >= 400 and g.random() < 0.3)
    if cluster:
        # a dense cluster where the cameras look: bins over the cap beside
        # sparse ones, and light-plane discs that overlap by the hundred
        k = g.random(n) < 0.6
        ctr[k] = target + 0.04 * g.normal(size=(int(k.sum()), 3))
    rad = 10.0 ** g.uniform(-3.3, -0.7, n) * min(1.0, (400.0 / n) ** (1.0 / 3.0))
    sp = np.concatenate([ctr, rad[:, None]], 1).astype(np.float32)
    al = g.integers(0, 1 << 24, n, dtype=np.uint32) | np.uint32(0xFF000000)
    w, h = int(g.integers(9, 130)), int(g.integers(9, 100))
    spp = int(g.choice(SPPS))
    mode = str(g.choice(MODES, p=_MODE_P))
    zoom = 2.0 ** g.uniform(-1.0, 3.0)
    if mode == "look":
        pose = look_at_pose(g.uniform(-1.0, 2.3, 3), target)
    elif mode == "inside":
        pose = look_at_pose(g.uniform(0.1, 1.18, 3), target)
    elif mode == "beside":
        # beside one of the larger spheres, on the camera plane through its
        # centre, a short focal length: the sphere lies across that plane (the
        # wide list) and fills one side of the image
        big = np.argsort(sp[:, 3])[-max(1, n // 8):]
        k = int(big[g.integers(0, len(big))])
        c, r = sp[k, :3].astype(np.float64), float(sp[k, 3])
        f = target - c
        e = np.cross(f, g.normal(size=3))
        pos = c + g.uniform(1.02, 1.5) * r * e / np.linalg.norm(e)
        pose = look_at_pose(pos, pos + f)
        zoom = 2.0 ** g.uniform(-1.0, 0.5)
    elif mode == "far":
        dist = 10.0 ** g.uniform(0.7, 2.7)     # crosses the occluder lists' camera gate
        d = g.normal(size=3)
        pose = look_at_pose(target + dist * d / np.linalg.norm(d), target)
        zoom = dist / 1.5
    else:
        pose = display_pose(tuple(g.uniform(-1.0, 2.3, 3)), float(g.uniform(-180, 180)),
                            float(g.uniform(-80, 80)))
    K = np.array(rt.resize_intrinsic(w, h), np.float32).copy()
    K[0, 0] *= np.float32(zoom * 2.0 ** g.uniform(-0.5, 0.5))
    K[1, 1] *= np.float32(zoom * 2.0 ** g.uniform(-0.5, 0.5))
    if g.random() < 0.25:
        K[1, 1] = -K[1, 1]
    if g.random() < 0.3:
        K[0, 2] += np.float32(g.uniform(-0.5, 0.5) * w)
        K[1, 2] += np.float32(g.uniform(-0.5, 0.5) * h)
    if g.random() < 0.7:
        light = tuple(float(x) for x in g.normal(size=3))
    else:
        light = [0.0, 0.0, 0.0]
        light[int(g.integers(0, 3))] = float(g.choice([-1.0, 1.0]))
        light = tuple(light)
    shadows = bool(g.random() < 0.8)
    jitter = bool(g.integers(0, 2)) if spp > 1 else None
    ambient = float(g.uniform(0.0, 0.5))
    progressive = bool(g.random() < 1.0 / 6.0)
    return dict(seed=seed, n=n, sp=sp, al=al, depth=depth, leaf=leaf, w=w, h=h, spp=spp, mode=mode, cluster=cluster,
                pose=np.asarray(pose, np.float32).reshape(4, 4), K=K, light=light, ambient=ambient,
                shadows=shadows, jitter=jitter, progressive=progressive)


def oracle_scene(orc, c):
    return orc.Scene(c["sp"], c["al"], max_depth=c["depth"], leaf_capacity=c["leaf"])


def oracle_frames(s, c):
    """The oracle's frames of the case: [(rgba8, radiance, counters)], two
    for a progressive case (the running sums carried over)."""
    acc = np.zeros((c["h"], c["w"], 4), np.float32) if c["progressive"] else None
    return [s.render(c["w"], c["h"], c["pose"], c["K"], spp=c["spp"], jitter=c["jitter"],
                     shadows=c["shadows"], light_dir=c["light"], ambient=c["ambient"], frame=k, accum=acc)
            for k in range(2 if c["progressive"] else 1)]


def bin_counts(cls, rect, w, h):
    """Entries per 8x8 bin: every binned sphere counts in each bin its
    rectangle overlaps (screen_bins.hip, bins_count_kernel)."""
    nbx, nby = (w + BIN - 1) // BIN, (h + BIN - 1) // BIN
    cnt = np.zeros((nby + 1, nbx + 1), np.int64)      # a difference array
    r = rect[cls == BINNED] // BIN
    np.add.at(cnt, (r[:, 1], r[:, 0]), 1)
    np.add.at(cnt, (r[:, 3] + 1, r[:, 0]), -1)
    np.add.at(cnt, (r[:, 1], r[:, 2] + 1), -1)
    np.add.at(cnt, (r[:, 3] + 1, r[:, 2] + 1), 1)
    return cnt.cumsum(0).cumsum(1)[:nby, :nbx]


_MODELS = {}


def model(seed, dump, orc, hits=True):
    """The CPU model of a case: per sphere class / rectangle / near bound (a
    sphere in no leaf is dropped, as on the device: no walk finds it
    either), the wide count, the per-bin counts and the path the plain frame
    must report; the oracle's frames; with `hits`, the oracle's primary hits
    of the pixel-centre rays."""
    m = _MODELS.get(seed)
    if m is None:
        c = plain_case(seed)
        s = oracle_scene(orc, c)
        cls, rect, near = rects(dump, c["sp"], c["pose"], c["K"], c["w"], c["h"])
        _, prim_idx = s.export_bfs()
        in_tree = np.zeros(c["n"], bool)
        in_tree[prim_idx] = True
        cls = np.where(in_tree, cls, 0)
        counts = bin_counts(cls, rect, c["w"], c["h"])
        wide, entries = int((cls == WIDE).sum()), int(counts.sum())
        if c["progressive"] and c["spp"] < 8:
            reason = "kernel"      # progressive frames under 8 spp run the block-tile queue: no bins
        elif not frame_gate(dump, c["pose"], c["K"], c["w"], c["h"]):
            reason = "camera"
        elif entries > 6 * c["n"] + 65536:
            reason = "capacity"    # (the first frame's entry buffer, rt_bins_host.cpp screen_bins)
        elif wide > WIDE_CAP:
            reason = "wide"
        else:
            reason = "on"
        m = dict(case=c, cls=cls, rect=rect, near=near, in_tree=in_tree, counts=counts, wide=wide,
                 entries=entries, reason=reason, frames=oracle_frames(s, c), hits=None)
        s.close()
        _MODELS[seed] = m
    if hits and m["hits"] is None:
        c = m["case"]
        s = oracle_scene(orc, c)
        m["hits"] = primary_hits(orc, s, c["pose"], c["K"], c["w"], c["h"], 1)
        s.close()
    return m
