"""Seeded cases for the pixel-pair frames (rt_shade.h shade_pixel_pair,
DESIGN.md 5.1 rounds 26 and 27) and their CPU model, shared by
test_pair_fuzz_cpu.py and test_gpu_pair_fuzz.py.

pair_case(seed): plain_fuzz.plain_case's distribution of scenes, cameras,
intrinsics, lights and ambient (restated here: plain_case returns what it
always did), moved to where a binned frame of 33 .. 64 spp shades two pixels a
wave pass and to that path's fallbacks at the smallest shapes: sample counts
that leave lanes invalid, frames 1 .. 17 pixels wide beside ones of up to 96,
heights from 1, per-case caps of the bins and of the occluder lists (a bin
over the cap beside a listed one, a sphere whose shadow rays walk beside a
listed one), forced tickets of 2, 4 and 8 wave tiles, the frame's dense
flag, and controls that shade no pair (no shadow rays, a camera outside the
occluder lists' gate, a ticket of one tile, forced or chosen).

model(seed, dump, oracle): plain_fuzz.model's, extended by the case's bin cap
(a bin with count > cap walks) and the dense flag.
"""
import numpy as np

import raytracingstudy_amd as rt
from raytracingstudy_amd.camera import display_pose

from bins_native import WIDE, frame_gate, rects
from bins_oracle import look_at_pose, primary_hits
from plain_fuzz import WIDE_CAP, bin_counts, oracle_scene

SEEDS = 96
# The cases are default_rng(BASE + seed).  A frame of one colour cannot be told
# from a wrong one (test_pair_fuzz_cpu.py asks that no pairable case is such a
# frame).  An empty sky of one colour is turned away from in pair_case; seed
# 64's draw is the other kind, a camera that sees nothing but the unlit side
# of one sphere, and is replaced by the draw after the last seed's.
_REDRAWN = {64: 96}
BASE = 34700
SPPS = (33, 34, 47, 48, 56, 63, 64)     # 33: one valid lane over half a wave; 63: one invalid; 64: none
MODES = ("look", "inside", "beside", "yaw", "far")
_MODE_P = (0.3, 0.2, 0.35, 0.1, 0.05)
SMALL_W = (1, 2, 3, 7, 8, 9, 15, 16, 17)      # each side of one and two bins, odd and even
BIN_CAPS = (64, 1, 2, 5, 16)            # RT_TEST_BIN_CAP (64: the product's)
OCC_CAPS = (32, 1, 2, 6)                # RT_TEST_OCC_CAP (32: the product's, one case in ten)
_OCC_P = (0.1, 0.3, 0.3, 0.3)
TICKETS = (0, 1, 2, 3, 4)               # the option field: 0 auto, k -> 1 << (k - 1) wave tiles a ticket
# A ticket of one wave tile shades no pair (rt_sched.h pair_starts), and at these
# frame sizes the auto ticket is one tile (size_wave_queue: under 16 tiles a
# wave): fields 0 and 1 are controls, one seed in eight each; the other six
# take the forced tickets of 2, 4 and 8 tiles in turn.
_TICKET_OF = (2, 3, 4, 0, 2, 3, 4, 1)
BUILT = ("on", "dense", "wide", "capacity")    # the reasons of a frame that built bins


def pair_case(seed: int) -> dict:
    g = np.random.default_rng(BASE + _REDRAWN.get(seed, seed))
    n = int(g.choice([1, 7, 50, 400, 3000], p=[0.05, 0.1, 0.25, 0.4, 0.2]))
    depth = int(g.integers(1, 9))     # (the oracle aborts on deeper trees over radii like these)
    leaf = int(g.integers(1, 17))
    ctr = g.uniform(-0.2, 1.48, (n, 3))
    target = g.uniform(0.3, 1.0, 3)
    cluster = bool(n >= 400 and g.random() < 0.5)
    if cluster:
        k = g.random(n) < 0.6
        ctr[k] = target + 0.04 * g.normal(size=(int(k.sum()), 3))
    rad = 10.0 ** g.uniform(-3.3, -0.7, n) * min(1.0, (400.0 / n) ** (1.0 / 3.0))
    sp = np.concatenate([ctr, rad[:, None]], 1).astype(np.float32)
    al = g.integers(0, 1 << 24, n, dtype=np.uint32) | np.uint32(0xFF000000)
    small = bool(g.random() < 0.3)
    w = int(g.choice(SMALL_W)) if small else int(g.integers(9, 97))
    h = int(g.integers(1, 65))
    spp = int(g.choice(SPPS))
    mode = str(g.choice(MODES, p=_MODE_P))
    zoom = 2.0 ** g.uniform(-1.0, 3.0)
    if mode == "look":
        pose = look_at_pose(g.uniform(-1.0, 2.3, 3), target)
    elif mode == "inside":
        pose = look_at_pose(g.uniform(0.1, 1.18, 3), target)
    elif mode == "beside":
        # beside one of the larger spheres, on the camera plane through its
        # centre: the sphere lies across that plane (the wide list)
        big = np.argsort(sp[:, 3])[-max(1, n // 8):]
        k = int(big[g.integers(0, len(big))])
        c, r = sp[k, :3].astype(np.float64), float(sp[k, 3])
        f = target - c
        e = np.cross(f, g.normal(size=3))
        pos = c + g.uniform(1.02, 1.5) * r * e / np.linalg.norm(e)
        pose = look_at_pose(pos, pos + f)
        zoom = 2.0 ** g.uniform(-1.0, 0.5)
    elif mode == "far":
        dist = 10.0 ** g.uniform(0.7, 2.7)     # outside the occluder lists' camera gate
        d = g.normal(size=3)
        pose = look_at_pose(target + dist * d / np.linalg.norm(d), target)
        zoom = dist / 1.5
    else:
        pose = display_pose(tuple(g.uniform(-1.0, 2.3, 3)), float(g.uniform(-180, 180)),
                            float(g.uniform(-80, 80)))
    # the camera turned half round about the x axis through the root box's
    # centre, with the scene, if it faces where the sky is one colour (the miss
    # colour follows the ray's y and z where they are positive): no frame is a
    # blank that a wrong one could not be told from
    P = np.asarray(pose, np.float64).reshape(4, 4)
    if P[2, 1] < 0.0 and P[2, 2] < 0.0:
        turn = lambda v: np.array([v[0], 1.28 - v[1], 1.28 - v[2]])
        sp[:, 1:3] = np.float32(1.28) - sp[:, 1:3]
        pose = look_at_pose(turn(P[3, :3]), turn(P[3, :3] + P[2, :3]))
    # FOV 80 over the longer side: a narrow frame is a window, not a fisheye
    # (which the bins' camera gate refuses)
    zoom *= max(w, h) / w
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
    shadows = bool(g.random() < 0.9)        # (without shadow rays a frame is not a pair instance)
    jitter = bool(g.random() < 0.75)
    ambient = float(g.uniform(0.0, 0.5))
    bin_cap = int(g.choice(BIN_CAPS))
    occ_cap = int(g.choice(OCC_CAPS, p=_OCC_P))
    ticket = _TICKET_OF[seed % len(_TICKET_OF)]
    dense = bool(g.random() < 0.125)        # RT_TEST_BIN_MEAN=0: every pair returns at its first test
    return dict(seed=seed, n=n, sp=sp, al=al, depth=depth, leaf=leaf, w=w, h=h, spp=spp, mode=mode, cluster=cluster,
                pose=np.asarray(pose, np.float32).reshape(4, 4), K=K, light=light, ambient=ambient,
                shadows=shadows, jitter=jitter, bin_cap=bin_cap, occ_cap=occ_cap, ticket=ticket,
                bin_mean=0 if dense else 1000000)


def case_env(c) -> dict:
    """The test hooks of a case (read when the renderer is made)."""
    return {"RT_TEST_BIN_MIN_SAMPLES": "0", "RT_TEST_BIN_MEAN": str(c["bin_mean"]),
            "RT_TEST_BIN_CAP": str(c["bin_cap"]), "RT_TEST_OCC_CAP": str(c["occ_cap"]),
            # the scene rule refuses no scene its lists
            "RT_TEST_OCC_MEAN": "1e9"}


def oracle_frame(s, c, **kw):
    """The oracle's (rgba8, radiance, counters) of the case; kw replaces
    render arguments (spp, shadows)."""
    a = dict(spp=c["spp"], jitter=c["jitter"], shadows=c["shadows"], light_dir=c["light"], ambient=c["ambient"])
    a.update(kw)
    return s.render(c["w"], c["h"], c["pose"], c["K"], **a)


_MODELS = {}


def model(seed, dump, orc, hits=True):
    """plain_fuzz.model for pair_case(seed): per sphere class / rectangle /
    near bound, the wide count, the per-bin counts and which bins are over the
    case's cap, the path the frame must report, the oracle's frame; with
    `hits`, the oracle's primary hits of the pixel-centre rays.
    pairable: the frame shades pixel pairs as far as the model knows it: bins
    on (the device flag clear), shadow rays, no far camera (the occluder
    lists' gate), and a forced ticket of two wave tiles or more."""
    m = _MODELS.get(seed)
    if m is None:
        c = pair_case(seed)
        s = oracle_scene(orc, c)
        cls, rect, near = rects(dump, c["sp"], c["pose"], c["K"], c["w"], c["h"])
        _, prim_idx = s.export_bfs()
        in_tree = np.zeros(c["n"], bool)
        in_tree[prim_idx] = True
        cls = np.where(in_tree, cls, 0)
        counts = bin_counts(cls, rect, c["w"], c["h"])
        wide, entries = int((cls == WIDE).sum()), int(counts.sum())
        if not frame_gate(dump, c["pose"], c["K"], c["w"], c["h"]):
            reason = "camera"
        elif entries > 6 * c["n"] + 65536:
            reason = "capacity"
        elif wide > WIDE_CAP:
            reason = "wide"
        elif entries > c["bin_mean"] * int((counts > 0).sum()):
            reason = "dense"       # (screen_bins.hip bins_decide: total > mean_max * non-empty)
        else:
            reason = "on"
        m = dict(case=c, cls=cls, rect=rect, near=near, in_tree=in_tree, counts=counts, over=counts > c["bin_cap"],
                 wide=wide, entries=entries, reason=reason, frame=oracle_frame(s, c), hits=None,
                 pairable=reason == "on" and c["shadows"] and c["mode"] != "far" and c["ticket"] >= 2)
        s.close()
        _MODELS[seed] = m
    if hits and m["hits"] is None:
        c = m["case"]
        s = oracle_scene(orc, c)
        m["hits"] = primary_hits(orc, s, c["pose"], c["K"], c["w"], c["h"], 1)
        s.close()
    return m
