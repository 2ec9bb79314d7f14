"""Seeded cases for the query kernels (rt_trace_rays, rt_trace_rays_multi,
rt_query_overlaps, rt_render_gbuffer and the host one-shots; DESIGN.md 5.7 to
5.11) and their expectations, shared by test_query_fuzz_cpu.py and
test_gpu_query_fuzz.py.

query_case(seed): plain_fuzz.plain_case(seed)'s scene, tree, camera, intrinsic
and frame size (a grown, non-cubic root box; radii over three decades; leaf
capacities 1..16, depths 1..8, root-is-leaf trees; cameras inside, beside and
far from the cloud; negated focal lengths, principal points off the image),
with 520 rays and 520 probes made for that scene's own box.

model(seed, oracle): what the queries must answer, from the references alone:
oracle.Scene.trace (nearest / any, with per-ray counters), multihit_ref's
brute force (multi), overlap_ref's brute force (overlaps), gbuffer_ref over
the oracle (G-buffer).  Computed once per seed and kept.
"""
import numpy as np

import gbuffer_ref
import multihit_ref as mr
import overlap_ref as ov
from plain_fuzz import SEEDS, oracle_scene, plain_case     # noqa: F401  (SEEDS: for the tests)

NO_HIT = 0xFFFFFFFF
INF = np.float32(np.inf)
# rays, in this order; the bad rays are last so that rays[:N_ORACLE] is what the oracle is given
N_SURFACE, N_AIMED, N_RANDOM, N_AXIS, N_WITHIN, N_BAD_RAYS = 192, 128, 64, 64, 64, 8
N_ORACLE = N_SURFACE + N_AIMED + N_RANDOM + N_AXIS + N_WITHIN
N_RAYS = N_ORACLE + N_BAD_RAYS
# probes, in this order
N_OWN, N_INSIDE, N_POINTS, N_SMALL, N_LARGE, N_FAR, N_BAD_PROBES = 192, 64, 64, 128, 32, 32, 8
N_PROBES = N_OWN + N_INSIDE + N_POINTS + N_SMALL + N_LARGE + N_FAR + N_BAD_PROBES
BAD_PROBES = slice(N_PROBES - N_BAD_PROBES, N_PROBES)


def _unit(g, n):
    d = g.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def scene_box(sp):
    """(lo, hi) float64: the configured cube [0, 1.28]^3 grown to hold every sphere."""
    c, r = sp[:, :3].astype(np.float64), sp[:, 3:4].astype(np.float64)
    return np.minimum(0.0, (c - r).min(axis=0)), np.maximum(1.28, (c + r).max(axis=0))


def _on(g, sp, n, f):
    """n points at c + f * r * unit of random spheres (float64)."""
    k = g.integers(0, len(sp), n)
    return sp[k, :3].astype(np.float64) + f * sp[k, 3:4].astype(np.float64) * _unit(g, n)


def _rays(sp, lo, hi, g):
    S = hi - lo
    rays = np.zeros((N_RAYS, 8), np.float32)
    at = 0
    # origins just off random spheres' surfaces, random directions, a short window
    s = rays[at:at + N_SURFACE]
    s[:, :3] = _on(g, sp, N_SURFACE, 1.001)
    s[:, 3] = 1e-5
    s[:, 4:7] = _unit(g, N_SURFACE)
    s[:, 7] = 0.5
    at += N_SURFACE
    # from around the box, half a box size out on every side, at a point inside a random sphere
    o = g.uniform(lo - 0.5 * S, hi + 0.5 * S, (N_AIMED, 3))
    aim = _on(g, sp, N_AIMED, 0.7) - o
    rays[at:at + N_AIMED, :3] = o
    rays[at:at + N_AIMED, 4:7] = aim / np.linalg.norm(aim, axis=1, keepdims=True)
    rays[at:at + N_AIMED, 7] = INF
    at += N_AIMED
    # from around the box in random directions
    rays[at:at + N_RANDOM, :3] = g.uniform(lo - 0.5 * S, hi + 0.5 * S, (N_RANDOM, 3))
    rays[at:at + N_RANDOM, 4:7] = _unit(g, N_RANDOM)
    rays[at:at + N_RANDOM, 7] = INF
    at += N_RANDOM
    # axis-parallel through a point inside a random sphere, from 1.5 box sizes back; 30% with a
    # second component equal to the first (a diagonal of a coordinate plane, `dir` not unit)
    through = _on(g, sp, N_AXIS, 0.3)
    d = np.zeros((N_AXIS, 3))
    axis = g.integers(0, 3, N_AXIS)
    sign = g.choice([-1.0, 1.0], N_AXIS)
    second = g.random(N_AXIS) < 0.3
    other = (axis + g.integers(1, 3, N_AXIS)) % 3
    d[np.arange(N_AXIS), axis] = sign
    d[second, other[second]] = sign[second]
    rays[at:at + N_AXIS, :3] = through - 1.5 * S.max() * d
    rays[at:at + N_AXIS, 4:7] = d
    rays[at:at + N_AXIS, 7] = INF
    at += N_AXIS
    # origins inside a random sphere: its far root
    rays[at:at + N_WITHIN, :3] = _on(g, sp, N_WITHIN, 0.5)
    rays[at:at + N_WITHIN, 4:7] = _unit(g, N_WITHIN)
    rays[at:at + N_WITHIN, 7] = INF
    at += N_WITHIN
    # bad rays: ordinary ones with one component replaced, in x, y and z; some with a finite tmax
    b = rays[at:]
    b[:, :3] = g.uniform(lo, hi, (N_BAD_RAYS, 3))
    b[:, 4:7] = _unit(g, N_BAD_RAYS)
    b[:, 7] = (INF, 2.0, INF, INF, 2.0, 0.75, INF, 2.0)
    for i, (col, v) in enumerate(((0, np.nan), (1, np.inf), (2, -np.inf), (4, np.nan), (5, np.inf),
                                  (6, np.nan), (4, -np.inf), (2, np.nan))):
        b[i, col] = v
    return rays


def _probes(sp, lo, hi, g):
    S = hi - lo
    n = len(sp)
    pr = np.zeros((N_PROBES, 4), np.float32)
    at = 0
    pr[:N_OWN] = sp[np.arange(N_OWN) % n]             # the scene's own first spheres
    at += N_OWN
    pr[at:at + N_INSIDE, :3] = _on(g, sp, N_INSIDE, 0.5)
    at += N_INSIDE
    pr[at:at + N_POINTS, :3] = g.uniform(lo, hi, (N_POINTS, 3))
    at += N_POINTS
    pr[at:at + N_SMALL, :3] = g.uniform(lo, hi, (N_SMALL, 3))
    pr[at:at + N_SMALL, 3] = 10.0 ** g.uniform(-3.3, -0.7, N_SMALL)
    at += N_SMALL
    pr[at:at + N_LARGE, :3] = g.uniform(lo, hi, (N_LARGE, 3))
    pr[at:at + N_LARGE, 3] = g.uniform(0.2, 0.5, N_LARGE) * S.max()
    at += N_LARGE
    pr[at:at + N_FAR, :3] = hi + g.uniform(1.0, 2.0, (N_FAR, 3)) * S
    pr[at:at + N_FAR, 3] = g.uniform(0.0, 0.3, N_FAR)
    at += N_FAR
    # bad probes: an ordinary one (it holds sphere 0's centre) with one component replaced
    b = pr[at:]
    b[:] = (*sp[0, :3], 0.1)
    for i, (col, v) in enumerate(((0, np.nan), (1, np.inf), (2, -np.inf), (3, np.nan), (3, np.inf),
                                  (3, -np.inf), (3, -1e-6), (3, -1.0))):
        b[i, col] = v
    return pr


def query_case(seed: int) -> dict:
    """plain_case(seed) with `rays` (520, 8) in rt_ray layout, `probes` (520, 4)
    in rt_probe layout (both read-only) and the box they were made for."""
    c = plain_case(seed)
    lo, hi = scene_box(c["sp"])
    c["lo"], c["hi"] = lo, hi
    c["rays"] = _rays(c["sp"], lo, hi, np.random.default_rng(9000 + seed))
    c["probes"] = _probes(c["sp"], lo, hi, np.random.default_rng(9500 + seed))
    c["rays"].setflags(write=False)
    c["probes"].setflags(write=False)
    return c


def oracle_trace(scene, rays, any_hit):
    """hit (n,) bool, t (n,) float32 (a miss: the ray's tmax), sphere (n,) uint32
    (a miss: NO_HIT), and per-ray node / prim counts."""
    n = len(rays)
    hit = np.zeros(n, bool)
    t = np.zeros(n, np.float32)
    sphere = np.full(n, NO_HIT, np.uint32)
    nodes = np.zeros(n, np.uint64)
    prims = np.zeros(n, np.uint64)
    for i, r in enumerate(rays):
        h, th, idx, cnt = scene.trace(r[0:3], r[4:7], r[3], r[7], any_hit=any_hit)
        hit[i], t[i], sphere[i] = h, (th if h else r[7]), (idx if h else NO_HIT)
        nodes[i], prims[i] = cnt[2], cnt[3]
    return hit, t, sphere, nodes, prims


def _frozen(arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


_MODELS = {}


def model(seed, orc, gbuffer=False):
    """The expectations of a case (read-only arrays):
      nearest, any  (hit, t, sphere, nodes, prims) over all 520 rays: the oracle's
                    walk on the first 512; the 8 bad rays are not given to it
                    (test_gpu_query.test_edge_rays says why) and hold the miss
                    {tmax, NO_HIT} with no node or prim counted
      multi         multihit_ref.reference(sp, rays, 16): (t, sphere, count, total)
      overlap, overlap_skip   overlap_ref.reference(sp, probes, 16[, skip_self])
      info, root    the oracle tree's counts and its grown root box
      gbuffer       with `gbuffer`: gbuffer_ref.expected of the case's camera
      pixels        with `gbuffer`: up to two pixels (x, y) that hit and two that miss"""
    m = _MODELS.get(seed)
    if m is None:
        c = query_case(seed)
        s = oracle_scene(orc, c)
        m = dict(case=c, info=s.info(), root=s.root(), gbuffer=None, pixels=None)
        for kind in ("nearest", "any"):
            hit, t, sphere, nodes, prims = oracle_trace(s, c["rays"][:N_ORACLE], kind == "any")
            bad = c["rays"][N_ORACLE:]
            m[kind] = _frozen((np.concatenate([hit, np.zeros(N_BAD_RAYS, bool)]),
                               np.concatenate([t, bad[:, 7]]),
                               np.concatenate([sphere, np.full(N_BAD_RAYS, NO_HIT, np.uint32)]),
                               np.concatenate([nodes, np.zeros(N_BAD_RAYS, np.uint64)]),
                               np.concatenate([prims, np.zeros(N_BAD_RAYS, np.uint64)])))
        s.close()
        m["multi"] = _frozen(mr.reference(c["sp"], c["rays"], mr.K_MAX))
        m["overlap"] = _frozen(ov.reference(c["sp"], c["probes"], ov.K_MAX))
        m["overlap_skip"] = _frozen(ov.reference(c["sp"], c["probes"], ov.K_MAX, skip_self=True))
        _MODELS[seed] = m
    if gbuffer and m["gbuffer"] is None:
        c = m["case"]
        s = oracle_scene(orc, c)
        m["gbuffer"] = gbuffer_ref.expected(orc, s, c["sp"], c["al"], c["pose"], c["K"], c["w"], c["h"])
        s.close()
        hit = m["gbuffer"]["sphere"].reshape(-1) != NO_HIT
        px = []
        for flat in (np.flatnonzero(hit), np.flatnonzero(~hit)):
            px += [int(flat[(a * len(flat)) // 3]) for a in (1, 2)][:len(flat)] if len(flat) else []
        m["pixels"] = [(p % c["w"], p // c["w"]) for p in px]
    return m
