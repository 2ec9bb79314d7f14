"""The CPU reference of the sphere-overlap query (rt_query_overlaps, DESIGN.md
5.11) and the scenes and probes its tests share (test_overlap_cpu.py,
test_gpu_overlap.py).

The acceptance predicate is d2 <= s * s with dx = p.x - c.x (likewise dy, dz),
d2 = (dx*dx + dy*dy) + dz*dz, s = R + r: every operation one IEEE f32
operation, which numpy restates exactly on float32 arrays (no fused multiply-
add, no wider intermediate), so no native program is needed.
"""
import functools

import numpy as np

import multihit_ref as mr

NO_HIT = 0xFFFFFFFF
MORE = 0x80000000
K_MAX = 16
N_CONTACT, N_INSIDE, N_POINTS, N_SMALL, N_LARGE, N_FAR = 384, 128, 128, 256, 64, 64
N_PROBES = N_CONTACT + N_INSIDE + N_POINTS + N_SMALL + N_LARGE + N_FAR
FAR = slice(N_PROBES - N_FAR, N_PROBES)

# the octrees: A, B and D are multihit_ref's; the hand-made scenes follow
E_TREE = dict(root_min=(0.0, 0.0, 0.0), root_max=(1.0, 1.0, 1.0), max_depth=4, leaf_capacity=2)
# F: scene A moved 1000 units from the origin, where an ulp of a coordinate (6e-5) is
# 50 times the builders' margin: the grown box's M term is what keeps its pairs
F_OFFSET = 1000.0
F_TREE = dict(root_min=(F_OFFSET,) * 3, root_max=(F_OFFSET + 1.28,) * 3, max_depth=7, leaf_capacity=8)
# G: three spheres that end 1e-5 below the root's mid plane, one per axis, in F's
# root box (with a fourth, and one sphere a leaf, so that the root splits)
G_TREE = dict(root_min=(F_OFFSET,) * 3, root_max=(F_OFFSET + 1.28,) * 3, max_depth=3, leaf_capacity=1)
TREES = {"A": mr.tree("A"), "B": mr.tree("B"), "D": mr.tree("D"),
         "one": dict(max_depth=7, leaf_capacity=8), "five": dict(max_depth=7, leaf_capacity=8),
         "E": E_TREE, "F": F_TREE, "G": G_TREE}


@functools.lru_cache(maxsize=None)
def spheres(name):
    """(n, 4) float32 spheres of scene `name` (read-only).  "one" and "five":
    the root is a leaf.  "E": 18 spheres of radius 1/8 on a lattice of pitch
    1/4 (every neighbour pair exactly tangent, every sphere tangent to cell
    faces of its depth-4 octree over [0, 1]^3), then a duplicate of sphere 0.
    "F": scene A moved by (1000, 1000, 1000), coordinates rounded to f32 there.
    "G": g_probes()'s scene."""
    if name in ("A", "B", "D"):
        return mr.spheres(name)
    if name == "F":
        sp = np.array(mr.spheres("A"), np.float32)
        sp[:, :3] += np.float32(F_OFFSET)
    elif name == "G":
        sp = _g_scene()[0]
    elif name == "one":
        sp = np.array([(0.5, 0.625, 0.75, 0.125)], np.float32)
    elif name == "five":
        sp = np.array([(0.25, 0.25, 0.25, 0.125), (0.5, 0.25, 0.25, 0.125), (1.0, 1.0, 1.0, 0.25),
                       (0.5, 0.25, 0.25, 0.125), (0.625, 0.75, 0.5, 0.0625)], np.float32)
    elif name == "E":
        g = [(x, y, z, 0.125) for z in (0.375, 0.625) for y in (0.25, 0.5, 0.75) for x in (0.25, 0.5, 0.75)]
        sp = np.array(g + [g[0]], np.float32)
    else:
        raise KeyError(name)
    sp.setflags(write=False)
    return sp


def _unit(g, n):
    d = g.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


@functools.lru_cache(maxsize=None)
def probes(name):
    """(1024, 4) float32 probes in rt_probe layout (read-only), from
    default_rng(3) in this order: the scene's first 384 spheres (a smaller
    scene's, repeated); 128 points at c + 0.5 r * unit of random spheres; 128
    points uniform in [-0.1, 1.38]^3; 256 probes with centres there and R in
    [0, 0.1]; 64 large ones, centres in [0, 1.28]^3, R in [0.2, 0.5]; 64 far
    ones, components +-[2, 3], R in [0, 0.3].  Scene F's and G's uniform and large
    centres are moved with the scene; its far probes stay where they are."""
    sp = spheres(name)
    off = np.float32(F_OFFSET if name in ("F", "G") else 0.0)
    g = np.random.default_rng(3)
    out = np.zeros((N_PROBES, 4), np.float32)
    at = 0
    out[:N_CONTACT] = sp[np.arange(N_CONTACT) % len(sp)]
    at += N_CONTACT
    k = g.integers(0, len(sp), N_INSIDE)
    out[at:at + N_INSIDE, :3] = sp[k, :3] + 0.5 * sp[k, 3:4] * _unit(g, N_INSIDE)
    at += N_INSIDE
    out[at:at + N_POINTS, :3] = g.uniform(-0.1, 1.38, (N_POINTS, 3)) + off
    at += N_POINTS
    out[at:at + N_SMALL, :3] = g.uniform(-0.1, 1.38, (N_SMALL, 3)) + off
    out[at:at + N_SMALL, 3] = g.uniform(0.0, 0.1, N_SMALL)
    at += N_SMALL
    out[at:at + N_LARGE, :3] = g.uniform(0.0, 1.28, (N_LARGE, 3)) + off
    out[at:at + N_LARGE, 3] = g.uniform(0.2, 0.5, N_LARGE)
    at += N_LARGE
    out[at:, :3] = g.uniform(2.0, 3.0, (N_FAR, 3)) * g.choice([-1.0, 1.0], (N_FAR, 3))
    out[at:, 3] = g.uniform(0.0, 0.3, N_FAR)
    out.setflags(write=False)
    return out


def accepted(sp, pr, skip_self=False):
    """(n_probes, n_spheres) bool: the predicate, in f32, in the spec's order."""
    sp = np.ascontiguousarray(sp, np.float32)
    pr = np.ascontiguousarray(pr, np.float32)
    acc = np.zeros((len(pr), len(sp)), bool)
    with np.errstate(all="ignore"):
        for a in range(0, len(pr), 128):  # (in slices: the temporaries stay small)
            p = pr[a:a + 128]
            dx = p[:, None, 0] - sp[None, :, 0]
            dy = p[:, None, 1] - sp[None, :, 1]
            dz = p[:, None, 2] - sp[None, :, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
            s = p[:, None, 3] + sp[None, :, 3]
            assert d2.dtype == np.float32 and s.dtype == np.float32
            acc[a:a + 128] = d2 <= s * s
    ok = np.isfinite(pr).all(axis=1) & (pr[:, 3] >= 0)
    acc &= ok[:, None]
    if skip_self:
        i = np.arange(min(len(pr), len(sp)))
        acc[i, i] = False
    return acc


def reference(sp, pr, k=K_MAX, skip_self=False):
    """Brute force over all of `sp` for every probe: (indices (n, k) uint32,
    count (n,) uint32, more (n,) bool, total (n,) int64) in the layout of
    rt_query_overlaps; `total` is the size of each probe's accepted set."""
    acc = accepted(sp, pr, skip_self)
    n = len(acc)
    indices = np.full((n, k), NO_HIT, np.uint32)
    total = acc.sum(axis=1).astype(np.int64)
    for i in np.flatnonzero(total):
        members = np.flatnonzero(acc[i])[:k]  # ascending
        indices[i, :len(members)] = members
    return indices, np.minimum(total, k).astype(np.uint32), total > k, total


@functools.lru_cache(maxsize=None)
def expected(name):
    """reference() of scene `name`'s probe mix at k = 16, computed once
    (read-only).  A smaller k's answer is its first k columns: cut()."""
    out = reference(spheres(name), probes(name), K_MAX)
    for a in out:
        a.setflags(write=False)
    return out


def cut(ref, k):
    """The answer for k <= the reference's k from its (indices, count, more, total)."""
    indices, _, _, total = ref
    assert k <= indices.shape[1]
    return (np.ascontiguousarray(indices[:, :k]), np.minimum(total, k).astype(np.uint32), total > k)


def e_probes():
    """Scene E's boundary probes, (probes (n, 4) float32, cases): each case is
    (probe row, sphere index, accepted?).
      * every lattice neighbour pair (i, j) with i on the high side: sphere i as
        the probe is exactly tangent to j (accepted), and moved one ulp further
        along that axis it is not;
      * point probes (R = 0) on sphere j's surface where it touches a cell face
        (x = c.x + 1/8, a multiple of 1/16), and one ulp further out."""
    sp = spheres("E")
    rows, cases = [], []
    for i in range(18):
        for j in range(18):
            d = sp[i, :3] - sp[j, :3]
            axis = np.flatnonzero(d)
            if len(axis) == 1 and d[axis[0]] == np.float32(0.25):
                rows.append(sp[i].copy())
                cases.append((len(rows) - 1, j, True))
                moved = sp[i].copy()
                moved[axis[0]] = np.nextafter(moved[axis[0]], np.float32(np.inf))
                rows.append(moved)
                cases.append((len(rows) - 1, j, False))
    for j in range(18):
        on = np.array((sp[j, 0] + np.float32(0.125), sp[j, 1], sp[j, 2], 0.0), np.float32)
        rows.append(on)
        cases.append((len(rows) - 1, j, True))
        out = on.copy()
        out[0] = np.nextafter(out[0], np.float32(np.inf))
        rows.append(out)
        cases.append((len(rows) - 1, j, False))
    return np.array(rows, np.float32), cases


@functools.lru_cache(maxsize=None)
def _g_scene():
    """Scene G and its three probes.  In a root box 1000 units from the origin
    an ulp of a coordinate is 2^-14 = 6.1e-5, 50 times the builders' margin.
    Sphere a (a = x, y, z) ends 1e-5 below the root's mid plane e on axis a, so
    only cells below e list it; probe a sits 3 ulps above e on that axis with
    the radius at which f32 just accepts the pair.  Its box's lower corner,
    p - R = e - 1e-5 in real numbers, rounds to e itself in f32: a box without
    the M term of the slack starts at the plane and misses every cell below it."""
    f32, f64 = np.float32, np.float64
    lo = f64(f32(F_OFFSET))
    e = lo + (f64(f32(F_OFFSET + 1.28)) - lo) * 0.5   # the builders' cell edge, lo + ext * (c / cells)
    assert f64(f32(e)) == e
    sp = np.zeros((4, 4), f32)
    pr = np.zeros((3, 4), f32)
    for a in range(3):
        c = np.full(3, F_OFFSET + 0.3, f32)
        c[a] = f32(F_OFFSET + 0.6)
        r = f32(e - 1e-5 - f64(c[a]))
        p = c.copy()
        p[a] = f32(e + 3 * 2.0 ** -14)
        d = p[a] - c[a]
        R = f32(f64(p[a]) - (f64(c[a]) + f64(r)))
        while not d * d <= (R + r) * (R + r):   # the smallest R near it that f32 accepts
            R = np.nextafter(R, f32(np.inf))
        assert abs(f64(p[a]) - f64(R) - (e - 1e-5)) < 1e-7
        sp[a] = (*c, r)
        pr[a] = (*p, R)
    sp[3] = (F_OFFSET + 0.9, F_OFFSET + 0.9, F_OFFSET + 0.9, 0.05)
    sp.setflags(write=False)
    pr.setflags(write=False)
    return sp, pr


def g_probes():
    """Scene G's three probes: probe a touches sphere a and nothing else."""
    return _g_scene()[1]
