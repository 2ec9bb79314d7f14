"""The CPU reference of the swept-sphere query (rt_sweep_spheres, DESIGN.md
5.14) and the scenes and casts its tests share (test_sweep_cpu.py,
test_gpu_sweep.py, test_gpu_sweep_fuzz.py).

tests/native/sweep_ref.cpp, compiled with the address and undefined-behaviour
sanitizers and run as a child process exactly as multihit_ref.py runs its own,
brute-forces every sphere for every cast with explicit fmaf.  Spheres, rays,
radii and results travel as raw binary files.
"""
import functools
import os
import subprocess
import tempfile

import numpy as np

import overlap_ref as ov

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_HIT = 0xFFFFFFFF
ENTRY_ONLY, SKIP_SELF = 1, 2
SCENES = ("A", "B", "D", "one", "five", "E", "F", "G")
# casts, in this order: multihit_ref.rays' three kinds, then the four kinds of this query
N_SURFACE, N_AIMED, N_RANDOM, N_FAR, N_AXIS, N_INSIDE, N_CONTACT = 384, 192, 192, 64, 64, 64, 64
N_CASTS = N_SURFACE + N_AIMED + N_RANDOM + N_FAR + N_AXIS + N_INSIDE + N_CONTACT
FAR = slice(N_SURFACE + N_AIMED + N_RANDOM, N_SURFACE + N_AIMED + N_RANDOM + N_FAR)
BOX = 1.28          # the configured cube's size: "1,000 x the box size away" is 1280


def normalise_f32(d):
    """Directions normalised in f32: each component divided by the f32 length
    sqrt((x*x + y*y) + z*z), every operation one f32 operation."""
    d = np.ascontiguousarray(d, np.float32)
    n = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    assert n.dtype == np.float32
    with np.errstate(all="ignore"):
        return d / n[:, None]


def _unit(g, n):
    d = g.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


@functools.lru_cache(maxsize=None)
def casts(name):
    """(rays (1024, 8) float32 in rt_ray layout, radii (1024,) float32), both
    read-only, for overlap_ref's scene `name`, from default_rng(23), every
    direction normalised in f32:
      384 from just off sphere surfaces with a short window, 192 from around the
      root box aimed at its centre, 192 from around it in random directions
      (multihit_ref.rays' three kinds);
      64 from 1,000 x the box size away: 32 aimed at a point inside a sphere,
      32 axis-parallel through a sphere's centre (on G: down axis a onto
      sphere a, whose top is 1e-5 below a cell face);
      64 axis-parallel through a point inside a sphere, from 1.5 boxes back;
      64 that start inside a sphere;
      64 that start in contact: the ball overlaps a sphere by less than its R.
    Radii by i % 3: 0, uniform in [0, 0.02], uniform in [0.02, 0.2]; the contact
    casts have R in [0.02, 0.2].  Scene F's and G's casts are moved with the scene."""
    sp = np.asarray(ov.spheres(name), np.float64)
    m = len(sp)
    off = ov.F_OFFSET if name in ("F", "G") else 0.0
    g = np.random.default_rng(23)
    rays = np.zeros((N_CASTS, 8), np.float64)
    radii = np.zeros(N_CASTS, np.float64)
    cls = np.arange(N_CASTS) % 3
    radii[cls == 1] = g.uniform(0.0, 0.02, (cls == 1).sum())
    radii[cls == 2] = g.uniform(0.02, 0.2, (cls == 2).sum())
    at = 0
    k = g.integers(0, m, N_SURFACE)
    s = rays[:N_SURFACE]
    s[:, :3] = sp[k, :3] + 1.001 * sp[k, 3:4] * _unit(g, N_SURFACE)
    s[:, 3] = 1e-5
    s[:, 4:7] = _unit(g, N_SURFACE)
    s[:, 7] = 0.5
    at += N_SURFACE
    o = rays[at:at + N_AIMED + N_RANDOM]
    o[:, :3] = g.uniform(-0.5, 1.78, (N_AIMED + N_RANDOM, 3)) + off
    aim = (0.64 + off) - o[:N_AIMED, :3]
    o[:N_AIMED, 4:7] = aim / np.linalg.norm(aim, axis=1, keepdims=True)
    o[N_AIMED:, 4:7] = _unit(g, N_RANDOM)
    o[:, 7] = np.inf
    at += N_AIMED + N_RANDOM
    # far: aimed at a point inside a sphere; then straight along an axis through a centre
    f = rays[at:at + N_FAR]
    half = N_FAR // 2
    k = g.integers(0, m, half)
    through = sp[k, :3] + 0.3 * sp[k, 3:4] * _unit(g, half)
    back = _unit(g, half)
    f[:half, :3] = through + 1000.0 * BOX * back
    f[:half, 4:7] = -back
    j = np.arange(half)
    # (scene G: down axis a onto sphere a, which ends 1e-5 below the root's mid plane)
    axis, sphere = j % 3, (j % 3 if name == "G" else j % m)
    sign = np.where((j // 12) % 2 == 0, 1.0, 1.0 if name == "G" else -1.0)
    d = np.zeros((half, 3))
    d[j, axis] = -sign
    f[half:, :3] = sp[sphere, :3] - d * (1000.0 * BOX * (1.0 + 0.37 * j / half))[:, None]
    f[half:, 4:7] = d
    f[:, 7] = np.inf
    at += N_FAR
    a = rays[at:at + N_AXIS]
    k = g.integers(0, m, N_AXIS)
    through = sp[k, :3] + 0.3 * sp[k, 3:4] * _unit(g, N_AXIS)
    d = np.zeros((N_AXIS, 3))
    d[np.arange(N_AXIS), g.integers(0, 3, N_AXIS)] = g.choice([-1.0, 1.0], N_AXIS)
    a[:, :3] = through - 1.5 * BOX * d
    a[:, 4:7] = d
    a[:, 7] = np.inf
    at += N_AXIS
    w = rays[at:at + N_INSIDE]
    k = g.integers(0, m, N_INSIDE)
    w[:, :3] = sp[k, :3] + 0.5 * sp[k, 3:4] * _unit(g, N_INSIDE)
    w[:, 4:7] = _unit(g, N_INSIDE)
    w[:, 7] = np.inf
    at += N_INSIDE
    c = rays[at:]
    k = g.integers(0, m, N_CONTACT)
    radii[at:] = g.uniform(0.02, 0.2, N_CONTACT)
    c[:, :3] = sp[k, :3] + (sp[k, 3] + g.uniform(0.2, 0.9, N_CONTACT) * radii[at:])[:, None] * _unit(g, N_CONTACT)
    c[:, 4:7] = _unit(g, N_CONTACT)
    c[:, 7] = np.inf
    rays = rays.astype(np.float32)
    rays[:, 4:7] = normalise_f32(rays[:, 4:7])
    radii = radii.astype(np.float32)
    rays.setflags(write=False)
    radii.setflags(write=False)
    return rays, radii


def cast_ok(rays, radii):
    """The validity rule, in f32 in the spec's order."""
    rays = np.ascontiguousarray(rays, np.float32)
    radii = np.ascontiguousarray(radii, np.float32)
    d = rays[:, 4:7]
    with np.errstate(all="ignore"):
        n2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        unit = np.abs(n2 - np.float32(1.0)) <= np.float32(2.0 ** -18)
        return (np.isfinite(rays[:, :3]).all(axis=1) & np.isfinite(d).all(axis=1) & np.isfinite(radii)
                & (radii >= 0) & unit)


def _build(src, prefix):
    d = tempfile.TemporaryDirectory(prefix=prefix)
    exe = os.path.join(d.name, os.path.splitext(src)[0])
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "native", src)])
    return d, exe


@functools.lru_cache(maxsize=None)
def _exe():
    """The reference program, compiled once per process into a directory that
    lives as long as the process."""
    return _build("sweep_ref.cpp", "sweep_ref_")


def reference(sp, rays, radii, flags=0):
    """Brute force over all of `sp` for every cast: (t (n,) float32, sphere (n,)
    uint32) in the layout of rt_sweep_spheres; `radii` a scalar or (n,)."""
    d, exe = _exe()
    n = len(rays)
    rr = np.ascontiguousarray(np.broadcast_to(np.asarray(radii, np.float32), (n,)))
    with tempfile.TemporaryDirectory(dir=d.name) as td:
        ps, pr, pq, po = (os.path.join(td, f) for f in ("spheres.f32", "rays.f32", "radii.f32", "out.u32"))
        np.ascontiguousarray(sp, np.float32).tofile(ps)
        np.ascontiguousarray(rays, np.float32).tofile(pr)
        rr.tofile(pq)
        r = subprocess.run([exe, ps, pr, pq, str(int(flags)), po], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, r.stderr  # a sanitizer report fails the test
        raw = np.fromfile(po, np.uint32).reshape(n, 2)
    return np.ascontiguousarray(raw[:, 0]).view(np.float32), np.ascontiguousarray(raw[:, 1])


@functools.lru_cache(maxsize=None)
def expected(name, flags=0):
    """reference() of scene `name`'s casts, computed once per flags (read-only)."""
    out = reference(ov.spheres(name), *casts(name), flags)
    for a in out:
        a.setflags(write=False)
    return out


def fuzz_casts(c):
    """A query_fuzz.query_case's casts: its 520 rays with the directions of the
    ordinary ones renormalised in f32 (its deliberately bad rays stay as they
    are), and as radii its probes' radius column (bad ones included) with every
    third radius 0."""
    from query_fuzz import N_ORACLE
    rays = np.array(c["rays"], np.float32)
    rays[:N_ORACLE, 4:7] = normalise_f32(rays[:N_ORACLE, 4:7])
    radii = np.array(c["probes"][:, 3], np.float32)
    radii[::3] = 0.0
    return rays, radii


# Scene L: a sheet of 256 small spheres in one z layer of the root box [0, 1]^3,
# one per depth-4 cell of that layer, and one oblique cast across the sheet's
# plane that slips between them: the guide has to follow the line, not its box.
L_TREE = dict(root_min=(0.0, 0.0, 0.0), root_max=(1.0, 1.0, 1.0), max_depth=4, leaf_capacity=1)


def l_scene():
    """(spheres (256, 4), rays (1, 8), radius 0.0)."""
    ij = np.arange(16)
    x, y = np.meshgrid((ij + 0.5) / 16, (ij + 0.5) / 16, indexing="ij")
    sp = np.stack([x.ravel(), y.ravel(), np.full(256, 17 / 32), np.full(256, 1 / 64)], axis=1).astype(np.float32)
    ray = np.zeros((1, 8), np.float32)
    ray[0, :3] = (-0.25, 0.13, 0.55125)
    ray[0, 4:7] = normalise_f32(np.array([(1.0, 0.5, 0.0)], np.float32))[0]
    ray[0, 7] = np.inf
    return sp, ray, 0.0
