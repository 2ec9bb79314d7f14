"""The CPU reference of the ordered multi-hit query and the
scenes and rays its tests share (test_multihit_cpu.py, test_gpu_multihit.py).

tests/native/multihit_ref.cpp, compiled with the address and undefined-behaviour
sanitizers and run as a child process, brute-forces every sphere for every ray
with explicit fmaf (a numpy restatement through float64 would round twice).
Spheres, rays and results travel as raw binary files.
"""
import functools
import os
import subprocess
import tempfile

import numpy as np

import raytracingstudy_amd as rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_HIT = 0xFFFFFFFF
K_MAX = 16
# A and B are test_gpu_query.py's scenes; D is dense: about 14 leaf references
# per sphere, so every ray meets the same sphere in several leaves
SCENES = {"A": dict(n=1000, max_depth=7, leaf_capacity=8),
          "B": dict(n=20000, max_depth=12, leaf_capacity=2),
          "D": dict(n=1500, max_depth=5, leaf_capacity=8)}
N_SURFACE, N_AIMED, N_RANDOM = 512, 256, 256
N_RAYS = N_SURFACE + N_AIMED + N_RANDOM


@functools.lru_cache(maxsize=None)
def spheres(name):
    """(n, 4) float32 spheres of scene `name` (read-only)."""
    if name == "D":
        g = np.random.default_rng(7)
        c = g.uniform(0, 1.28, (1500, 3))
        r = g.uniform(0.04, 0.08, 1500)
        sp = np.concatenate([c, r[:, None]], 1).astype(np.float32)
    else:
        sp = np.array(rt.generate_spheres(SCENES[name]["n"], rt.SEED)[0], np.float32)
    sp.setflags(write=False)
    return sp


def tree(name):
    return dict(max_depth=SCENES[name]["max_depth"], leaf_capacity=SCENES[name]["leaf_capacity"])


def _unit(g, n):
    d = g.normal(size=(n, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def rays(name):
    """(1024, 8) float32 in rt_ray layout (read-only): 512 rays from just off
    sphere surfaces with a short window, 256 from around the root box aimed at
    its centre, 256 from around it in random directions."""
    sp = spheres(name)
    g = np.random.default_rng(2)
    out = np.zeros((N_RAYS, 8), np.float32)
    k = g.integers(0, len(sp), N_SURFACE)
    s = out[:N_SURFACE]
    s[:, :3] = sp[k, :3] + np.float32(1.001) * sp[k, 3:4] * _unit(g, N_SURFACE)
    s[:, 3] = 1e-5
    s[:, 4:7] = _unit(g, N_SURFACE)
    s[:, 7] = 0.5
    o = out[N_SURFACE:]
    o[:, :3] = g.uniform(-0.5, 1.78, (N_AIMED + N_RANDOM, 3))
    aim = np.float32(0.64) - o[:N_AIMED, :3].astype(np.float64)
    o[:N_AIMED, 4:7] = (aim / np.linalg.norm(aim, axis=1, keepdims=True)).astype(np.float32)
    o[N_AIMED:, 4:7] = _unit(g, N_RANDOM)
    o[:, 7] = np.inf
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _exe():
    """The reference program, compiled once per process into a directory that
    lives as long as the process."""
    d = tempfile.TemporaryDirectory(prefix="multihit_ref_")
    exe = os.path.join(d.name, "multihit_ref")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "multihit_ref.cpp")])
    return d, exe


def reference(sp, ray_set, k=K_MAX):
    """Brute force over all of `sp` for every ray: (t (n, k) float32, sphere
    (n, k) uint32, count (n,) uint32, total (n,) uint32), in the layout of
    rt_trace_rays_multi; `total` is the size of each ray's accepted set."""
    d, exe = _exe()
    n = len(ray_set)
    with tempfile.TemporaryDirectory(dir=d.name) as td:
        ps, pr, po = (os.path.join(td, f) for f in ("spheres.f32", "rays.f32", "out.u32"))
        np.ascontiguousarray(sp, np.float32).tofile(ps)
        np.ascontiguousarray(ray_set, np.float32).tofile(pr)
        r = subprocess.run([exe, ps, pr, str(int(k)), po], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, r.stderr  # a sanitizer report fails the test
        raw = np.fromfile(po, np.uint32).reshape(n, 2 * k + 2)
    hits = raw[:, :2 * k].reshape(n, k, 2)
    t = np.ascontiguousarray(hits[:, :, 0]).view(np.float32)
    sphere = np.ascontiguousarray(hits[:, :, 1])
    return t, sphere, raw[:, 2 * k].copy(), raw[:, 2 * k + 1].copy()


@functools.lru_cache(maxsize=None)
def expected(name):
    """reference() of scene `name`'s rays at k = 16, computed once (read-only).
    The k smallest for k < 16 are its first k columns: cut()."""
    out = reference(spheres(name), rays(name), K_MAX)
    for a in out:
        a.setflags(write=False)
    return out


def cut(ref, ray_set, k):
    """The answer for k <= the reference's k from its (t, sphere, count, total):
    the first k columns, count = min(k, total).  (A slot past the count already
    holds the ray's tmax and NO_HIT.)"""
    t, sphere, _, total = ref
    assert k <= t.shape[1] and len(ray_set) == len(t)
    return (np.ascontiguousarray(t[:, :k]), np.ascontiguousarray(sphere[:, :k]),
            np.minimum(total, k).astype(np.uint32))
