"""CPU tests of the swept-sphere query (rt_sweep_spheres, rt_sweep_at,
rt_pick_thick): the surface (header, ctypes mirror, the error
path with no renderer, the C++ wrapper), the brute-force reference the GPU
tests compare against (tests/sweep_ref.py) pinned to the oracle and to the
multi-hit reference, the header's validity and test against that reference bit
for bit, and the grown-cell slab test's slack: descending the oracle's tree by
the header's test, with the answer's own t as the bound, reaches a leaf that
lists the answer, for every cast.  The queries themselves run in
test_gpu_sweep.py and test_gpu_sweep_fuzz.py.
"""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from raytracingstudy_amd import _lib

import multihit_ref as mr
import overlap_ref as ov
import sweep_ref as sr
from bins_native import f32_args
from plain_fuzz import SEEDS, oracle_scene
from query_fuzz import query_case
from test_overlap_cpu import _leaves

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
NO_HIT = sr.NO_HIT


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- surface ----------------------------------------------------------------
def _header():
    src = open(os.path.join(INCLUDE, "rt.h")).read()
    return " ".join(re.sub(r"/\*.*?\*/", "", src, flags=re.S).split())


def test_header_declares_the_sweep_entry_points():
    src = _header()
    assert "enum { RT_SWEEP_ENTRY_ONLY = 1u, RT_SWEEP_SKIP_SELF = 2u };" in src
    assert ("int rt_sweep_spheres(rt_renderer* r, const void* dev_rays, const void* dev_radii, float radius, "
            "uint32_t n, uint32_t flags, void* dev_hits, void* stream, rt_stats* stats);") in src
    assert ("int rt_sweep_at(rt_renderer* r, const float origin[3], const float dir[3], float radius, "
            "float tmax, uint32_t flags, rt_hit* hit_out, float point_out[3]);") in src
    assert ("int rt_pick_thick(rt_renderer* r, float u, float v, float radius, rt_hit* hit_out, "
            "float point_out[3]);") in src
    assert re.search(r"#define RT_ABI_VERSION 4\b", src)  # additive: the version stays
    # the header states the unit-length rule and that an f32-normalised direction passes
    text = " ".join(open(os.path.join(INCLUDE, "rt.h")).read().replace("*", " ").split())
    assert "|((dx dx + dy dy) + dz dz) - 1| > 2^-18" in text and "normalised in f32" in text


def test_ctypes_mirror_matches_the_header():
    assert _lib.load().rt_abi_version() == 4
    assert (_lib.RT_SWEEP_ENTRY_ONLY, _lib.RT_SWEEP_SKIP_SELF) == (1, 2)
    res, args = _lib.SIGNATURES["rt_sweep_spheres"]
    assert res is ctypes.c_int and len(args) == 9
    assert args[3] is ctypes.c_float and args[4] is ctypes.c_uint32 and args[5] is ctypes.c_uint32
    res, args = _lib.SIGNATURES["rt_sweep_at"]
    assert res is ctypes.c_int and len(args) == 8
    assert args[3] is ctypes.c_float and args[4] is ctypes.c_float and args[5] is ctypes.c_uint32
    res, args = _lib.SIGNATURES["rt_pick_thick"]
    assert res is ctypes.c_int and len(args) == 6 and all(a is ctypes.c_float for a in args[1:4])


def test_sweeps_without_a_renderer_are_errors_not_crashes():
    """No GPU, hence no handle: the three calls report RT_E_INVALID, name
    themselves and leave their outputs untouched."""
    lib = _lib.load()
    rays = (ctypes.c_float * 8)()
    hit = _lib.RtHit()
    hit.t, hit.sphere = 7.0, 7
    pt = (ctypes.c_float * 3)(7.0, 7.0, 7.0)
    assert lib.rt_sweep_spheres(None, None, None, 0.0, 0, 0, None, None, None) == _lib.RT_E_INVALID
    assert lib.rt_sweep_spheres(None, ctypes.addressof(rays), None, 0.1, 1, 0, ctypes.addressof(hit), None,
                                None) == _lib.RT_E_INVALID
    assert b"rt_sweep_spheres" in lib.rt_last_error(None)
    o = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    d = (ctypes.c_float * 3)(1.0, 0.0, 0.0)
    assert lib.rt_sweep_at(None, o, d, 0.1, 1.0, 0, ctypes.byref(hit), pt) == _lib.RT_E_INVALID
    assert b"rt_sweep_at" in lib.rt_last_error(None)
    assert lib.rt_pick_thick(None, 1.0, 1.0, 0.1, ctypes.byref(hit), pt) == _lib.RT_E_INVALID
    assert b"rt_pick_thick" in lib.rt_last_error(None)
    assert (hit.t, hit.sphere, list(pt)) == (7.0, 7, [7.0, 7.0, 7.0])  # untouched


def test_cpp_wrapper_with_the_sweep_methods_compiles(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "no C++ compiler"
    src = tmp_path / "use_sweep.cpp"
    src.write_text('#include <cmath>\n#include "rt_renderer.hpp"\n'
                   "uint32_t use(rtamd::KernelRenderer& r, const void* rays, const void* radii, void* hits,\n"
                   "             void* stream) {\n"
                   "    rt_stats st;\n"
                   "    r.sweepSpheres(rays, 4u, 0.05f, hits);\n"
                   "    r.sweepSpheres(rays, 4u, 0.0f, hits, radii, RT_SWEEP_ENTRY_ONLY | RT_SWEEP_SKIP_SELF, stream, &st);\n"
                   "    const float o[3] = {0.5f, 0.5f, 0.5f}, d[3] = {1.0f, 0.0f, 0.0f};\n"
                   "    float at[3];\n"
                   "    const rt_hit a = r.sweepAt(o, d, 0.05f, INFINITY);\n"
                   "    const rt_hit b = r.sweepAt(o, d, 0.05f, 2.0f, RT_SWEEP_ENTRY_ONLY, at);\n"
                   "    const rt_hit c = r.pickThick(10.0f, 20.0f, 0.01f, at);\n"
                   "    return a.sphere + b.sphere + c.sphere + r.pickThick(1.0f, 2.0f, 0.0f).sphere;\n"
                   "}\n")
    r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", INCLUDE, str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---- the reference: pinned to the oracle, and not vacuous -----------------------
def test_f32_normalised_directions_are_valid_casts():
    """Every cast of every mix is valid: a direction normalised in f32 is of
    unit length to 2^-18 in the rule's own arithmetic, by a wide margin."""
    worst = 0.0
    for name in sr.SCENES:
        rays, radii = sr.casts(name)
        assert sr.cast_ok(rays, radii).all(), name
        d = rays[:, 4:7]
        n2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        worst = max(worst, float(np.abs(n2 - np.float32(1.0)).max()))
    assert worst <= 2.0 ** -22


@pytest.mark.parametrize("name", sr.SCENES)
def test_reference_at_radius_zero_is_the_oracles_brute_force(oracle, name):
    """R = 0, no flags: orc_trace_brute's hit, t bits and sphere on every cast
    of the mix (all are valid), and multihit_ref's first column at k = 1."""
    sp = ov.spheres(name)
    rays, _ = sr.casts(name)
    t, sphere = sr.reference(sp, rays, 0.0)
    sc = oracle.Scene(sp, None, **ov.TREES[name])
    for i, r in enumerate(rays):
        h, th, idx, _ = sc.trace(r[0:3], r[4:7], r[3], r[7], brute=True)
        if h:
            assert (sphere[i], _bits(t[i:i + 1])[0]) == (idx, _bits(np.float32(th))), (name, i)
        else:
            assert sphere[i] == NO_HIT and _bits(t[i:i + 1])[0] == _bits(r[7:8])[0], (name, i)
    sc.close()
    mt, ms, mc, _ = mr.reference(sp, rays, 1)
    assert np.array_equal(ms[:, 0], sphere) and np.array_equal(_bits(mt[:, 0]), _bits(t)), name
    assert np.array_equal(mc, (sphere != NO_HIT).astype(np.uint32))


def _leaf_cells(nodes, root_is_leaf):
    """{(depth, cx, cy, cz)} of the tree's leaves."""
    return {tuple(int(v) for v in row[:4]) for row in _leaves(nodes, root_is_leaf)}


def _centre_off_the_ray(oracle, name, rays, sphere):
    """Per cast with an answer: whether the winning sphere's centre lies in no
    leaf cell that the centre ray (the whole line, in float64) crosses."""
    sp = np.asarray(ov.spheres(name), np.float64)
    tree = ov.TREES[name]
    sc = oracle.Scene(ov.spheres(name), None, **tree)
    nodes, _ = sc.export_bfs()
    rmin, rmax = (np.asarray(a, np.float64) for a in sc.root())
    root_is_leaf = sc.info()["n_nodes"] == 1
    sc.close()
    cells = _leaf_cells(nodes, root_is_leaf)
    D = tree["max_depth"]
    out = np.zeros(len(rays), bool)
    for i in np.flatnonzero(sphere != NO_HIT):
        c = sp[sphere[i], :3]
        gc = np.clip(np.floor((c - rmin) / (rmax - rmin) * (1 << D)).astype(np.int64), 0, (1 << D) - 1)
        cell = next(((d, *(gc >> (D - d))) for d in range(D + 1) if (d, *(int(v) for v in gc >> (D - d))) in cells),
                    None)
        assert cell is not None, (name, i)   # the centre's cell lists the sphere, so it is a leaf
        d = cell[0]
        size = (rmax - rmin) / (1 << d)
        lo = rmin + np.array(cell[1:], np.float64) * size
        o, v = rays[i, :3].astype(np.float64), rays[i, 4:7].astype(np.float64)
        with np.errstate(all="ignore"):
            ta, tb = (lo - o) / v, (lo + size - o) / v
        t0, t1 = np.fmin(ta, tb), np.fmax(ta, tb)
        still = v == 0
        inside = (o >= lo) & (o <= lo + size)
        t0[still], t1[still] = np.where(inside[still], -np.inf, np.inf), np.where(inside[still], np.inf, -np.inf)
        out[i] = not max(t0.max(), float(rays[i, 3])) <= min(t1.min(), float(rays[i, 7]))
    return out


def test_cast_mixes_are_not_vacuous(oracle):
    """From the reference alone, per 1024-cast mix of A, B and D, at least 16
    each: hits, misses, casts whose sphere differs from their own R = 0 answer,
    casts whose answer changes under ENTRY_ONLY, and casts whose winning
    sphere's centre lies in no cell the centre ray crosses (what walk<> cannot
    find).  On E an exact tie in t resolved by index: sphere 18 is sphere 0
    again, so every cast that answers 0 tied with 18.  Measured:
      A  hits 749, misses 275, differ 441, entry 309, off the ray 169
      B  hits 819, misses 205, differ 523, entry 300, off the ray 420
      D  hits 886, misses 138, differ 459, entry 303, off the ray 524"""
    for name in ("A", "B", "D"):
        rays, radii = sr.casts(name)
        t, sphere = sr.expected(name)
        _, thin = sr.reference(ov.spheres(name), rays, 0.0)
        te, entry = sr.expected(name, sr.ENTRY_ONLY)
        got = dict(hits=int((sphere != NO_HIT).sum()), misses=int((sphere == NO_HIT).sum()),
                   differ=int((sphere != thin).sum()),
                   entry=int(((entry != sphere) | (_bits(te) != _bits(t))).sum()),
                   off=int(_centre_off_the_ray(oracle, name, rays, sphere).sum()))
        print(name, got)
        assert sum((got["hits"], got["misses"])) == sr.N_CASTS
        assert min(got.values()) >= 16, (name, got)
    t, sphere = sr.expected("E")
    assert np.array_equal(ov.spheres("E")[0], ov.spheres("E")[18])
    assert (sphere == 0).sum() >= 1 and not (sphere == 18).any()
    # skip-self takes exactly sphere i from cast i: on E, cast 0 then answers the duplicate at the same t
    ts, skip = sr.expected("E", sr.SKIP_SELF)
    rows = np.flatnonzero(sphere == np.arange(sr.N_CASTS))
    assert np.all(skip[rows] != rows)
    same = np.ones(sr.N_CASTS, bool)
    same[rows] = False
    assert np.array_equal(skip[same], sphere[same]) and np.array_equal(_bits(ts[same]), _bits(t[same]))


def test_scene_l_cast_misses():
    sp, ray, R = sr.l_scene()
    t, sphere = sr.reference(sp, ray, R)
    assert sphere[0] == NO_HIT and np.isinf(t[0]) and sr.cast_ok(ray, np.zeros(1, np.float32))[0]


# ---- the header's arithmetic -------------------------------------------------------
@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    """tests/native/sweep_math_dump.cpp, a stand-alone program built with the
    address and undefined-behaviour sanitizers; a sanitizer report fails the test."""
    d = tmp_path_factory.mktemp("sweep_math")
    exe = str(d / "sweep_math_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "sweep_math_dump.cpp")])

    def run(*args):
        r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, r.stderr
        return r.stdout
    run.dir = d
    return run


def _file(dump, name, a, dtype=np.float32):
    path = str(dump.dir / name)
    np.ascontiguousarray(a, dtype).tofile(path)
    return path


def odd_casts(sp):
    """Casts that the validity rule and the window decide, around sphere 0 of
    `sp`: (rays (n, 8), radii (n,), valid (n,) as the rule has it)."""
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    c = np.asarray(sp[0, :3], np.float32)
    base = np.array((c[0] - 2.0, c[1], c[2], 0.0, 1.0, 0.0, 0.0, inf), np.float32)
    rows, radii, valid = [], [], []

    def add(ok, R=0.01, **cols):
        r = base.copy()
        for col, v in cols.items():
            r[int(col[1:])] = v
        rows.append(r)
        radii.append(R)
        valid.append(ok)

    add(True)
    for col in ("c0", "c1", "c2", "c4", "c5", "c6"):
        add(False, **{col: nan})
        add(False, **{col: inf})
        add(False, **{col: -inf})
    add(True, c3=nan)            # the window decides: nothing is past a NaN tmin
    add(True, c3=-inf)
    add(True, c3=inf)
    add(True, c7=nan)
    add(True, c7=-inf)
    add(False, R=nan)
    add(False, R=inf)
    add(False, R=-inf)
    add(False, R=-1e-6)
    add(False, R=-1.0)
    add(True, R=-0.0)
    add(True, R=0.0)
    add(True, R=1e30)            # finite: everything is touched from the start
    add(False, c4=0.0)           # a zero direction
    add(False, c4=2.0)           # not of unit length
    add(False, c4=0.999)
    add(False, c4=np.float32(1.0 + 2.0 ** -18))   # |d|^2 - 1 is 2^-17: past the rule
    add(True, c4=np.float32(1.0 + 2.0 ** -20))
    add(True, c7=1.0, c3=1.0)    # tmax <= tmin
    add(True, c7=0.5, c3=1.0)
    add(True, c0=c[0] + 50.0)    # far outside the root box, pointing away
    add(True, c0=-0.0, c5=-0.0, c6=-0.0)
    return np.array(rows, np.float32), np.array(radii, np.float32), np.array(valid)


@pytest.mark.parametrize("name", sr.SCENES)
def test_header_is_the_reference(dump, name):
    """rt_sweep_math.h's sweep_cast_ok and sweep_isect, which the kernel runs,
    over every sphere against the reference program, bit for bit: the scene's
    mix and the odd casts, every flag combination."""
    sp = ov.spheres(name)
    rays, radii = sr.casts(name)
    orays, oradii, valid = odd_casts(sp)
    rays, radii = np.concatenate([rays, orays]), np.concatenate([radii, oradii])
    assert np.array_equal(sr.cast_ok(orays, oradii), valid)
    for flags in range(4):
        rows = np.array([[int(t, 16) for t in line.split()] for line in
                         dump("best", _file(dump, "r.f32", rays), _file(dump, "q.f32", radii),
                              _file(dump, "s.f32", sp), flags).splitlines()], np.int64)
        t, sphere = sr.reference(sp, rays, radii, flags)
        assert np.array_equal(rows[:, 0] == 1, sr.cast_ok(rays, radii)), (name, flags)
        assert np.array_equal(rows[:, 2].astype(np.uint32), sphere), (name, flags)
        assert np.array_equal(rows[:, 1].astype(np.uint32), _bits(t)), (name, flags)
        assert np.all(sphere[sr.N_CASTS:][~valid] == NO_HIT)
        assert np.array_equal(_bits(t[sr.N_CASTS:][~valid]), _bits(orays[~valid, 7]))


def _descend(dump, sc, depth, rays, radii, t, sphere, noslack=False):
    """(reached (n,) bool, node records read (n,)) of the header's descent of
    the oracle scene's exported tree with the bounds `t`, looking for `sphere`."""
    nodes, prim_idx = sc.export_bfs()
    rmin, rmax = sc.root()
    root_is_leaf = sc.info()["n_nodes"] == 1
    want = np.stack([_bits(t), np.asarray(sphere, np.uint32)], axis=1)
    out = dump("descend", depth, *f32_args(rmin), *f32_args(rmax), int(root_is_leaf), int(noslack),
               _file(dump, "nodes.u32", nodes, np.uint32), _file(dump, "idx.u32", prim_idx, np.uint32),
               _file(dump, "r.f32", rays), _file(dump, "q.f32", radii), _file(dump, "want.u32", want, np.uint32))
    rows = np.array([[int(v) for v in line.split()] for line in out.splitlines()], np.int64).reshape(-1, 2)
    assert len(rows) == len(rays)
    return rows[:, 0] == 1, rows[:, 1]


def _lost(dump, oracle, name, noslack=False):
    """(cast, flags) of the mix's answers that the descent does not reach, and
    how many answers there are."""
    sc = oracle.Scene(ov.spheres(name), None, **ov.TREES[name])
    rays, radii = sr.casts(name)
    lost, answers = [], 0
    for flags in (0, sr.ENTRY_ONLY):
        t, sphere = sr.expected(name, flags)
        hit = sphere != NO_HIT
        reached, _ = _descend(dump, sc, ov.TREES[name]["max_depth"], rays[hit], radii[hit], t[hit], sphere[hit],
                              noslack)
        lost += [(int(i), flags) for i in np.flatnonzero(hit)[~reached]]
        answers += int(hit.sum())
    sc.close()
    return lost, answers


@pytest.mark.parametrize("name", sr.SCENES)
def test_the_grown_cells_reach_a_leaf_of_every_answer(oracle, dump, name):
    """The pruning condition, no tolerance: for every cast of the mix with an
    answer, with and without ENTRY_ONLY, descending the oracle's tree by the
    header's grown-cell test reaches a leaf that lists the answering sphere.
    The bound is the answer's own t: the test is monotone in the bound, and
    the kernel's bound never falls below the answer's t, so this is the
    tightest bound it can hold.  F and G are 1000 units from the origin, and
    every mix has casts from 1280 units away."""
    lost, answers = _lost(dump, oracle, name)
    assert not lost, (name, lost[:8])
    assert answers >= (2 if name == "one" else 600), answers


def test_the_grown_cells_reach_a_leaf_of_every_answer_on_the_fuzz_scenes(oracle, dump):
    """The same condition on the 64 query_fuzz scenes (grown, non-cubic root
    boxes, radii over three decades, depths 1..8) with test_gpu_sweep_fuzz.py's
    casts, with and without ENTRY_ONLY."""
    total = 0
    for seed in range(SEEDS):
        c = query_case(seed)
        rays, radii = sr.fuzz_casts(c)
        sc = oracle_scene(oracle, c)
        for flags in (0, sr.ENTRY_ONLY):
            t, sphere = sr.reference(c["sp"], rays, radii, flags)
            hit = sphere != NO_HIT
            reached, _ = _descend(dump, sc, c["depth"], rays[hit], radii[hit], t[hit], sphere[hit])
            assert reached.all(), (seed, flags, np.flatnonzero(hit)[~reached][:8])
            total += int(hit.sum())
        sc.close()
    assert total > 20000, total


def test_the_slack_is_used(oracle, dump):
    """With the per-cast and the scene's slack at zero (the growth by R stays)
    the same descent loses answers on F or G: casts from 1280 units away, whose
    t is good to 6e-5 only, at spheres that end within 1e-5 of a cell face."""
    lost = {name: _lost(dump, oracle, name, noslack=True)[0] for name in ("F", "G")}
    print({k: len(v) for k, v in lost.items()})
    assert len(lost["F"]) + len(lost["G"]) >= 1


def test_scene_l_descent_follows_the_line(oracle, dump):
    """Scene L's cast crosses the root box obliquely in the sheet's z layer.  A
    line crosses at most 2^d + 2^(d-1) + 1 cells of depth d of its plane: 50
    records for depths 0 to 4.  Its bounding box holds a 16 x 8 block of the
    sheet's cells: 128 depth-4 records alone.  The header's descent, with the
    bound a miss keeps (tmax), reads no more than 64."""
    sp, ray, R = sr.l_scene()
    sc = oracle.Scene(sp, None, **sr.L_TREE)
    info = sc.info()
    _, nodes = _descend(dump, sc, sr.L_TREE["max_depth"], ray, np.full(1, R, np.float32), ray[:, 7],
                        np.full(1, NO_HIT, np.uint32))
    sc.close()
    print("scene L:", info, "records read:", int(nodes[0]))
    assert info["n_leaves"] == 256 and info["depth_reached"] == 4
    assert 16 <= nodes[0] <= 64
