"""CPU tests of the closest-sphere query (rt_query_closest, rt_closest_at;
DESIGN.md 5.12): the surface (header, ctypes mirror, the error path with no
renderer, the C++ wrapper), the properties of the numpy reference the GPU
tests compare against (tests/closest_ref.py), the header's key against that
reference bit for bit, and the grown box's slack: no sphere of an answer may
lie outside every leaf that a descent bounded by its key visits.  The queries
themselves run in test_gpu_closest.py and test_gpu_closest_fuzz.py.
"""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from raytracingstudy_amd import _lib

import closest_ref as cr
import overlap_ref as ov
from bins_native import f32_args
from plain_fuzz import SEEDS, oracle_scene
from query_fuzz import query_case
from test_overlap_cpu import _leaves

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")


# ---- surface ----------------------------------------------------------------
def _header():
    src = open(os.path.join(INCLUDE, "rt.h")).read()
    return " ".join(re.sub(r"/\*.*?\*/", "", src, flags=re.S).split())


def test_header_declares_the_closest_entry_points():
    src = _header()
    assert "#define RT_CLOSEST_MAX 16" in src
    assert "enum { RT_CLOSEST_SKIP_SELF = 1u };" in src
    assert "typedef struct rt_near { float dist; uint32_t sphere; } rt_near;" in src
    assert ("int rt_query_closest(rt_renderer* r, const void* dev_probes, uint32_t n, uint32_t k, "
            "uint32_t flags, void* dev_near, void* dev_counts, void* stream, rt_stats* stats);") in src
    assert ("int rt_closest_at(rt_renderer* r, const float point[3], float max_dist, uint32_t k, "
            "rt_near* near_out, uint32_t* count_out);") in src
    assert re.search(r"#define RT_ABI_VERSION 4\b", src)  # additive: the version stays
    # the header says that this is not rt_query_overlaps' set
    text = " ".join(open(os.path.join(INCLUDE, "rt.h")).read().replace("*", " ").split())
    assert "not rt_query_overlaps' set" in text


def test_ctypes_mirror_matches_the_header():
    assert _lib.load().rt_abi_version() == 4
    assert (_lib.RT_CLOSEST_MAX, _lib.RT_CLOSEST_SKIP_SELF) == (16, 1)
    assert ctypes.sizeof(_lib.RtNear) == 8
    assert [f for f, _ in _lib.RtNear._fields_] == ["dist", "sphere"]
    res, args = _lib.SIGNATURES["rt_query_closest"]
    assert res is ctypes.c_int and len(args) == 9
    assert args[2] is ctypes.c_uint32 and args[3] is ctypes.c_uint32 and args[4] is ctypes.c_uint32
    res, args = _lib.SIGNATURES["rt_closest_at"]
    assert res is ctypes.c_int and len(args) == 6 and args[2] is ctypes.c_float and args[3] is ctypes.c_uint32


def test_closest_without_a_renderer_is_an_error_not_a_crash():
    """No GPU, hence no handle: both calls report RT_E_INVALID, name themselves
    and leave their outputs untouched."""
    lib = _lib.load()
    probes = (_lib.RtProbe * 1)()
    near = (_lib.RtNear * 4)()
    for s in near:
        s.dist, s.sphere = 7.0, 7
    cnt = ctypes.c_uint32(7)
    assert lib.rt_query_closest(None, None, 0, 1, 0, None, None, None, None) == _lib.RT_E_INVALID
    assert lib.rt_query_closest(None, ctypes.addressof(probes), 1, 4, 0, ctypes.addressof(near),
                                None, None, None) == _lib.RT_E_INVALID
    assert b"rt_query_closest" in lib.rt_last_error(None)
    c = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    assert lib.rt_closest_at(None, c, 0.1, 4, near, ctypes.byref(cnt)) == _lib.RT_E_INVALID
    assert b"rt_closest_at" in lib.rt_last_error(None)
    assert cnt.value == 7 and [(s.dist, s.sphere) for s in near] == [(7.0, 7)] * 4  # untouched


def test_cpp_wrapper_with_the_closest_methods_compiles(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "no C++ compiler"
    src = tmp_path / "use_closest.cpp"
    src.write_text('#include <cmath>\n#include "rt_renderer.hpp"\n'
                   "static_assert(sizeof(rt_near) == 8 && sizeof(rt_near) == sizeof(rt_hit), \"a hit's layout\");\n"
                   "uint32_t use(rtamd::KernelRenderer& r, const void* probes, void* near, void* counts,\n"
                   "             void* stream) {\n"
                   "    rt_stats st;\n"
                   "    r.queryClosest(probes, 4u, 3u, near);\n"
                   "    r.queryClosest(probes, 4u, RT_CLOSEST_MAX, near, counts, RT_CLOSEST_SKIP_SELF, stream, &st);\n"
                   "    const float p[3] = {0.5f, 0.5f, 0.5f};\n"
                   "    rt_near out[4];\n"
                   "    return r.closestAt(p, INFINITY, 4u, out) + r.closestAt(p, 0.05f, 1u, out);\n"
                   "}\n")
    r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", INCLUDE, str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---- the reference's properties -----------------------------------------------
def test_probe_mixes_are_not_vacuous():
    """From the reference alone, per 1024-probe mix: probes with an empty set,
    with more than 16 members (the answer is truncated) and with 1..16 (fillers
    follow the answer); negative keys (a probe inside a sphere); on E, equal
    keys among the answers (exact ties, and the duplicate sphere).  Measured:
      A  270 / 361 / 393, 513 negative, 0 tied     D  132 / 362 / 530, 664 negative
      B  157 / 371 / 496, 514 negative             E  297 / 341 / 386, 532 negative, 407 tied"""
    for name in ("A", "B", "D"):
        got = cr.mix_counts(cr.expected(name))
        assert got["empty"] + got["truncated"] + got["partial"] == ov.N_PROBES, name
        assert got["empty"] >= 100 and got["truncated"] >= 300 and got["partial"] >= 300, (name, got)
        assert got["negative"] >= 300, (name, got)
    assert cr.mix_counts(cr.expected("E"))["tied"] >= 300
    # the three radius classes are all there, and an unbounded probe lists min(16, n) spheres
    pr = cr.probes("A")
    assert np.isinf(pr[1::3, 3]).all() and np.all(pr[2::3, 3] == cr.CUTOFF) and np.all(pr[0::3, 3] < 1.0)
    assert np.all(cr.expected("A")[2][1::3] == 16)


def test_reference_order_fillers_and_odd_probes():
    sp = ov.spheres("A")
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    c = sp[5, :3]
    pr = np.array([(*c, 0.0), (*c, -0.0), (*c, inf), (*c, -1e-6), (*c, -1.0), (nan, c[1], c[2], 0.1),
                   (c[0], inf, c[2], 0.1), (c[0], c[1], -inf, inf), (*c, nan), (*c, -inf),
                   (1e20, 0.0, 0.0, inf), (1e20, 0.0, 0.0, 1e30)], np.float32)
    dist, sphere, count, total = cr.reference(sp, pr, 4)
    assert sphere[0, 0] == 5 and dist[0, 0] == -sp[5, 3]              # the centre: key = -r
    assert np.array_equal(sphere[0], sphere[1]) and total[0] == total[1] >= 1   # R = -0 is R = 0
    assert total[2] == len(sp) and count[2] == 4
    assert np.all(np.diff(dist[2]) >= 0)
    assert np.all(total[3:10] == 0) and np.all(sphere[3:10] == cr.NO_HIT)
    # every slot of an empty probe holds its radius as given, bit for bit
    assert np.array_equal(dist[3:10].view(np.uint32), np.repeat(pr[3:10, 3:4], 4, axis=1).view(np.uint32))
    assert np.signbit(dist[1, count[1]:]).all()   # (-0 stays -0)
    # d2 overflows: every key is +inf, all accepted by R = +inf, the k smallest indices; none by a finite R
    assert total[10] == len(sp) and list(sphere[10]) == [0, 1, 2, 3] and np.all(np.isinf(dist[10]))
    assert total[11] == 0
    # skip_self removes exactly sphere i from probe i
    own = np.array(sp[:8])
    own[:, 3] = inf
    plain, skip = cr.reference(sp, own, 4), cr.reference(sp, own, 4, skip_self=True)
    for i in range(8):
        assert i in plain[1][i] and i not in skip[1][i]
        assert [s for s in plain[1][i] if s != i][:3] == list(skip[1][i][:3])


def test_scene_e_ties_are_ordered_by_index_and_the_duplicate_is_listed_twice():
    sp = ov.spheres("E")
    assert np.array_equal(sp[0], sp[18])
    dist, sphere, count, total = cr.expected("E")
    held = sphere != cr.NO_HIT
    tie = (dist[:, 1:] == dist[:, :-1]) & held[:, 1:]
    assert np.all(sphere[:, 1:][tie] > sphere[:, :-1][tie])
    whole = total <= 16
    has0 = (sphere == 0).any(axis=1)
    assert (has0 & whole).sum() >= 4 and np.array_equal(has0[whole], (sphere == 18).any(axis=1)[whole])
    rows = np.flatnonzero(has0 & whole)   # equal keys, 18 after 0 (other spheres of that key in between)
    at0, at18 = np.argmax(sphere[rows] == 0, axis=1), np.argmax(sphere[rows] == 18, axis=1)
    assert np.all(at18 > at0) and np.array_equal(dist[rows, at18], dist[rows, at0])


# ---- the header's arithmetic: key and grown box ---------------------------------
@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    """tests/native/closest_math_dump.cpp, a stand-alone program built with the
    address and undefined-behaviour sanitizers; a sanitizer report fails the test."""
    d = tmp_path_factory.mktemp("closest_math")
    exe = str(d / "closest_math_dump")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "closest_math_dump.cpp")])

    def run(*args):
        r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, r.stderr
        return r.stdout
    run.dir = d
    return run


def _file(dump, name, a):
    path = str(dump.dir / name)
    np.ascontiguousarray(a, np.float32).tofile(path)
    return path


def test_numpy_reference_is_the_headers_key(dump):
    """rt_closest_math.h's closest_probe_ok and closest_key, which the kernel
    runs, against the numpy restatement, bit for bit: scene A's and E's mixes
    and the odd probes (non-finite, -0, negative, a d2 that overflows)."""
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    odd = np.array([(0.5, 0.5, 0.5, -0.0), (0.5, 0.5, 0.5, -1e-6), (nan, 0.5, 0.5, 0.1), (0.5, inf, 0.5, 0.1),
                    (0.5, 0.5, -inf, inf), (0.5, 0.5, 0.5, inf), (0.5, 0.5, 0.5, -inf), (0.5, 0.5, 0.5, nan),
                    (1e20, 0.5, 0.5, inf), (-3e38, 3e38, 0.5, 1.0)], np.float32)
    for name in ("A", "E"):
        sp = ov.spheres(name)
        pr = np.concatenate([cr.probes(name), odd])
        rows = np.array([[int(t, 16) for t in line.split()]
                         for line in dump("keys", _file(dump, "p.f32", pr), _file(dump, "s.f32", sp)).splitlines()],
                        np.int64)
        assert rows.shape == (len(pr), 1 + len(sp))
        assert np.array_equal(rows[:, 0] == 1, cr.probe_ok(pr)), name
        ok = cr.probe_ok(pr)   # (a non-finite centre's keys may be NaN, whose payload is not specified)
        assert np.array_equal(rows[ok, 1:].astype(np.uint32), cr.keys(sp, pr[ok]).view(np.uint32)), name
    assert list(cr.probe_ok(odd)) == [True, False, False, False, False, True, False, False, True, True]


def _members_reached(dump, sp, pr, ref, nodes, prim_idx, rmin, rmax, depth, root_is_leaf):
    """For every sphere among every probe's answers, whether the header's box at
    max(key, 0) meets the cell of some leaf that lists the sphere (a cell is
    met unless lo >= its upper edge or hi < its lower edge on some axis, in
    grid units: what the descent's mid-plane tests amount to).  Returns the
    (probe, sphere) pairs that are not reached and the number checked."""
    lv = _leaves(nodes, root_is_leaf)
    assert lv[:, 5].sum() == len(prim_idx)
    order = np.argsort(lv[:, 4], kind="stable")   # references in leaf order
    assert np.array_equal(np.cumsum(lv[order, 5]) - lv[order, 5], lv[order, 4])
    ref_leaf = np.repeat(order, lv[order, 5])
    size = 1 << (depth - lv[:, 0])
    cell_lo = (lv[:, 1:4] * size[:, None]).astype(np.float32)         # integers <= 2^16: exact
    cell_hi = ((lv[:, 1:4] + 1) * size[:, None]).astype(np.float32)
    by_sphere = np.argsort(prim_idx, kind="stable")
    first = np.searchsorted(prim_idx[by_sphere], np.arange(len(sp) + 1))
    dist, sphere = ref[0], ref[1]
    pi, slot = np.nonzero(sphere != cr.NO_HIT)
    rec = np.concatenate([pr[pi, :3], dist[pi, slot][:, None]], axis=1)
    rows = dump("box", depth, *f32_args(rmin), *f32_args(rmax), _file(dump, "pairs.f32", rec)).split()
    box = np.array([int(t, 16) for t in rows], np.int64).astype(np.uint32).view(np.float32).reshape(len(rec), 6)
    sph = sphere[pi, slot].astype(np.int64)
    missed = []
    for s in np.unique(sph):
        leaves = ref_leaf[by_sphere[first[s]:first[s + 1]]]
        assert len(leaves), s
        q = np.flatnonzero(sph == s)
        step = max(1, 2_000_000 // len(leaves))
        for a in range(0, len(q), step):
            b = box[q[a:a + step]]
            met = np.all(~(b[:, None, :3] >= cell_hi[None, leaves]) & ~(b[:, None, 3:] < cell_lo[None, leaves]),
                         axis=2)
            missed += [(int(pi[j]), int(s)) for j in q[a:a + step][~met.any(axis=1)]]
    return missed, len(rec)


@pytest.mark.parametrize("name", ["A", "D", "F", "G"])
def test_the_grown_box_reaches_a_leaf_of_every_answer(oracle, dump, name):
    """The pruning condition, no tolerance: for every probe of the mix and every
    sphere among its 16 answers, the box of the sphere's own key reaches a leaf
    that lists it.  The box is monotone in the bound, and the descent's bound
    never falls below the key of a sphere that belongs in the answer, so this
    covers every bound the descent can hold.  F is A far from the origin, G's
    probes (overlap_ref.g_probes, unbounded here) sit 3 ulps above a plane
    their sphere ends below."""
    sp, pr = ov.spheres(name), cr.probes(name)
    if name == "G":
        pr = np.concatenate([cr.with_cutoffs(ov.g_probes()), np.array(ov.g_probes()), pr])
    tree = ov.TREES[name]
    sc = oracle.Scene(sp, None, **tree)
    nodes, prim_idx = sc.export_bfs()
    rmin, rmax = sc.root()
    info = sc.info()
    sc.close()
    ref = cr.reference(sp, pr, 16)
    missed, pairs = _members_reached(dump, sp, pr, ref, nodes, prim_idx, rmin, rmax, tree["max_depth"],
                                     info["n_nodes"] == 1)
    assert not missed, (name, missed[:8])
    assert pairs > (6000 if name != "G" else 1000), pairs


def test_the_grown_box_reaches_a_leaf_of_every_answer_on_the_fuzz_scenes(oracle, dump):
    """The same condition on the 64 query_fuzz scenes (grown, non-cubic root
    boxes, radii over three decades, depths 1..8), their 520 probes with the
    mix's radius substitution, k = 16."""
    total = 0
    for seed in range(SEEDS):
        c = query_case(seed)
        pr = cr.with_cutoffs(c["probes"])
        sc = oracle_scene(oracle, c)
        nodes, prim_idx = sc.export_bfs()
        rmin, rmax = sc.root()
        info = sc.info()
        sc.close()
        ref = cr.reference(c["sp"], pr, 16)
        missed, pairs = _members_reached(dump, c["sp"], pr, ref, nodes, prim_idx, rmin, rmax, c["depth"],
                                         info["n_nodes"] == 1)
        assert not missed, (seed, missed[:8])
        total += pairs
    assert total > 60000, total
