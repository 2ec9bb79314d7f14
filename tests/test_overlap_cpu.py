"""CPU tests of the sphere-overlap query (rt_query_overlaps, rt_overlaps_at;
DESIGN.md 5.11): the surface (header, ctypes mirror, the error path with no
renderer, the C++ wrapper), the properties of the numpy reference the GPU
tests compare against (tests/overlap_ref.py), and the grown box's slack: no
accepted pair may lie outside every leaf the box-guided descent visits.  The
queries themselves run in test_gpu_overlap.py.
"""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from raytracingstudy_amd import _lib

import overlap_ref as ov

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")


# ---- surface ----------------------------------------------------------------
def _header():
    src = open(os.path.join(INCLUDE, "rt.h")).read()
    return " ".join(re.sub(r"/\*.*?\*/", "", src, flags=re.S).split())


def test_header_declares_the_overlap_entry_points():
    src = _header()
    assert "#define RT_OVERLAP_MAX 16" in src
    assert "#define RT_OVERLAP_MORE 0x80000000u" in src
    assert "enum { RT_OVERLAP_SKIP_SELF = 1u };" in src
    assert "typedef struct rt_probe { float center[3]; float radius; } rt_probe;" in src
    assert ("int rt_query_overlaps(rt_renderer* r, const void* dev_probes, uint32_t n, uint32_t k, "
            "uint32_t flags, void* dev_indices, void* dev_counts, void* stream, rt_stats* stats);") in src
    assert ("int rt_overlaps_at(rt_renderer* r, const float center[3], float radius, uint32_t k, "
            "uint32_t* indices_out, uint32_t* count_out);") in src
    assert re.search(r"#define RT_ABI_VERSION 4\b", src)  # additive: the version stays


def test_ctypes_mirror_matches_the_header():
    assert _lib.load().rt_abi_version() == 4
    assert (_lib.RT_OVERLAP_MAX, _lib.RT_OVERLAP_MORE, _lib.RT_OVERLAP_SKIP_SELF) == (16, 0x80000000, 1)
    assert ctypes.sizeof(_lib.RtProbe) == 16
    res, args = _lib.SIGNATURES["rt_query_overlaps"]
    assert res is ctypes.c_int and len(args) == 9
    assert args[2] is ctypes.c_uint32 and args[3] is ctypes.c_uint32 and args[4] is ctypes.c_uint32
    res, args = _lib.SIGNATURES["rt_overlaps_at"]
    assert res is ctypes.c_int and len(args) == 6 and args[2] is ctypes.c_float and args[3] is ctypes.c_uint32


def test_overlap_without_a_renderer_is_an_error_not_a_crash():
    """No GPU, hence no handle: both calls report RT_E_INVALID, name themselves
    and leave their outputs untouched."""
    lib = _lib.load()
    probes = (_lib.RtProbe * 1)()
    idx = (ctypes.c_uint32 * 4)(7, 7, 7, 7)
    cnt = ctypes.c_uint32(7)
    assert lib.rt_query_overlaps(None, None, 0, 1, 0, None, None, None, None) == _lib.RT_E_INVALID
    assert lib.rt_query_overlaps(None, ctypes.addressof(probes), 1, 4, 0, ctypes.addressof(idx),
                                 None, None, None) == _lib.RT_E_INVALID
    assert b"rt_query_overlaps" in lib.rt_last_error(None)
    c = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    assert lib.rt_overlaps_at(None, c, 0.1, 4, idx, ctypes.byref(cnt)) == _lib.RT_E_INVALID
    assert b"rt_overlaps_at" in lib.rt_last_error(None)
    assert cnt.value == 7 and list(idx) == [7, 7, 7, 7]  # untouched


def test_cpp_wrapper_with_the_overlap_methods_compiles(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "no C++ compiler"
    src = tmp_path / "use_overlap.cpp"
    src.write_text('#include "rt_renderer.hpp"\n'
                   "static_assert(sizeof(rt_probe) == 16, \"a scene sphere's layout\");\n"
                   "uint32_t use(rtamd::KernelRenderer& r, const void* probes, void* idx, void* counts,\n"
                   "             void* stream) {\n"
                   "    rt_stats st;\n"
                   "    r.queryOverlaps(probes, 4u, 3u, idx);\n"
                   "    r.queryOverlaps(probes, 4u, RT_OVERLAP_MAX, idx, counts, RT_OVERLAP_SKIP_SELF, stream, &st);\n"
                   "    const float c[3] = {0.5f, 0.5f, 0.5f};\n"
                   "    uint32_t out[4];\n"
                   "    bool more = false;\n"
                   "    return r.overlapsAt(c, 0.05f, 4u, out, &more) + r.overlapsAt(c, 0.0f, 4u, out);\n"
                   "}\n")
    r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", INCLUDE, str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---- the reference's properties -----------------------------------------------
def test_probe_mixes_are_not_vacuous():
    """From the reference alone: every scene's mix truncates at k = 16, has
    empty probes, and its far probes are all empty; D's contact probes have
    several members; B has a very large set."""
    for name in ("A", "B", "D"):
        total = ov.expected(name)[3]
        assert len(total) == ov.N_PROBES == 1024
        assert (total > 16).sum() >= 32, name
        assert (total == 0).sum() >= 64, name
        assert np.all(total[ov.FAR] == 0), name
    assert (ov.expected("D")[3][:ov.N_CONTACT] >= 3).sum() >= 200
    assert ov.expected("B")[3].max() > 1000


def test_reference_of_non_finite_and_negative_probes_is_empty():
    sp = ov.spheres("A")
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    c = sp[5, :3]
    pr = np.array([(*c, 0.0), (*c, -0.0), (*c, -1e-6), (*c, -1.0), (nan, c[1], c[2], 0.1),
                   (c[0], inf, c[2], 0.1), (c[0], c[1], -inf, 0.1), (*c, nan), (*c, inf), (*c, -inf)],
                  np.float32)
    idx, count, more, total = ov.reference(sp, pr, 4)
    assert 5 in idx[0] and 5 in idx[1] and total[0] == total[1] >= 1   # R = -0 is R = 0
    assert np.all(total[2:] == 0) and np.all(count[2:] == 0) and not more[2:].any()
    assert np.all(idx[2:] == ov.NO_HIT)


def test_reference_skip_self_removes_exactly_index_i():
    sp = ov.spheres("D")
    pr = ov.probes("D")
    plain, skip = ov.accepted(sp, pr), ov.accepted(sp, pr, skip_self=True)
    i = np.arange(len(pr))
    assert np.all(plain[i[:ov.N_CONTACT], i[:ov.N_CONTACT]])    # a sphere touches itself
    diff = plain != skip
    assert np.array_equal(np.argwhere(diff), np.argwhere(np.eye(len(pr), len(sp), dtype=bool) & plain))
    # fewer probes than spheres, and more: a probe past the last sphere skips nothing
    few = ov.accepted(sp[:100], pr, skip_self=True)
    assert np.array_equal(few[100:], ov.accepted(sp[:100], pr)[100:])


def test_scene_e_tangent_pairs_and_duplicates():
    """Exactly tangent pairs are accepted (the test is closed), the same probes
    one ulp further out are not, and a duplicate pair is reported twice."""
    sp = ov.spheres("E")
    pr, cases = ov.e_probes()
    acc = ov.accepted(sp, pr)
    tangent = [(p, j) for p, j, yes in cases if yes]
    moved = [(p, j) for p, j, yes in cases if not yes]
    assert len(tangent) >= 16 + 18 and len(moved) == len(tangent)
    assert all(acc[p, j] for p, j in tangent)
    assert not any(acc[p, j] for p, j in moved)
    # the tangent probes are tangent: d2 == s * s in f32 (not merely <=)
    for p, j in tangent[:16]:
        d = pr[p, :3] - sp[j, :3]
        s = pr[p, 3] + sp[j, 3]
        assert (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2] == s * s
    assert np.array_equal(sp[0], sp[18])
    assert np.array_equal(acc[:, 0], acc[:, 18]) and acc[:, 0].sum() >= 4
    idx = ov.reference(sp, sp[:1], 16)[0][0]   # sphere 0 as the probe: itself, its copy, 3 neighbours
    assert list(idx[:5]) == [0, 1, 3, 9, 18] and np.all(idx[5:] == ov.NO_HIT)


# ---- the header's arithmetic: predicate and grown box ---------------------------
@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    """tests/native/overlap_math_dump.cpp, a stand-alone program built with the
    address and undefined-behaviour sanitizers; a sanitizer report fails the test."""
    d = tmp_path_factory.mktemp("overlap_math")
    exe = str(d / "overlap_math_dump")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "overlap_math_dump.cpp")])

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


def test_numpy_reference_is_the_headers_predicate(dump):
    """rt_overlap_math.h's overlap_probe_ok and overlap_accepts, which the kernel
    runs, against the numpy restatement: scene A's mix, scene E's boundary
    probes and the non-finite ones, pair by pair."""
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    odd = np.array([(0.5, 0.5, 0.5, -0.0), (0.5, 0.5, 0.5, -1e-6), (nan, 0.5, 0.5, 0.1),
                    (0.5, inf, 0.5, 0.1), (0.5, 0.5, 0.5, inf), (0.5, 0.5, 0.5, nan)], np.float32)
    for name, pr in (("A", np.concatenate([ov.probes("A"), odd])), ("E", np.concatenate([ov.e_probes()[0], odd]))):
        sp = ov.spheres(name)
        out = dump("accepts", _file(dump, "p.f32", pr), _file(dump, "s.f32", sp)).split()
        got = np.array([[ch == "1" for ch in line] for line in out])
        assert np.array_equal(got, ov.accepted(sp, pr)), name


def _leaves(nodes, root_is_leaf):
    """(depth, cx, cy, cz, first ref, count) of every leaf of a tree in the
    product's record layout: children consecutive, valid ones only."""
    if root_is_leaf:
        return np.array([(0, 0, 0, 0, nodes[0, 0], nodes[0, 1])], np.int64)
    out, todo = [], [(0, 0, 0, 0, 0)]
    while todo:
        slot, d, cx, cy, cz = todo.pop()
        first, y = int(nodes[slot, 0]), int(nodes[slot, 1])
        valid, leafm = y & 0xFF, (y >> 8) & 0xFF
        k = 0
        for ch in range(8):
            if not valid & (1 << ch):
                continue
            c = (2 * cx + (ch & 1), 2 * cy + ((ch >> 1) & 1), 2 * cz + ((ch >> 2) & 1))
            if leafm & (1 << ch):
                out.append((d + 1, *c, int(nodes[first + k, 0]), int(nodes[first + k, 1])))
            else:
                todo.append((first + k, d + 1, *c))
            k += 1
    return np.array(out, np.int64)


def test_scene_g_pairs_are_accepted_from_above_the_mid_plane():
    sp, pr = ov.spheres("G"), ov.g_probes()
    assert np.array_equal(ov.accepted(sp, pr), np.eye(3, 4, dtype=bool))
    for a in range(3):   # the sphere ends below the plane, the probe's centre lies above it
        e = 1000.0 + (float(np.float32(1001.28)) - 1000.0) * 0.5
        assert float(sp[a, a]) + float(sp[a, 3]) < e - 5e-6 and e < float(pr[a, a])
        assert float(pr[a, a]) - float(pr[a, 3]) < e - 5e-6   # the probe's real reach ends below the plane too


@pytest.mark.parametrize("name", ["A", "D", "F", "G"])
def test_the_grown_box_reaches_a_leaf_of_every_accepted_pair(oracle, dump, name):
    """For every accepted (probe, sphere) pair of the 1024-probe mix, some leaf of
    the oracle's tree lists the sphere and has a cell the probe's grown box
    meets (lo < the cell's upper edge and hi >= its lower edge on every axis,
    in grid units: what the descent's mid-plane tests amount to).  A condition,
    no tolerance.  F is A far from the origin: there an ulp of a coordinate is
    far above the builders' margin; G's three pairs are made so that a box
    without the M term of the slack loses them (overlap_ref._g_scene).  The cells are the ones the builders' own double formula
    (scene_build.cpp: lo + ext * (c / cells)) lists the sphere in."""
    sp, pr = ov.spheres(name), ov.probes(name)
    if name == "G":
        pr = np.concatenate([ov.g_probes(), pr])
    tree = ov.TREES[name]
    D = tree["max_depth"]
    sc = oracle.Scene(sp, None, **tree)
    nodes, prim_idx = sc.export_bfs()
    rmin, rmax = sc.root()
    info = sc.info()
    sc.close()
    lv = _leaves(nodes, info["n_nodes"] == 1)
    assert len(lv) == info["n_leaves"] and lv[:, 5].sum() == info["n_prim_refs"] == len(prim_idx)
    order = np.argsort(lv[:, 4], kind="stable")   # references in leaf order
    assert np.array_equal(np.cumsum(lv[order, 5]) - lv[order, 5], lv[order, 4])
    ref_leaf = np.repeat(order, lv[order, 5])
    # the builders' double formula lists every reference's sphere in its cell
    lo, ext = rmin.astype(np.float64), rmax.astype(np.float64) - rmin.astype(np.float64)
    cells = (1 << lv[:, 0]).astype(np.float64)[:, None]
    blo = lo + ext * (lv[:, 1:4] / cells)
    bhi = lo + ext * ((lv[:, 1:4] + 1) / cells)
    c = sp[prim_idx, :3].astype(np.float64)
    e = np.maximum(np.maximum(blo[ref_leaf] - c, c - bhi[ref_leaf]), 0.0)
    r = sp[prim_idx, 3].astype(np.float64) + 1e-6 * ext.max()
    assert np.all((e * e).sum(axis=1) <= r * r)
    # the grown boxes, from the header
    from bins_native import f32_args
    rows = dump("box", D, *f32_args(rmin), *f32_args(rmax), _file(dump, "probes.f32", pr)).split()
    rows = np.array([int(t, 16) for t in rows], np.int64).reshape(len(pr), 7)
    ok = rows[:, 0] == 1
    box = rows[:, 1:].astype(np.uint32).view(np.float32).reshape(len(pr), 6)
    assert ok.all()
    size = (1 << (D - lv[:, 0]))
    cell_lo = (lv[:, 1:4] * size[:, None]).astype(np.float32)         # integers <= 2^16: exact
    cell_hi = ((lv[:, 1:4] + 1) * size[:, None]).astype(np.float32)
    acc = ov.accepted(sp, pr)
    pairs = 0
    for i in range(len(pr)):
        members = np.flatnonzero(acc[i])
        if not len(members):
            continue
        met = np.all((box[i, :3] < cell_hi) & (box[i, 3:] >= cell_lo), axis=1)
        reached = np.zeros(len(sp), bool)
        reached[prim_idx[met[ref_leaf]]] = True
        assert reached[members].all(), (name, i, members[~reached[members]])
        pairs += len(members)
    assert pairs > (4000 if name != "G" else 100)
