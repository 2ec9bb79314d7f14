"""CPU tests of the ordered multi-hit query (rt_trace_rays_multi, rt_pick_multi;
DESIGN.md 5.9).  They pin the brute-force reference the GPU tests compare
against (tests/multihit_ref.py) to the CPU oracle, and check the surface: the
header's declarations, the ctypes mirror, the error path with no renderer, and
the C++ wrapper's methods.  The queries themselves run in test_gpu_multihit.py.
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")


@pytest.mark.parametrize("name", ["A", "B", "D"])
def test_reference_k1_is_the_oracles_brute_force_nearest(oracle, name):
    """For k = 1 the reference is oracle.Scene.trace(brute=True) on every ray of
    the mix: hit flag, t bit for bit, sphere index."""
    sp, rays = mr.spheres(name), mr.rays(name)
    t, sphere, count = mr.cut(mr.expected(name), rays, 1)
    sc = oracle.Scene(sp, None, **mr.tree(name))
    hits = 0
    for i, r in enumerate(rays):
        h, th, idx, _ = sc.trace(r[0:3], r[4:7], r[3], r[7], brute=True)
        assert count[i] == (1 if h else 0), i
        if h:
            hits += 1
            assert sphere[i, 0] == idx, i
            assert t[i, 0].view(np.uint32) == np.float32(th).view(np.uint32), i
        else:
            assert sphere[i, 0] == mr.NO_HIT and t[i, 0].view(np.uint32) == r[7].view(np.uint32), i
    sc.close()
    assert 100 < hits < mr.N_RAYS  # both outcomes


def test_reference_full_sets_are_the_union_of_one_sphere_oracle_scenes(oracle):
    """On the first 48 spheres of the dense scene: every ray whose accepted set
    has fewer than 16 members has exactly the spheres that, alone in an oracle
    scene, are hit (brute force), at the same t bits, in (t, index) order."""
    sp, rays = mr.spheres("D")[:48], mr.rays("D")
    t, sphere, count, total = mr.reference(sp, rays, mr.K_MAX)
    singles = [oracle.Scene(s[None, :]) for s in sp]
    checked = multi = 0
    for i, r in enumerate(rays):
        if total[i] >= mr.K_MAX:
            continue
        exp = []
        for j, s in enumerate(singles):
            h, th, _, _ = s.trace(r[0:3], r[4:7], r[3], r[7], brute=True)
            if h:
                exp.append((np.float32(th), j))
        exp.sort()  # (t, index): no NaN among accepted t
        assert count[i] == total[i] == len(exp), i
        assert [int(x) for x in sphere[i, :len(exp)]] == [j for _, j in exp], i
        assert [int(x) for x in t[i, :len(exp)].view(np.uint32)] == [int(th.view(np.uint32)) for th, _ in exp], i
        assert np.all(sphere[i, len(exp):] == mr.NO_HIT), i
        assert np.all(t[i, len(exp):].view(np.uint32) == r[7].view(np.uint32)), i
        checked += 1
        multi += len(exp) >= 2
    for s in singles:
        s.close()
    # nearly every ray is checked; 48 spheres fill about 2% of the box, so only
    # a few rays cross two of them: enough to see an order
    assert checked > 900 and multi >= 8


def test_reference_of_non_finite_rays_is_empty():
    sp = mr.spheres("A")
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    rays = np.array([(0.64, 0.64, 3.0, 0.0, 0.0, 0.0, -1.0, inf),    # an ordinary hit
                     (0.64, 0.64, 3.0, 0.0, 0.0, 0.0, -inf, inf),
                     (0.64, inf, 3.0, 0.0, 0.0, 0.0, -1.0, inf),
                     (0.64, 0.64, 0.64, 0.0, nan, 0.6, 0.8, inf),
                     (0.64, 0.64, nan, 0.0, 0.6, 0.0, 0.8, 2.0)], np.float32)
    t, sphere, count, total = mr.reference(sp, rays, 4)
    assert count[0] >= 1 and sphere[0, 0] == 459
    assert np.all(count[1:] == 0) and np.all(total[1:] == 0) and np.all(sphere[1:] == mr.NO_HIT)
    assert np.array_equal(t[1:].view(np.uint32), np.repeat(rays[1:, 7:8], 4, 1).view(np.uint32))


def _header():
    src = open(os.path.join(INCLUDE, "rt.h")).read()
    return " ".join(re.sub(r"/\*.*?\*/", "", src, flags=re.S).split())


def test_header_declares_the_multihit_entry_points():
    src = _header()
    assert "#define RT_MULTIHIT_MAX 16" in src
    assert ("int rt_trace_rays_multi(rt_renderer* r, const void* dev_rays, uint32_t n, uint32_t k, "
            "void* dev_hits, void* dev_counts, void* stream, rt_stats* stats);") in src
    assert ("int rt_pick_multi(rt_renderer* r, float u, float v, uint32_t k, rt_hit* hits_out, "
            "uint32_t* count_out);") in src
    assert re.search(r"#define RT_ABI_VERSION 4\b", src)  # additive: the version stays


def test_ctypes_mirror_matches_the_header():
    assert _lib.RT_MULTIHIT_MAX == 16
    res, args = _lib.SIGNATURES["rt_trace_rays_multi"]
    assert res is ctypes.c_int and len(args) == 8 and args[2] is ctypes.c_uint32 and args[3] is ctypes.c_uint32
    res, args = _lib.SIGNATURES["rt_pick_multi"]
    assert res is ctypes.c_int and len(args) == 6 and args[3] is ctypes.c_uint32
    assert ctypes.sizeof(_lib.RtHit) == 8  # what dev_hits holds n*k of


def test_multihit_without_a_renderer_is_an_error_not_a_crash():
    """No GPU, hence no handle: the calls report RT_E_INVALID and leave a
    message, whatever else they were given."""
    lib = _lib.load()
    rays = (_lib.RtRay * 1)()
    hits = (_lib.RtHit * 4)()
    cnt = ctypes.c_uint32(7)
    assert lib.rt_trace_rays_multi(None, None, 0, 1, None, None, None, None) == _lib.RT_E_INVALID
    assert lib.rt_trace_rays_multi(None, ctypes.addressof(rays), 1, 4, ctypes.addressof(hits),
                                   None, None, None) == _lib.RT_E_INVALID
    assert b"rt_trace_rays_multi" in lib.rt_last_error(None)
    assert lib.rt_pick_multi(None, 1.0, 2.0, 4, hits, ctypes.byref(cnt)) == _lib.RT_E_INVALID
    assert b"rt_pick_multi" in lib.rt_last_error(None)
    assert cnt.value == 7  # untouched


def test_cpp_wrapper_with_the_multihit_methods_compiles(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "no C++ compiler"
    src = tmp_path / "use_multihit.cpp"
    src.write_text('#include "rt_renderer.hpp"\n'
                   "uint32_t use(rtamd::KernelRenderer& r, const void* rays, void* hits, void* counts,\n"
                   "             void* stream) {\n"
                   "    rt_stats st;\n"
                   "    r.traceRaysMulti(rays, 4u, 3u, hits);\n"
                   "    r.traceRaysMulti(rays, 4u, RT_MULTIHIT_MAX, hits, counts, stream, &st);\n"
                   "    rt_hit h[4];\n"
                   "    return r.pickMulti(10.0f, 20.0f, 4u, h);\n"
                   "}\n")
    r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", INCLUDE, str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
