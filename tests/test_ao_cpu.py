"""CPU tests of the ambient-occlusion layer (rt_render_ao): the
header's arithmetic (csrc/rt_ao_math.h through tests/native/ao_math_dump.cpp)
against tests/ao_ref.py bit for bit; the directions' properties from the
reference alone; the oracle's any-hit bit against its brute-force loop on every
AO ray test_gpu_ao.py compares; the main scene's coverage, so that a layer of
all ones, all zeros or the miss value cannot pass there; and the surface (header,
ctypes mirror, the error path with no renderer, the C++ wrapper).  The layer
itself runs in test_gpu_ao.py and test_gpu_ao_fuzz.py.
"""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from raytracingstudy_amd import _lib

import ao_ref as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
NO_HIT = ar.NO_HIT


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _unit(v):
    """float64 directions normalised, then rounded to float32 once."""
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


# ---- the header's arithmetic -----------------------------------------------------
@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    """tests/native/ao_math_dump.cpp, a stand-alone program built with the
    address and undefined-behaviour sanitizers; a sanitizer report fails the test."""
    d = tmp_path_factory.mktemp("ao_math")
    exe = str(d / "ao_math_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "ao_math_dump.cpp")])

    def run(*args):
        r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, r.stderr
        return r.stdout
    run.dir = d
    return run


def _cancelling_normal(k, pid, i):
    """A unit normal for which n + s nearly cancels: minus the sphere point s that
    direction i of pixel pid draws (recovered from the direction about n = 0)."""
    s, fb, _ = ar.directions(k, [pid], [i], np.zeros((1, 3), np.float32))
    # about a zero normal the direction is s / |s|: s itself to a rounding
    assert not fb[0]
    return -s[0]


def _tuples():
    """(normal (m, 3), pid (m,), i (m,), salt (m,)): 4096 random tuples, the six
    axis-aligned normals, normals of a sphere hit far from its centre's scale
    (not of unit length), and normals that nearly cancel their own s."""
    g = np.random.default_rng(515)
    m = 4096
    n = _unit(g.normal(size=(m, 3)))
    pid = g.integers(0, 1 << 21, m).astype(np.uint32)
    i = g.integers(0, 64, m).astype(np.uint32)
    salt = g.integers(0, 1 << 32, m, dtype=np.uint64).astype(np.uint32)
    salt[:512] = 0
    axes = np.concatenate([np.eye(3), -np.eye(3)]).astype(np.float32)
    n = np.concatenate([n, np.repeat(axes, 8, axis=0), n[:64] * np.float32(1.001)])
    pid = np.concatenate([pid, np.arange(48, dtype=np.uint32), pid[:64]])
    i = np.concatenate([i, np.arange(48, dtype=np.uint32) % 64, i[:64]])
    salt = np.concatenate([salt, np.zeros(48, np.uint32), salt[:64]])
    cn, cp, ci, cs = [], [], [], []
    for j in range(64):
        s = int(g.integers(0, 4))
        p_, i_ = int(g.integers(0, 408)), int(g.integers(0, 64))
        base = _cancelling_normal(ar.key(s), p_, i_)
        # the exact opposite, and neighbours a few 1e-4 away: some fall below 2^-20, some just above
        for scale in (0.0, 2e-4, 6e-4, 2e-3):
            cn.append(base + np.float32(scale) * g.normal(size=3).astype(np.float32))
            cp.append(p_), ci.append(i_), cs.append(s)
    n = np.concatenate([n, np.array(cn, np.float32)])
    pid = np.concatenate([pid, np.array(cp, np.uint32)])
    i = np.concatenate([i, np.array(ci, np.uint32)])
    salt = np.concatenate([salt, np.array(cs, np.uint32)])
    return n, pid, i, salt


def _ref_directions(n, pid, i, salt):
    d = np.zeros_like(n)
    fb = np.zeros(len(n), bool)
    for s in np.unique(salt):
        at = salt == s
        d[at], fb[at], _ = ar.directions(ar.key(int(s)), pid[at], i[at], n[at])
    return d, fb


def test_header_is_the_reference_bit_for_bit(dump):
    n, pid, i, salt = _tuples()
    rec = np.zeros(len(n), np.dtype([("n", np.float32, 3), ("pid", np.uint32), ("i", np.uint32), ("salt", np.uint32)]))
    rec["n"], rec["pid"], rec["i"], rec["salt"] = n, pid, i, salt
    path = str(dump.dir / "tuples.bin")
    rec.tofile(path)
    rows = np.array([[int(t, 16) for t in line.split()] for line in dump("dirs", ar.SEED, path).splitlines()],
                    np.int64)
    d, fb = _ref_directions(n, pid, i, salt)
    assert len(rows) == len(n) >= 4000
    assert np.array_equal(rows[:, :3].astype(np.uint32), _bits(d))
    assert np.array_equal(rows[:, 3] == 1, fb)
    # the cancelling normals did reach the |n + s|^2 < 2^-20 branch, and its other side
    tail = fb[-256:]
    assert 16 <= tail.sum() <= 240, int(tail.sum())
    assert np.array_equal(_bits(d[-256:][tail]), _bits(n[-256:][tail]))   # the fallback is n itself


def test_header_validity(dump):
    for rays in range(0, 130):
        assert dump("valid", rays, "3f800000")[0] == ("1" if rays in ar.RAYS else "0"), rays
    assert dump("valid", 0x80000000, "3f800000")[0] == "0"
    for radius, ok in ((0.1, 1), (np.inf, 1), (1e-38, 1), (0.0, 0), (-0.0, 0), (-1.0, 0), (-np.inf, 0), (np.nan, 0)):
        assert dump("valid", 16, "%08x" % _bits(np.float32(radius))[0])[1] == str(ok), radius


# ---- the directions' properties, from the reference alone ------------------------
@pytest.fixture(scope="module")
def cloud_of_directions():
    """2^16 directions: 1024 pixels x 64 rays, a random unit normal per pixel."""
    g = np.random.default_rng(77)
    n = np.repeat(_unit(g.normal(size=(1024, 3))), 64, axis=0)
    pid = np.repeat(np.arange(1024, dtype=np.uint32), 64)
    i = np.tile(np.arange(64, dtype=np.uint32), 1024)
    d, fb, drawn = ar.directions(ar.key(0), pid, i, n)
    return n, pid, i, d, fb, drawn


def test_directions_are_unit_and_in_the_hemisphere(cloud_of_directions):
    n, _, _, d, _, _ = cloud_of_directions
    d64, n64 = d.astype(np.float64), n.astype(np.float64)
    assert np.abs((d64 * d64).sum(axis=1) - 1.0).max() <= 2.0 ** -21
    assert ((d64 * n64).sum(axis=1) >= 0.0).all()


def test_directions_are_cosine_weighted(cloud_of_directions):
    """The mean of dir.n over 2^16 directions is 2/3 to 0.005: 5 sigma, with
    sigma = sqrt(1/18) / 256.  Under 1% fall back to the normal ((1 - pi/6)^8 =
    0.26%), and a direction takes 1.91 candidates on average (6 / pi)."""
    n, _, _, d, fb, drawn = cloud_of_directions
    mean = float((d.astype(np.float64) * n.astype(np.float64)).sum(axis=1).mean())
    print("mean dir.n", mean, "fallback", int(fb.sum()), "candidates", float(drawn.mean()))
    assert abs(mean - 2.0 / 3.0) <= 0.005
    assert fb.mean() < 0.01
    assert 1.8 <= drawn.mean() <= 2.0


def test_two_salts_share_no_direction_on_a_pixel(cloud_of_directions):
    n, pid, i, d, _, _ = cloud_of_directions
    for salt in (1, 2, 0xFFFFFFFF):
        d2, _, _ = ar.directions(ar.key(salt), pid, i, n)
        a = _bits(d).reshape(1024, 64, 3)
        b = _bits(d2).reshape(1024, 64, 3)
        # per pixel: no direction of one salt equals any direction of the other
        same = (a[:, :, None, :] == b[:, None, :, :]).all(axis=3)
        fb = (a == _bits(n).reshape(1024, 64, 3)).all(axis=2)     # the fallback is n under every salt
        assert not (same & ~fb[:, :, None]).any(), salt
    assert len({int(ar.key(s)[0]) for s in range(4096)}) == 4096


# ---- the oracle's bit against the brute force, on the GPU test's rays ----------------
# (case, rays, radius, salt): what test_gpu_ao.py compares
GPU_SETTINGS = ([(c, rays, radius, 0) for c in ("main", "small") for rays in (1, 4, 16, 64) for radius in ar.RADII]
                + [("small", rays, 0.1, 0) for rays in (2, 8, 32)]
                + [("main", 16, 0.1, salt) for salt in (1, 0xFFFFFFFF)]
                + [(c, 16, 0.1, 0) for c in ("inside", "away", "thin", "one", "empty")]
                + [("inside", 4, float("inf"), 0), ("one", 64, float("inf"), 0)])


@pytest.mark.parametrize("case", sorted(ar.CASES))
def test_oracle_bit_is_the_brute_force(oracle, case):
    sc = ar.oracle_scene(oracle, ar.CASES[case][0])
    total = 0
    for c, rays, radius, salt in GPU_SETTINGS:
        if c != case:
            continue
        e = ar.case_expected(oracle, c, rays, radius, salt)
        recs = e["rays"].reshape(-1, 8)
        assert np.array_equal(ar.brute_bits(sc, recs), e["bits"].reshape(-1)), (c, rays, radius, salt)
        total += len(recs)
    assert total > 0 or case in ("away", "empty")


# ---- coverage of the main scene ------------------------------------------------------
def _coverage(e, rays):
    hit = e["gbuffer"]["sphere"] != NO_HIT
    occ = e["occluded"]
    return dict(pixels=hit.size, hit=int(hit.sum()), partly=int(((occ > 0) & (occ < rays) & hit).sum()),
                fully=int(((occ == rays) & hit).sum()), unoccluded=int(((occ == 0) & hit).sum()))


def test_main_scene_is_not_vacuous(oracle):
    """From the reference alone, on the 408 pixels of `main`.  Measured:
      rays 16, radius 0.1   hit 247, partly 162, fully 0,  unoccluded 85
      rays 4,  radius inf   hit 247, partly 145, fully 41, unoccluded 61"""
    a = _coverage(ar.case_expected(oracle, "main", 16, 0.1), 16)
    b = _coverage(ar.case_expected(oracle, "main", 4, float("inf")), 4)
    print(a, b)
    assert a["pixels"] == 408
    assert 2 * a["hit"] >= a["pixels"] and 10 * (a["pixels"] - a["hit"]) >= a["pixels"]
    assert 2 * a["partly"] >= a["hit"] and 10 * a["unoccluded"] >= a["hit"]
    assert 20 * b["fully"] >= b["hit"]
    e = ar.case_expected(oracle, "main", 16, 0.1)
    assert (e["ao"][e["gbuffer"]["sphere"] == NO_HIT] == 1.0).all()
    assert np.array_equal(e["ao"], (16 - e["occluded"].astype(np.float64)) / 16)
    # the edge cases are what their names say
    inside = ar.case_expected(oracle, "inside", 16, 0.1)["gbuffer"]
    assert (inside["sphere"] != NO_HIT).all() and (inside["sphere"] == 0).sum() >= 8
    one = ar.case_expected(oracle, "one", 16, 0.1)
    assert (one["gbuffer"]["sphere"] == 0).sum() >= 8 and not one["occluded"].any()
    for name in ("away", "empty"):
        assert (ar.case_expected(oracle, name, 16, 0.1)["gbuffer"]["sphere"] == NO_HIT).all()
    assert 2 <= (ar.case_expected(oracle, "thin", 16, 0.1)["gbuffer"]["sphere"] != NO_HIT).sum() <= 15


# ---- surface -----------------------------------------------------------------------
def _header():
    src = open(os.path.join(INCLUDE, "rt.h")).read()
    return " ".join(re.sub(r"/\*.*?\*/", "", src, flags=re.S).split())


def test_header_declares_the_call():
    src = _header()
    assert ("typedef struct rt_ao_params { uint32_t rays; float radius; uint32_t salt; uint32_t flags; } "
            "rt_ao_params;") in src
    assert "typedef struct rt_ao_out { void* dev_ao; void* dev_occluded; } rt_ao_out;" in src
    assert ("int rt_render_ao(rt_renderer* r, const rt_ao_params* p, const rt_ao_out* out, void* stream, "
            "rt_stats* stats);") in src
    assert re.search(r"#define RT_ABI_VERSION 4\b", src)  # additive: the version stays


def test_ctypes_mirror_matches_the_header():
    lib = _lib.load()
    assert lib.rt_abi_version() == 4
    assert ctypes.sizeof(_lib.RtAoParams) == 16 and ctypes.sizeof(_lib.RtAoOut) == 16
    assert [f[0] for f in _lib.RtAoParams._fields_] == ["rays", "radius", "salt", "flags"]
    assert _lib.RtAoParams.radius.offset == 4 and _lib.RtAoOut.dev_occluded.offset == 8
    res, args = _lib.SIGNATURES["rt_render_ao"]
    assert res is ctypes.c_int and len(args) == 5
    assert args[1]._type_ is _lib.RtAoParams and args[2]._type_ is _lib.RtAoOut
    assert hasattr(lib, "rt_render_ao")


def test_render_ao_without_a_renderer_is_an_error_not_a_crash():
    lib = _lib.load()
    p = _lib.RtAoParams(16, 0.1, 0, 0)
    o = _lib.RtAoOut(None, None)
    assert lib.rt_render_ao(None, ctypes.byref(p), ctypes.byref(o), None, None) == _lib.RT_E_INVALID
    assert b"rt_render_ao" in lib.rt_last_error(None)


def test_cpp_wrapper_with_render_ao_compiles(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "no C++ compiler"
    src = tmp_path / "use_ao.cpp"
    src.write_text('#include <cmath>\n#include "rt_renderer.hpp"\n'
                   "uint64_t use(rtamd::KernelRenderer& r, void* ao, void* occ, void* stream) {\n"
                   "    rt_stats st;\n"
                   "    r.renderAO(16u, 0.1f, ao);\n"
                   "    r.renderAO(64u, INFINITY, nullptr, occ, 7u, stream, &st);\n"
                   "    static_assert(sizeof(rt_ao_params) == 16 && sizeof(rt_ao_out) == 16, \"the ABI's sizes\");\n"
                   "    return st.shadow_rays;\n"
                   "}\n")
    r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", INCLUDE, str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
