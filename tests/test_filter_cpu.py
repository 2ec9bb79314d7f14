"""CPU tests of the guide-driven layer filter (rt_filter_layer, rt_apply_layer;
DESIGN.md 5.16): the header's arithmetic and plan (csrc/rt_filter_math.h through
tests/native/filter_math_dump.cpp) against tests/filter_ref.py bit for bit; the
reference's own properties; whether the filter at its defaults does what it is
for (a 4-ray AO layer closer to a converged one than unfiltered); and the
surface (header, ctypes mirror, the error path with no renderer, the C++
wrapper).  The kernels run in test_gpu_filter.py.
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
import filter_ref as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
NO_HIT = fr.NO_HIT
INF = np.float32(np.inf)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _hex(x):
    return "%08x" % _bits(np.float32(x)).reshape(-1)[0]


# ---- the header's arithmetic -----------------------------------------------------
@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    """tests/native/filter_math_dump.cpp, a stand-alone program built with the
    address and undefined-behaviour sanitizers; a sanitizer report fails the test."""
    d = tmp_path_factory.mktemp("filter_math")
    exe = str(d / "filter_math_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "filter_math_dump.cpp")])

    def run(*args):
        r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, r.stderr
        return r.stdout
    run.dir = d
    return run


def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def _weight_grid():
    """Records {k, n_p, n_q, t_p, t_q, sigma, normal_power}: every pair of 14
    normals (random unit ones, an axis and its opposite, a zero normal, one of
    length 1.001, a NaN one) x 10 depth pairs (equal, near, far, t_p tiny, huge, and
    a denormal pair whose sigma * t_p underflows: iz = +inf, e = 0 * inf, a NaN weight) x
    sigma (0.05, 1e-3, +inf) x every normal_power, under a few kernel entries."""
    g = np.random.default_rng(2030)
    rnd = _unit(g.normal(size=(8, 3)))
    normals = np.concatenate([rnd, [[0, 0, 1], [0, 0, -1], [0, 0, 0]], rnd[:1] * np.float32(1.001),
                              -rnd[1:2], [[np.nan, 0, 1]]]).astype(np.float32)
    depths = np.array([(1.0, 1.0), (1.0, 1.01), (1.0, 1.05), (2.5, 0.3), (1e-30, 1e-30), (1e-30, 1.0),
                       (1e-38, 2e-38), (3e38, 1.0), (0.7, 0.7000001), (1e-44, 1e-44)], np.float32)
    sigmas = np.array([0.05, 1e-3, np.inf], np.float32)
    ks = np.array([K1 * K2 for K1 in fr.K for K2 in fr.K], np.float32)
    rows = []
    for a in range(len(normals)):
        for b in range(len(normals)):
            for d in range(len(depths)):
                for s in sigmas:
                    for p in range(8):
                        rows.append((ks[(a + b + d + p) % len(ks)], normals[a], normals[b], depths[d, 0], depths[d, 1],
                                     s, p))
    rec = np.zeros(len(rows), np.dtype([("k", np.float32), ("n_p", np.float32, 3), ("n_q", np.float32, 3),
                                        ("t_p", np.float32), ("t_q", np.float32), ("sigma", np.float32),
                                        ("np", np.uint32)]))
    for name, col in zip(rec.dtype.names, zip(*rows)):
        rec[name] = np.array(col)
    assert rec.dtype.itemsize == 44
    return rec


def test_header_weight_is_the_reference_bit_for_bit(dump):
    rec = _weight_grid()
    path = str(dump.dir / "weights.bin")
    rec.tofile(path)
    rows = np.array([[int(t, 16) for t in line.split()] for line in dump("weights", path).splitlines()], np.int64)
    assert len(rows) == len(rec) >= 40000
    iz = np.zeros(len(rec), np.float32)
    w = np.zeros(len(rec), np.float32)
    for s in np.unique(rec["sigma"]):
        for p in range(8):
            at = (rec["sigma"] == s) & (rec["np"] == p)
            iz[at] = fr.inv_depth(s, rec["t_p"][at])
            w[at] = fr.weight(rec["k"][at], rec["n_p"][at], rec["n_q"][at], rec["t_p"][at], rec["t_q"][at], iz[at], p)

    def same(got, want):   # bit for bit; every NaN is one value (its payload is the platform's)
        got = got.astype(np.uint32).view(np.float32)
        return (_bits(got) == _bits(want)) | (np.isnan(got) & np.isnan(want))
    assert same(rows[:, 0], iz).all()
    assert same(rows[:, 1], w).all()
    # the grid reaches what it names: antiparallel and zero normals weigh 0, sigma = +inf drops the depth term
    assert (iz[rec["sigma"] == INF] == 0).all()
    anti = (rec["n_p"] == -rec["n_q"]).all(axis=1) & (rec["n_p"] != 0).any(axis=1)
    assert anti.sum() >= 100 and (w[anti & ~np.isnan(w)] == 0).all()
    assert np.isnan(w).sum() >= 100 and (w[~np.isnan(w)] >= 0).all() and (w > 0).sum() >= 10000
    flat = ((rec["sigma"] == INF) & (rec["np"] == 0) & ~np.isnan(w) & (rec["t_p"] < 1e38)
            & ~np.isnan(rec["n_p"]).any(axis=1) & ~np.isnan(rec["n_q"]).any(axis=1))
    dn = (rec["n_p"][flat].astype(np.float64) * rec["n_q"][flat]).sum(axis=1)
    assert np.allclose(w[flat], rec["k"][flat] * np.maximum(dn, 0), rtol=1e-5, atol=1e-7)


def test_header_taps_validity_and_plan(dump):
    taps = [int(t, 16) for t in dump("taps").split()]
    assert taps == [int(_bits(fr.K[abs(o)]).reshape(-1)[0]) for o in range(-2, 3)]
    assert float(sum(fr.K[abs(o)] for o in range(-2, 3))) == 1.0       # the B3 spline row sums to 1 exactly

    def valid(passes=3, channels=1, sigma=0.05, npow=5, flags=0):
        return dump("valid", passes, channels, _hex(sigma), npow, flags).strip()
    assert valid() == "11111"
    for passes in range(0, 9):
        ok = 1 <= passes <= 5
        assert valid(passes=passes) == ("11111" if ok else "00111"), passes
    assert valid(passes=0xFFFFFFFF)[:2] == "00"
    for channels in (0, 2, 3, 5, 8):
        assert valid(channels=channels) == "01011", channels
    assert valid(channels=4) == "11111"
    for sigma, ok in ((0.05, 1), (np.inf, 1), (1e-38, 1), (0.0, 0), (-0.0, 0), (-1.0, 0), (-np.inf, 0), (np.nan, 0)):
        assert valid(sigma=sigma) == ("11111" if ok else "01101"), sigma
    for npow in range(0, 12):
        assert valid(npow=npow) == ("11111" if npow <= 7 else "01110"), npow
    for flags in (1, 2, 0x80000000):
        assert valid(flags=flags) == "01111", flags
    for floor, ok in ((0.0, 1), (-0.0, 1), (0.25, 1), (1.0, 1), (1.0000001, 0), (-1e-9, 0), (np.nan, 0), (np.inf, 0)):
        assert dump("floor", _hex(floor)).strip() == str(ok), floor

    code = {"in": 0, "out": 1, "scratch": 2}
    for passes in range(1, 6):
        lines = dump("plan", passes).splitlines()
        rows = [tuple(int(t) for t in ln.split()) for ln in lines[:-1]]
        want = fr.plan(passes)
        assert rows == [(step, code[src], code[dst]) for step, src, dst in want]
        assert lines[-1] == ("1" if passes >= 2 else "0")
        # the plan's own sense: steps double, the input is only read, each pass reads what the
        # last one wrote and never its own destination, and the last pass writes the output
        assert [r[0] for r in rows] == [1 << s for s in range(passes)]
        assert rows[0][1] == 0 and rows[-1][2] == 1
        for s, (_, src, dst) in enumerate(rows):
            assert dst in (1, 2) and src != dst
            assert s == 0 or src == rows[s - 1][2]


@pytest.mark.parametrize("w,h,channels,passes,npow,sigma", [(31, 23, 1, 3, 5, 0.05), (5, 3, 4, 5, 0, np.inf),
                                                            (37, 29, 4, 2, 5, np.inf), (1, 1, 1, 5, 7, 0.05),
                                                            (40, 7, 1, 4, 2, 0.01)])
def test_header_filter_on_the_host_is_the_reference(dump, w, h, channels, passes, npow, sigma):
    """The specification's loops over the header's functions and plan, run on the
    host, give the reference's words on random guides: the tap order, the skipped
    taps, the copy of a miss and the buffers' alternation."""
    sphere, t, n = _guides(h, w, 10 * w + h)
    g = np.random.default_rng(w)
    v = g.random((h, w) if channels == 1 else (h, w, 4)).astype(np.float32)
    path = str(dump.dir / f"layer_{w}_{h}.bin")
    with open(path, "wb") as f:
        np.array([w, h, channels, passes, npow], np.uint32).tofile(f)
        np.array([sigma], np.float32).tofile(f)
        for a in (sphere, t, n, v):
            a.tofile(f)
    words = np.array([int(x, 16) for x in dump("layer", path).split()], np.int64).astype(np.uint32)
    want = fr.filter_layer(v, sphere, t, n, passes, sigma, npow)
    assert np.array_equal(words.reshape(v.shape), _bits(want))
    assert (sphere != NO_HIT).sum() < 2 or not np.array_equal(_bits(want), _bits(v))


# ---- the reference's own properties ----------------------------------------------
def _guides(h, w, seed, miss_share=0.3):
    """Random guides: unit normals, depths around 1 with jumps, some pixels missed."""
    g = np.random.default_rng(seed)
    sphere = g.integers(0, 50, (h, w)).astype(np.uint32)
    sphere[g.random((h, w)) < miss_share] = NO_HIT
    hit = sphere != NO_HIT
    t = np.where(hit, (1.0 + 0.2 * g.random((h, w)) + (g.random((h, w)) < 0.2)).astype(np.float32), INF)
    n = np.zeros((h, w, 4), np.float32)
    n[hit, :3] = _unit(g.normal(size=(int(hit.sum()), 3)) + [0, 0, 2.0])
    return sphere, t.astype(np.float32), n


@pytest.mark.parametrize("channels", [1, 4])
def test_a_layer_of_ones_stays_ones(channels):
    """w * 1 = w makes the two sums the same number, so the quotient is 1.0f for any guides."""
    sphere, t, n = _guides(23, 31, 1)
    one = np.ones((23, 31) if channels == 1 else (23, 31, 4), np.float32)
    for passes in (1, 3, 5):
        for npow, sigma in ((5, 0.05), (0, np.inf)):
            out = fr.filter_layer(one, sphere, t, n, passes, sigma, npow)
            assert np.array_equal(_bits(out), _bits(one))


def test_miss_pixels_are_copied_and_never_contribute():
    sphere, t, n = _guides(19, 27, 2)
    hit = sphere != NO_HIT
    g = np.random.default_rng(3)
    v = g.random((19, 27)).astype(np.float32)
    out = fr.filter_layer(v, sphere, t, n, 3, np.inf, 0)
    assert np.array_equal(_bits(out[~hit]), _bits(v[~hit]))
    assert (out[hit] != v[hit]).mean() > 0.9                      # the hit pixels did get filtered
    # whatever the miss pixels hold, NaN included, no hit pixel's output moves
    v2 = v.copy()
    v2[~hit] = np.where(g.random((~hit).sum()) < 0.5, np.nan, 1e30).astype(np.float32)
    out2 = fr.filter_layer(v2, sphere, t, n, 3, np.inf, 0)
    assert np.array_equal(_bits(out2[hit]), _bits(out[hit]))
    assert np.array_equal(_bits(out2[~hit]), _bits(v2[~hit]))
    # garbage guides (a NaN depth) copy the value: sw > 0 is false for a NaN
    t3 = t.copy()
    t3[hit] = np.nan
    out3 = fr.filter_layer(v, sphere, t3, n, 2, 0.05, 5)
    assert np.array_equal(_bits(out3), _bits(v))


def test_tiny_images():
    """A one-pixel image returns its input (its centre tap alone: sv / sw = v up to
    the one rounding of w * v / w, none for these values), and 5 passes on 5x3 work
    with every off-image tap skipped."""
    one = np.array([[0.625]], np.float32)
    for sphere in (7, NO_HIT):
        out = fr.filter_layer(one, np.array([[sphere]], np.uint32), np.array([[1.5]], np.float32),
                              np.array([[[0, 0, 1, 0]]], np.float32), 5, 0.05, 5)
        assert out.shape == (1, 1) and np.array_equal(_bits(out), _bits(one))
    sphere, t, n = _guides(3, 5, 4, miss_share=0.0)
    v = np.random.default_rng(5).random((3, 5, 4)).astype(np.float32)
    out = fr.filter_layer(v, sphere, t, n, 5, np.inf, 0)
    assert out.shape == v.shape and np.isfinite(out).all()
    assert out.min() >= v.min() - 1e-6 and out.max() <= v.max() + 1e-6      # convex combinations
    # passes 4 and 5 (steps 8 and 16) reach no neighbour on 5x3: each is the identity up to a rounding
    out3 = fr.filter_layer(v, sphere, t, n, 3, np.inf, 0)
    assert np.abs(out - out3).max() <= 4 * 2.0 ** -24
    # with no edges the filter is the plain B3 blur: a constant layer is a fixed point, a ramp keeps its mean inside
    flat = np.full((3, 5), 0.3, np.float32)
    assert np.abs(fr.filter_layer(flat, sphere, t, n, 5, np.inf, 0) - flat).max() <= 2.0 ** -24


def test_apply_layer_reference():
    g = np.random.default_rng(6)
    px = g.integers(0, 256, (4, 5, 4)).astype(np.uint8)
    layer = g.random((4, 5)).astype(np.float32)
    assert np.array_equal(fr.apply_layer(px, layer, 1.0), px)                  # m = 1 exactly
    assert np.array_equal(fr.apply_layer(px, np.ones_like(layer), 0.25), px)   # 0.25 + 0.75 * 1
    dark = fr.apply_layer(px, np.zeros_like(layer), 0.0)
    assert not dark[..., :3].any() and np.array_equal(dark[..., 3], px[..., 3])
    half = fr.apply_layer(px, np.full_like(layer, 0.5), 0.0)
    assert np.array_equal(half[..., :3], px[..., :3] // 2)                    # truncation
    out = fr.apply_layer(px, layer, 0.25)
    assert (out[..., :3] <= px[..., :3]).all() and np.array_equal(out[..., 3], px[..., 3])


# ---- what the filter is for --------------------------------------------------------
def test_filtered_4_ray_layer_is_nearer_the_converged_one(oracle):
    """The `small` AO case at radius 0.1.  Target: the 64-ray layer averaged over 8
    salts (512 rays a pixel).  Measure: the mean absolute error over hit pixels.
    The 4-ray layer filtered at the defaults must be strictly nearer the target
    than the unfiltered one.  Measured: unfiltered 0.08804, filtered 0.08162 (40 hit
    pixels of 81)."""
    case, radius = "small", 0.1
    target = np.mean([ar.case_expected(oracle, case, 64, radius, salt)["ao"].astype(np.float64)
                      for salt in range(8)], axis=0)
    e = ar.case_expected(oracle, case, 4, radius)
    g = e["gbuffer"]
    hit = g["sphere"] != NO_HIT
    raw = e["ao"]
    flt = fr.filter_layer(raw, g["sphere"], g["t"], g["normal"], **fr.DEFAULTS)
    err_raw = float(np.abs(raw.astype(np.float64) - target)[hit].mean())
    err_flt = float(np.abs(flt.astype(np.float64) - target)[hit].mean())
    print("hit pixels", int(hit.sum()), "of", hit.size, "MAE unfiltered", err_raw, "filtered", err_flt)
    assert hit.sum() >= 20 and err_raw > 0.0
    assert err_flt < err_raw


# ---- surface -----------------------------------------------------------------------
def _header():
    src = open(os.path.join(INCLUDE, "rt.h")).read()
    return " ".join(re.sub(r"/\*.*?\*/", "", src, flags=re.S).split())


def test_header_declares_the_calls():
    src = _header()
    assert ("typedef struct rt_filter_params { uint32_t passes; uint32_t channels; float depth_sigma; "
            "uint32_t normal_power; uint32_t flags; } rt_filter_params;") in src
    assert "void rt_filter_params_default(rt_filter_params*);" in src
    assert ("int rt_filter_layer(rt_renderer* r, const rt_filter_params* p, const rt_gbuffer* guides, "
            "const void* dev_in, void* dev_out, void* stream, rt_stats* stats);") in src
    assert ("int rt_apply_layer(rt_renderer* r, void* dev_rgba8, const void* dev_layer, float floor, "
            "void* stream);") in src
    assert re.search(r"#define RT_ABI_VERSION 4\b", src)  # additive: the version stays


def test_ctypes_mirror_and_defaults():
    lib = _lib.load()
    assert lib.rt_abi_version() == 4
    assert ctypes.sizeof(_lib.RtFilterParams) == 20
    assert [f[0] for f in _lib.RtFilterParams._fields_] == ["passes", "channels", "depth_sigma", "normal_power",
                                                            "flags"]
    assert _lib.RtFilterParams.depth_sigma.offset == 8 and _lib.RtFilterParams.flags.offset == 16
    res, args = _lib.SIGNATURES["rt_filter_layer"]
    assert res is ctypes.c_int and len(args) == 7
    assert args[1]._type_ is _lib.RtFilterParams and args[2]._type_ is _lib.RtGBuffer
    res, args = _lib.SIGNATURES["rt_apply_layer"]
    assert res is ctypes.c_int and len(args) == 5 and args[3] is ctypes.c_float
    p = _lib.RtFilterParams(9, 9, 9.0, 9, 9)
    lib.rt_filter_params_default(ctypes.byref(p))
    assert (p.passes, p.channels, p.normal_power, p.flags) == (3, 1, 5, 0)
    assert _bits(np.float32(p.depth_sigma)) == _bits(np.float32(0.05))
    assert (p.passes, float(np.float32(p.depth_sigma)), p.normal_power) == (
        fr.DEFAULTS["passes"], float(np.float32(fr.DEFAULTS["depth_sigma"])), fr.DEFAULTS["normal_power"])
    lib.rt_filter_params_default(None)   # tolerated


def test_calls_without_a_renderer_are_errors_not_crashes():
    lib = _lib.load()
    p = _lib.RtFilterParams(3, 1, 0.05, 5, 0)
    g = _lib.RtGBuffer(None, None, None)
    assert lib.rt_filter_layer(None, ctypes.byref(p), ctypes.byref(g), None, None, None, None) == _lib.RT_E_INVALID
    assert b"rt_filter_layer" in lib.rt_last_error(None)
    assert lib.rt_apply_layer(None, None, None, 0.0, None) == _lib.RT_E_INVALID
    assert b"rt_apply_layer" in lib.rt_last_error(None)


def test_cpp_wrapper_with_the_layer_calls_compiles(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "no C++ compiler"
    src = tmp_path / "use_filter.cpp"
    src.write_text('#include <cmath>\n#include "rt_renderer.hpp"\n'
                   "float use(rtamd::KernelRenderer& r, const void* in, void* out, const void* hits, const void* nrm,\n"
                   "          void* pbo, void* stream) {\n"
                   "    rt_stats st;\n"
                   "    r.filterLayer(in, out, hits, nrm);\n"
                   "    r.filterLayer(in, out, hits, nrm, 5u, 4u, INFINITY, 0u, stream, &st);\n"
                   "    r.applyLayer(out);\n"
                   "    r.applyLayer(out, 0.25f, pbo, stream);\n"
                   "    rt_filter_params p;\n"
                   "    rt_filter_params_default(&p);\n"
                   "    static_assert(sizeof(rt_filter_params) == 20, \"the ABI's size\");\n"
                   "    return st.ms + p.depth_sigma;\n"
                   "}\n")
    r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", INCLUDE, str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
