"""CPU tests of the one-bounce diffuse layer (rt_render_indirect, rt_add_layer;
DESIGN.md 5.18): the header's arithmetic (csrc/rt_indirect_math.h through
tests/native/indirect_math_dump.cpp) against tests/indirect_ref.py bit for bit;
the reference's colour of a ray pinned to the oracle's own frames; the oracle's
nearest hit against its brute-force loop on the main case's bounce rays; what
the layer must be on a lone sphere under a black sky; its w against ao_ref's ao;
and the surface (header, ctypes mirror, the error path with no renderer, the C++
wrapper).  The layer itself runs in test_gpu_indirect.py and
test_gpu_indirect_fuzz.py.
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
import indirect_ref as ir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
NO_HIT = ir.NO_HIT
INF = float("inf")
NAN_WORD = np.uint32(0x7FC00000)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _canon(words):
    """uint32 words of float32 values with every NaN replaced by one NaN word: which
    operand's payload an addition of two NaNs keeps is the compiler's choice."""
    w = np.array(words, np.uint32)
    w[np.isnan(w.view(np.float32))] = NAN_WORD
    return w


# ---- the header's arithmetic -----------------------------------------------------
@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    """tests/native/indirect_math_dump.cpp, a stand-alone program built with the
    address and undefined-behaviour sanitizers; a sanitizer report fails the test."""
    d = tmp_path_factory.mktemp("indirect_math")
    exe = str(d / "indirect_math_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "indirect_math_dump.cpp")])

    def run(*args):
        r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, r.stderr
        return r.stdout
    run.dir = d
    return run


def _rows(text):
    return np.array([[int(t, 16) for t in line.split()] for line in text.splitlines()], np.int64).astype(np.uint32)


def _hex(x):
    return "%08x" % _bits(np.float32(x))[0]


def test_header_validity(dump):
    for rays in list(range(0, 70)) + [128, 0x80000000]:
        got = dump("valid", rays, _hex(1.0), _hex(1.0), 0)
        ok = ir.params_ok(rays, 1.0, 1.0)
        assert got[0] == str(int(ok[1])) and got[3] == str(int(ok[0])), rays
    for radius in (0.1, np.inf, 1e-38, 0.0, -0.0, -1.0, -np.inf, np.nan):
        got = dump("valid", 4, _hex(radius), _hex(1.0), 0)
        ok = ir.params_ok(4, radius, 1.0)
        assert got[1] == str(int(ok[2])) and got[3] == str(int(ok[0])), radius
    for sky, want in ((0.0, 1), (-0.0, 1), (0.5, 1), (1.0, 1), (3e38, 1), (1e-45, 1), (-1e-45, 0), (-1.0, 0),
                      (np.inf, 0), (-np.inf, 0), (np.nan, 0)):
        got = dump("valid", 4, _hex(0.1), _hex(sky), 0)
        ok = ir.params_ok(4, 0.1, sky)
        assert ok[3] == bool(want), sky
        assert got[2] == str(want) and got[3] == str(want), sky
    for flags in (1, 2, 0x80000000):
        assert dump("valid", 4, _hex(0.1), _hex(1.0), flags).strip() == "1110"
    assert dump("valid", 4, _hex(0.1), _hex(1.0), 0).strip() == "1111"


def test_header_sky_colour_is_the_reference(dump):
    g = np.random.default_rng(1801)
    d = g.normal(size=(2048, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True).astype(np.float32)
    d[:8, 1] = (0.0, -0.0, 1.0, -1.0, 1.5, np.nan, np.inf, -np.inf)
    d[8:16, 2] = (0.0, -0.0, 1.0, -1.0, 1.5, np.nan, np.inf, -np.inf)
    for sky in (0.0, 0.5, 1.0, 3.25):
        rec = np.zeros(len(d), np.dtype([("dy", np.float32), ("dz", np.float32), ("sky", np.float32)]))
        rec["dy"], rec["dz"], rec["sky"] = d[:, 1], d[:, 2], sky
        path = str(dump.dir / "sky.bin")
        rec.tofile(path)
        assert np.array_equal(_canon(_rows(dump("sky", path))), _canon(_bits(ir.sky_color(d, sky)))), sky
    assert np.array_equal(_bits(ir.sky_color(d[16:], 1.0))[:, 0], np.full(len(d) - 16, _bits(np.float32(200.0) / np.float32(255.0))[0]))


def test_header_hit_colour_is_the_reference(dump):
    g = np.random.default_rng(1802)
    m = 4096
    al = g.integers(0, 1 << 32, m, dtype=np.uint64).astype(np.uint32)
    al[:4] = (0, 0xFFFFFFFF, 0xFFCCCCCC, 0x00010203)
    amb = g.uniform(0.0, 1.0, m).astype(np.float32)
    amb[:8] = (0.0, 1.0, 0.1, 0.0, 1.0, 0.1, 0.5, 0.25)
    lam = g.uniform(0.0, 1.0, m).astype(np.float32)
    lam[:8] = (0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1e-30, 0.99999994)
    rec = np.zeros(m, np.dtype([("al", np.uint32), ("amb", np.float32), ("lam", np.float32)]))
    rec["al"], rec["amb"], rec["lam"] = al, amb, lam
    path = str(dump.dir / "hit.bin")
    rec.tofile(path)
    exp = np.concatenate([ir.hit_color(al[i:i + 1], amb[i], lam[i:i + 1]) for i in range(m)])
    assert np.array_equal(_rows(dump("hit", path)), _bits(exp))


@pytest.mark.parametrize("rays", ar.RAYS)
def test_header_ordered_sum_is_the_reference(dump, rays):
    """Values of mixed magnitude (the sum's order shows in the last bits), all-equal
    ones, and records with a NaN or an infinity among them."""
    g = np.random.default_rng(1803 + rays)
    m = 512
    v = (g.normal(size=(m, rays)) * 10.0 ** g.uniform(-6, 6, (m, rays))).astype(np.float32)
    v[0] = 1.0
    v[1] = np.float32(0.1)
    v[2:34, :] = np.abs(v[2:34, :])
    v[40, g.integers(0, rays)] = np.nan
    v[41, g.integers(0, rays)] = np.inf
    v[42, 0] = np.inf
    v[42, rays - 1] = -np.inf if rays > 1 else np.inf
    path = str(dump.dir / f"sum{rays}.bin")
    v.tofile(path)
    got = _rows(dump("sum", rays, path))
    ts = ir.tree_sum(v)
    assert got.shape == (m, rays + 1)
    assert np.array_equal(_canon(got[:, :rays]), _canon(_bits(ts)))
    assert np.array_equal(_canon(got[:, rays]), _canon(_bits(ir.mean_of(ts[:, 0], rays))))
    assert np.isnan(ts[40, 0]) and (rays == 1 or np.isnan(ts[42, 0]))
    if rays >= 8:  # the pairing is not the left-to-right sum: some record tells them apart
        seq = v[:34, 0].copy()
        for i in range(1, rays):
            seq = seq + v[:34, i]
        assert (_bits(seq) != _bits(ts[:34, 0])).any()
    for hits in range(rays + 1):
        assert int(dump("open", rays, hits), 16) == _bits(ir.open_share(rays, hits)).reshape(-1)[0]


def test_header_add_layer_pixel_is_the_reference(dump):
    """Random pixels, layers and albedos with and without the albedo, gains 0, 1 and
    others, and layers holding NaN, +-inf, negative and huge values."""
    g = np.random.default_rng(1804)
    m = 4096
    px = g.integers(0, 1 << 32, m, dtype=np.uint64).astype(np.uint32)
    al = g.integers(0, 1 << 32, m, dtype=np.uint64).astype(np.uint32)
    lay = g.uniform(-0.25, 1.25, (m, 3)).astype(np.float32)
    special = np.array([np.nan, np.inf, -np.inf, -1.0, 0.0, -0.0, 1e30, -1e30, 1e-30, 1.0, 0.5, 3.4e38], np.float32)
    lay[:len(special) * 3] = np.repeat(special, 3)[:, None]
    has = g.integers(0, 2, m).astype(np.uint32)
    gain = g.choice(np.array([0.0, 1.0, 0.5, 2.0, 0.003, 100.0], np.float32), m).astype(np.float32)
    gain[:len(special) * 3] = np.tile(np.array([0.0, 1.0, 2.5], np.float32), len(special))
    rec = np.zeros(m, np.dtype([("px", np.uint32), ("lay", np.float32, 3), ("al", np.uint32), ("has", np.uint32),
                                ("gain", np.float32)]))
    rec["px"], rec["lay"], rec["al"], rec["has"], rec["gain"] = px, lay, al, has, gain
    assert rec.dtype.itemsize == 28
    path = str(dump.dir / "add.bin")
    rec.tofile(path)
    got = _rows(dump("add", path)).reshape(-1)
    exp = np.zeros(m, np.uint32)
    rgba = px.view(np.uint8).reshape(m, 1, 4)
    for i in range(m):
        out = ir.add_layer(rgba[i:i + 1], np.concatenate([lay[i], [7.0]]).astype(np.float32).reshape(1, 1, 4),
                           al[i:i + 1].reshape(1, 1) if has[i] else None, gain[i])
        exp[i] = out.view(np.uint32).reshape(-1)[0]
    assert np.array_equal(got, exp)
    assert np.array_equal(got >> 24, px >> 24)                       # alpha kept
    nan_rows = np.isnan(lay[:, 0]) | ((gain == 0) & np.isinf(lay[:, 0]))
    assert nan_rows.sum() >= 4 and not (got[nan_rows] & 0xFFFFFF).any()   # a NaN stores 0
    zero = (gain == 0) & np.isfinite(lay).all(axis=1)
    assert zero.sum() >= 100 and np.array_equal(got[zero], px[zero])      # gain 0 changes nothing


# ---- the reference's colour of a ray, pinned to the oracle's frames -----------------
@pytest.mark.parametrize("shadows,light,ambient", [(True, ir.LIGHT, ir.AMBIENT), (False, ir.LIGHT, ir.AMBIENT),
                                                   (True, (-0.3, 0.8, 0.5), 0.35), (False, (-0.3, 0.8, 0.5), 0.35)])
def test_colour_of_a_ray_is_the_oracles_frame(oracle, shadows, light, ambient):
    """An unjittered 1-spp 9x9 frame's radiance equals color_of_ray on the camera's
    rays (tmax = +inf, sky_scale = 1) word for word."""
    scene, pname, w, h = ar.CASES["small"]
    sp, al = ar.spheres(scene)
    sc = ar.oracle_scene(oracle, scene)
    P, K = ar.pose(pname), ar.intrinsic(oracle, "small")
    _, rad, cnt = sc.render(w, h, P, K, spp=1, jitter=False, shadows=shadows, light_dir=light, ambient=ambient,
                            radiance=True)
    o = np.asarray(P, np.float32).reshape(4, 4)[3, :3]
    L = ir.light_toward(light)
    kinds = set()
    cast = 0
    for y in range(h):
        for x in range(w):
            d = oracle.get_ray(P, K, float(x), float(y))
            c, kind, _, _, _, n, _, _ = ir.color_of_ray(sc, sp, al, o, d, INF, L, ambient, shadows, 1.0)
            assert np.array_equal(_bits(c), _bits(rad[y, x, :3])), (x, y, kind)
            kinds.add(kind)
            cast += n
    assert cast == int(cnt[0]) + int(cnt[1])
    assert {ir.ESCAPED, ir.LIT, ir.AWAY} <= kinds and ((ir.SHADOWED in kinds) == shadows)


def test_bounce_hits_of_main_are_the_brute_force(oracle):
    e = ir.case_expected(oracle, "main", 4, INF)
    sc = ar.oracle_scene(oracle, "cloud")
    recs = e["rays"].reshape(-1, 8)
    t, s = e["hit_t"].reshape(-1), e["hit_sphere"].reshape(-1)
    assert len(recs) >= 4 * 200
    for r, th, sh in zip(recs, t, s):
        hit, tb, ib, _ = sc.trace(r[0:3], r[4:7], float(r[3]), float(r[7]), brute=True)
        assert hit == (sh != NO_HIT)
        if hit:
            assert (_bits(np.float32(tb))[0], ib) == (_bits(th)[0], sh)
    # and the case is not vacuous: every kind of bounce ray, pixels that mix sky and hits
    kinds = e["kind"]
    for k in (ir.ESCAPED, ir.LIT, ir.SHADOWED, ir.AWAY):
        assert (kinds == k).sum() >= 20, k
    mixed = ((kinds == ir.ESCAPED).any(axis=1) & (kinds != ir.ESCAPED).any(axis=1)).sum()
    assert mixed >= 50
    assert len(e["shadow_rays"]) == ((kinds == ir.LIT) | (kinds == ir.SHADOWED)).sum()


def test_one_sphere_under_a_black_sky_receives_nothing(oracle):
    """A convex body sees none of itself: every bounce ray escapes, so with
    sky_scale = 0 a hit pixel's layer is {0, 0, 0, 1}, and so is a miss pixel's."""
    e = ir.case_expected(oracle, "one", 16, INF, sky_scale=0.0)
    assert len(e["pixel"]) >= 8 and (e["kind"] == ir.ESCAPED).all()
    assert np.array_equal(_bits(e["layer"]), _bits(np.broadcast_to(np.float32([0, 0, 0, 1]), e["layer"].shape)))
    assert not e["occluded"].any()
    lit = ir.case_expected(oracle, "one", 16, INF, sky_scale=1.0)["layer"]
    assert (lit[..., 0].reshape(-1)[e["pixel"]] > 0.78).all()        # the sky's red, 200/255


@pytest.mark.parametrize("rays", ar.RAYS)
def test_w_is_the_ao_layer(oracle, rays):
    e = ir.case_expected(oracle, "small", rays, 0.1)
    a = ar.case_expected(oracle, "small", rays, 0.1)
    assert np.array_equal(_bits(e["layer"][..., 3]), _bits(a["ao"]))
    assert np.array_equal(e["occluded"], a["occluded"])
    assert np.array_equal(_bits(e["rays"]), _bits(a["rays"]))


# ---- surface -----------------------------------------------------------------------
def _header():
    src = open(os.path.join(INCLUDE, "rt.h")).read()
    return " ".join(re.sub(r"/\*.*?\*/", "", src, flags=re.S).split())


def test_header_declares_the_calls():
    src = _header()
    assert ("typedef struct rt_indirect_params { uint32_t rays; float radius; uint32_t salt; float sky_scale; "
            "uint32_t flags; } rt_indirect_params;") in src
    assert "typedef struct rt_indirect_out { void* dev_layer; void* dev_occluded; } rt_indirect_out;" in src
    assert ("int rt_render_indirect(rt_renderer* r, const rt_indirect_params* p, const rt_indirect_out* out, "
            "void* stream, rt_stats* stats);") in src
    assert ("int rt_add_layer(rt_renderer* r, void* dev_rgba8, const void* dev_layer4, const void* dev_albedo, "
            "float gain, void* stream);") in src
    assert re.search(r"#define RT_ABI_VERSION 4\b", src)  # additive: the version stays


def test_ctypes_mirror_matches_the_header():
    lib = _lib.load()
    assert lib.rt_abi_version() == 4
    assert ctypes.sizeof(_lib.RtIndirectParams) == 20 and ctypes.sizeof(_lib.RtIndirectOut) == 16
    assert [f[0] for f in _lib.RtIndirectParams._fields_] == ["rays", "radius", "salt", "sky_scale", "flags"]
    assert _lib.RtIndirectParams.sky_scale.offset == 12 and _lib.RtIndirectOut.dev_occluded.offset == 8
    res, args = _lib.SIGNATURES["rt_render_indirect"]
    assert res is ctypes.c_int and len(args) == 5
    assert args[1]._type_ is _lib.RtIndirectParams and args[2]._type_ is _lib.RtIndirectOut
    res, args = _lib.SIGNATURES["rt_add_layer"]
    assert res is ctypes.c_int and len(args) == 6 and args[4] is ctypes.c_float
    assert hasattr(lib, "rt_render_indirect") and hasattr(lib, "rt_add_layer")


def test_calls_without_a_renderer_are_errors_not_crashes():
    lib = _lib.load()
    p = _lib.RtIndirectParams(4, 0.1, 0, 1.0, 0)
    o = _lib.RtIndirectOut(None, None)
    assert lib.rt_render_indirect(None, ctypes.byref(p), ctypes.byref(o), None, None) == _lib.RT_E_INVALID
    assert b"rt_render_indirect" in lib.rt_last_error(None)
    assert lib.rt_add_layer(None, None, None, None, 1.0, None) == _lib.RT_E_INVALID
    assert b"rt_add_layer" in lib.rt_last_error(None)


def test_cpp_wrapper_with_render_indirect_compiles(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "no C++ compiler"
    src = tmp_path / "use_indirect.cpp"
    src.write_text('#include <cmath>\n#include "rt_renderer.hpp"\n'
                   "uint64_t use(rtamd::KernelRenderer& r, void* layer, void* occ, void* albedo, void* stream) {\n"
                   "    rt_stats st;\n"
                   "    r.renderIndirect(4u, 0.1f, layer);\n"
                   "    r.renderIndirect(64u, INFINITY, nullptr, occ, 7u, 0.5f, stream, &st);\n"
                   "    r.addLayer(layer);\n"
                   "    r.addLayer(layer, 2.0f, albedo, nullptr, stream);\n"
                   "    static_assert(sizeof(rt_indirect_params) == 20 && sizeof(rt_indirect_out) == 16, \"the ABI's sizes\");\n"
                   "    return st.shadow_rays;\n"
                   "}\n")
    r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", INCLUDE, str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
