"""CPU tests of the ray-query surface (rt_trace_rays, rt_pick): the header's
declarations and struct sizes, the ctypes mirror, the error path with no
renderer, and the C++ wrapper's new methods.  No GPU compute here; the
queries themselves are checked in tests/test_gpu_query.py."""
import ctypes
import os
import re
import shutil
import subprocess

from raytracingstudy_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")


def _header():
    src = open(os.path.join(INCLUDE, "rt.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_declares_the_query_entry_points():
    src = " ".join(_header().split())
    assert re.search(r"int rt_trace_rays\(rt_renderer\* r, const void\* dev_rays, uint32_t n, "
                     r"uint32_t kind, void\* dev_hits, void\* stream, rt_stats\* stats\);", src)
    assert re.search(r"int rt_pick\(rt_renderer\* r, float u, float v, rt_hit\* hit_out, "
                     r"float point_out\[3\]\);", src)
    assert re.search(r"#define RT_NO_HIT 0xFFFFFFFFu", src)
    assert re.search(r"RT_QUERY_NEAREST = 0,", src) and re.search(r"RT_QUERY_ANY = 1\b", src)
    assert re.search(r"#define RT_ABI_VERSION 4\b", src)  # additive: the version stays


def test_header_struct_sizes(tmp_path):
    """rt_ray is 32 bytes (two float4 loads a lane), rt_hit 8 (one dwordx2 store),
    as a C compiler lays them out."""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rt.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(rt_ray), '
                   'sizeof(rt_hit), offsetof(rt_ray, tmin), offsetof(rt_ray, dir), '
                   'offsetof(rt_ray, tmax), offsetof(rt_hit, t), offsetof(rt_hit, sphere)); '
                   'return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, "-o", str(exe), str(src)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [32, 8, 12, 16, 28, 0, 4]


def test_ctypes_structs_match_the_header():
    assert ctypes.sizeof(_lib.RtRay) == 32 and ctypes.sizeof(_lib.RtHit) == 8
    assert (_lib.RtRay.origin.offset, _lib.RtRay.tmin.offset, _lib.RtRay.dir.offset,
            _lib.RtRay.tmax.offset) == (0, 12, 16, 28)
    assert (_lib.RtHit.t.offset, _lib.RtHit.sphere.offset) == (0, 4)
    assert _lib.RT_NO_HIT == 0xFFFFFFFF and (_lib.RT_QUERY_NEAREST, _lib.RT_QUERY_ANY) == (0, 1)
    assert "rt_trace_rays" in _lib.SIGNATURES and "rt_pick" in _lib.SIGNATURES


def test_query_without_a_renderer_is_an_error_not_a_crash():
    """No GPU, hence no handle (rt_create fails): the calls report RT_E_INVALID
    and leave a message, whatever else they were given."""
    lib = _lib.load()
    rays = (_lib.RtRay * 1)()
    hits = (_lib.RtHit * 1)()
    hit = _lib.RtHit()
    assert lib.rt_trace_rays(None, None, 0, _lib.RT_QUERY_NEAREST, None, None, None) == _lib.RT_E_INVALID
    assert lib.rt_trace_rays(None, ctypes.addressof(rays), 1, _lib.RT_QUERY_ANY,
                             ctypes.addressof(hits), None, None) == _lib.RT_E_INVALID
    assert b"rt_trace_rays" in lib.rt_last_error(None)
    assert lib.rt_pick(None, 1.0, 2.0, ctypes.byref(hit), None) == _lib.RT_E_INVALID
    assert b"rt_pick" in lib.rt_last_error(None)


def test_cpp_wrapper_with_the_query_methods_compiles(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "no C++ compiler"
    src = tmp_path / "use_query.cpp"
    src.write_text('#include "rt_renderer.hpp"\n'
                   "bool use(rtamd::KernelRenderer& r, const void* rays, void* hits, void* stream) {\n"
                   "    rt_stats st;\n"
                   "    r.traceRays(rays, 4u, hits);\n"
                   "    r.traceRays(rays, 4u, hits, RT_QUERY_ANY, stream, &st);\n"
                   "    rt_hit h;\n"
                   "    float p[3];\n"
                   "    return r.pick(10.0f, 20.0f) && r.pick(1.0f, 2.0f, &h, p) && h.sphere != RT_NO_HIT;\n"
                   "}\n")
    r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", INCLUDE, str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
