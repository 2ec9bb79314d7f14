"""The ambient-occlusion layer (rt_render_ao) against tests/ao_ref.py, pixel by pixel.

The kernel walks pixel (x, y)'s centre ray like the G-buffer, builds each AO
ray in registers (csrc/rt_ao_math.h) and walks it any-hit, so every pixel's
occluded count, its ao value (bit for bit) and the four counters must equal
the reference: oracle.get_ray + oracle.Scene.trace for the hit, the origin,
normal and directions restated in numpy float32, oracle.Scene.trace(...,
any_hit=True) per AO ray.  Every output buffer is pre-filled with 0xAB bytes
and is one record longer than the frame: an unwritten pixel and a write past
the end both show.  The expectation of a case is computed once and shared
(ao_ref.case_expected).
"""
import ctypes

import numpy as np
import pytest

import raytracingstudy_amd as rt
from raytracingstudy_amd import _lib

import ao_ref as ar

pytestmark = pytest.mark.gpu

NO_HIT = ar.NO_HIT
INF = float("inf")


def _renderer(oracle, case, **kw):
    scene, pname, w, h = ar.CASES[case]
    sp, al = ar.spheres(scene)
    r = rt.KernelRenderer(w, h, mode="scene", **kw)
    r.resize(w, h)
    r.setIntrinsic(ar.intrinsic(oracle, case))
    r.setPosition(ar.pose(pname))
    r.set_scene(sp, al, **ar.TREE)
    return r


def _run(r, w, h, rays, radius, salt=0, ao=True, occluded=True, stream=None, stats=False):
    """rt_render_ao into 0xAB-filled buffers of w*h + 1 records; the guard record
    of each must come back untouched."""
    import torch
    n = w * h
    bufs = {k: torch.full((n + 1, 4), 0xAB, dtype=torch.uint8, device="cuda")
            for k, on in (("ao", ao), ("occluded", occluded)) if on}
    if stream is None:
        torch.cuda.synchronize()
    ptr = {k: bufs[k].data_ptr() if k in bufs else None for k in ("ao", "occluded")}
    st = r.render_ao_device(rays, radius, ptr["ao"], ptr["occluded"], salt, stream=stream, stats=stats)
    if stream is None:
        r.synchronize()
    out = {"stats": st}
    for k, b in bufs.items():
        raw = b.cpu().numpy()  # on a caller's stream: ordered after the launch
        assert (raw[n] == 0xAB).all(), k
        out[k] = raw[:n].copy().view(np.uint32).reshape(h, w)   # ao: its bits
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_equal(got, exp, ao=True, occluded=True):
    if occluded:
        assert np.array_equal(got["occluded"], exp["occluded"])
    if ao:
        assert np.array_equal(got["ao"], _bits(exp["ao"]))   # bit for bit: a sentinel word never is one


def _assert_stats(st, exp, w, h):
    assert st.primary_rays == w * h and st.shadow_rays == exp["ao_rays"]
    assert (st.nodes_visited, st.prims_tested) == (exp["nodes"], exp["prims"])
    assert st.samples_per_pixel == 0 and st.ms > 0.0


@pytest.mark.parametrize("radius", ar.RADII)
@pytest.mark.parametrize("rays", [1, 4, 16, 64])
@pytest.mark.parametrize("case", ["main", "small"])
def test_layer_is_the_reference(gpu, oracle, case, rays, radius):
    """Both outputs together (a stats launch, then a plain one) and each alone."""
    _, _, w, h = ar.CASES[case]
    exp = ar.case_expected(oracle, case, rays, radius)
    with _renderer(oracle, case) as r:
        got = _run(r, w, h, rays, radius, stats=True)
        _assert_equal(got, exp)
        _assert_stats(got["stats"], exp, w, h)
        _assert_equal(_run(r, w, h, rays, radius), exp)
        for only in ("ao", "occluded"):
            sel = {k: k == only for k in ("ao", "occluded")}
            one = _run(r, w, h, rays, radius, **sel)
            assert only in one and len(one) == 2
            _assert_equal(one, exp, **sel)


def test_python_wrapper_and_every_ray_count(gpu, oracle):
    """render_ao returns the same arrays; 2, 8 and 32 rays a pixel are the
    reference too (the other four counts: test_layer_is_the_reference)."""
    _, _, w, h = ar.CASES["small"]
    with _renderer(oracle, "small") as r:
        for rays in (2, 8, 32):
            exp = ar.case_expected(oracle, "small", rays, 0.1)
            res = r.render_ao(rays, 0.1, stats=True)
            assert res["ao"].shape == (h, w) and res["ao"].dtype == np.float32
            assert np.array_equal(res["occluded"], exp["occluded"])
            assert np.array_equal(_bits(res["ao"]), _bits(exp["ao"]))
            _assert_stats(res["stats"], exp, w, h)
        assert "stats" not in r.render_ao(8, 0.1)


def test_same_bits_as_trace_rays_and_the_gbuffers_hit(gpu, oracle):
    """No oracle in the comparison: the reference's rays uploaded through
    trace_rays(kind="any") give the bits render_ao counts, and the rays start
    from render_gbuffer's hit."""
    _, _, w, h = ar.CASES["main"]
    for rays, radius in ((16, 0.1), (4, INF)):
        exp = ar.case_expected(oracle, "main", rays, radius)
        with _renderer(oracle, "main") as r:
            got = _run(r, w, h, rays, radius)
            g = r.render_gbuffer(albedo=False)
            assert np.array_equal(g["sphere"], exp["gbuffer"]["sphere"])
            assert np.array_equal(_bits(g["t"]), _bits(exp["gbuffer"]["t"]))
            assert np.array_equal(np.flatnonzero(g["sphere"].reshape(-1) != NO_HIT), exp["pixel"])
            recs = exp["rays"].reshape(-1, 8)
            t, sphere = r.trace_rays(recs, "any")
            count = np.zeros(w * h, np.uint32)
            count[exp["pixel"]] = (sphere != NO_HIT).reshape(-1, rays).sum(axis=1)
            assert np.array_equal(count.reshape(h, w), got["occluded"])
            assert np.array_equal((sphere != NO_HIT).reshape(-1, rays), exp["bits"])


@pytest.mark.parametrize("case,rays,radius", [("inside", 16, 0.1), ("inside", 4, INF), ("away", 16, 0.1),
                                              ("empty", 16, 0.1), ("one", 16, 0.1), ("one", 64, INF),
                                              ("thin", 16, 0.1)])
def test_edge_cases(gpu, oracle, case, rays, radius):
    """A camera inside a sphere (every pixel hits, the far root where sphere 0
    is nearest), a camera that sees nothing and an empty scene (1.0 / 0
    everywhere, nothing cast, nothing visited), one sphere (unoccluded wherever
    it is hit) and an image one pixel wide."""
    _, _, w, h = ar.CASES[case]
    exp = ar.case_expected(oracle, case, rays, radius)
    with _renderer(oracle, case) as r:
        got = _run(r, w, h, rays, radius, stats=True)
        _assert_equal(got, exp)
        _assert_stats(got["stats"], exp, w, h)
        _assert_equal(_run(r, w, h, rays, radius), exp)
    if case in ("away", "empty", "one"):
        assert not got["occluded"].any() and (got["ao"] == _bits(np.float32(1.0))[0]).all()
    if case in ("away", "empty"):
        assert got["stats"].shadow_rays == 0 and got["stats"].prims_tested == 0
    if case == "one":
        assert got["stats"].shadow_rays >= 8 * rays
    if case == "inside":
        assert got["stats"].shadow_rays == w * h * rays


def test_salts_differ_and_each_is_the_reference(gpu, oracle):
    _, _, w, h = ar.CASES["main"]
    with _renderer(oracle, "main") as r:
        layers = []
        for salt in (0, 1, 0xFFFFFFFF):
            exp = ar.case_expected(oracle, "main", 16, 0.1, salt)
            got = _run(r, w, h, 16, 0.1, salt, stats=True)
            _assert_equal(got, exp)
            _assert_stats(got["stats"], exp, w, h)
            layers.append(got["occluded"])
        assert (layers[0] != layers[1]).any() and (layers[0] != layers[2]).any()


def test_the_same_call_twice_is_identical(gpu, oracle):
    _, _, w, h = ar.CASES["main"]
    with _renderer(oracle, "main") as r:
        a = _run(r, w, h, 64, INF, 5)
        b = _run(r, w, h, 64, INF, 5)
        assert np.array_equal(a["ao"], b["ao"]) and np.array_equal(a["occluded"], b["occluded"])


@pytest.mark.parametrize("own_stream", [False, True])
def test_frames_are_undisturbed(gpu, oracle, own_stream):
    """A progressive renderer's frames 0 and 1, their running sums included, are
    byte-equal with and without AO calls (a stats one included) between them,
    on the handle's stream and on a caller's; the stats frame after them counts
    the same, and the call leaves the internal framebuffer alone."""
    import torch
    _, _, w, h = ar.CASES["main"]
    exp = ar.case_expected(oracle, "main", 16, 0.1)
    s = torch.cuda.Stream() if own_stream else None

    def frames(with_ao):
        out = []
        with _renderer(oracle, "main", spp=2, progressive=True, radiance=True) as r:
            for _ in range(2):
                r.render()
                out.append((r.readback(), r.readback_radiance()))
                if with_ao:
                    if s is not None:
                        with torch.cuda.stream(s):
                            _assert_equal(_run(r, w, h, 16, 0.1, stream=s.cuda_stream), exp)
                        s.synchronize()
                    else:
                        _assert_equal(_run(r, w, h, 16, 0.1), exp)
                    _assert_equal(_run(r, w, h, 16, 0.1, stats=True), exp)
                    assert np.array_equal(r.readback(), out[-1][0])
                    assert np.array_equal(_bits(r.readback_radiance()), _bits(out[-1][1]))
            st = r.render(stats=True)
            out.append((r.readback(), r.readback_radiance()))
        return out, (st.primary_rays, st.shadow_rays, st.nodes_visited, st.prims_tested, st.samples_per_pixel)

    plain, st_plain = frames(False)
    mixed, st_mixed = frames(True)
    for (a8, a32), (b8, b32) in zip(plain, mixed):
        assert np.array_equal(a8, b8) and np.array_equal(_bits(a32), _bits(b32))
    assert st_plain == st_mixed and st_plain[4] == 6
    assert not np.array_equal(plain[0][0], plain[1][0])  # the sums did accumulate


def test_layer_follows_resize_and_set_scene(gpu, oracle):
    """One handle: `small`, resized to `main`'s frame, then given the one-sphere
    scene at `one`'s size: each layer is its case's reference."""
    with _renderer(oracle, "small") as r:
        _assert_equal(_run(r, 9, 9, 16, 0.1), ar.case_expected(oracle, "small", 16, 0.1))
        _, _, w, h = ar.CASES["main"]
        r.resize(w, h)
        r.setIntrinsic(ar.intrinsic(oracle, "main"))
        got = _run(r, w, h, 16, 0.1, stats=True)
        _assert_equal(got, ar.case_expected(oracle, "main", 16, 0.1))
        _assert_stats(got["stats"], ar.case_expected(oracle, "main", 16, 0.1), w, h)
        sp, al = ar.spheres("one")
        r.set_scene(sp, al, **ar.TREE)
        r.resize(9, 9)
        r.setIntrinsic(ar.intrinsic(oracle, "one"))
        got = _run(r, 9, 9, 64, INF, stats=True)
        _assert_equal(got, ar.case_expected(oracle, "one", 64, INF))
        _assert_stats(got["stats"], ar.case_expected(oracle, "one", 64, INF), 9, 9)


def test_multi_device_handle_answers_from_device_0(gpu, oracle):
    _, _, w, h = ar.CASES["main"]
    exp = ar.case_expected(oracle, "main", 16, 0.1)
    with _renderer(oracle, "main", devices=[0, 0], transport="peer") as r:
        r.render()
        got = _run(r, w, h, 16, 0.1, stats=True)
        _assert_equal(got, exp)          # the whole frame, not devices[0]'s tiles
        _assert_stats(got["stats"], exp, w, h)


def test_refused_calls_launch_nothing(gpu, oracle):
    """Every refused call returns its code and leaves 0xAB-filled buffers as they were."""
    import torch
    lib = _lib.load()
    scene, pname, w, h = ar.CASES["small"]
    buf = torch.full((2, w * h, 4), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    a, o = buf[0].data_ptr(), buf[1].data_ptr()

    def code(r, rays=16, radius=0.1, flags=0, ao=a, occ=o, p=True, out=True):
        prm = _lib.RtAoParams(rays, radius, 0, flags)
        dst = _lib.RtAoOut(ao, occ)
        return lib.rt_render_ao(r._h, ctypes.byref(prm) if p else None, ctypes.byref(dst) if out else None,
                                None, None)

    with rt.KernelRenderer(w, h, mode="scene") as r:
        r.resize(w, h)
        r.setPosition(ar.pose(pname))
        assert code(r) == _lib.RT_E_NOSCENE
        with pytest.raises(_lib.RtError) as e:
            r.render_ao_device(16, 0.1, a, o)
        assert e.value.code == _lib.RT_E_NOSCENE
        sp, al = ar.spheres(scene)
        r.set_scene(sp, al, **ar.TREE)
        assert code(r, p=False) == _lib.RT_E_INVALID
        assert code(r, out=False) == _lib.RT_E_INVALID
        assert code(r, ao=None, occ=None) == _lib.RT_E_INVALID
        for rays in (0, 3, 5, 24, 65, 128, 0xFFFFFFFF):
            assert code(r, rays=rays) == _lib.RT_E_INVALID, rays
        for radius in (0.0, -0.0, -1.0, float("nan"), -INF):
            assert code(r, radius=radius) == _lib.RT_E_INVALID, radius
        for flags in (1, 2, 0x80000000):
            assert code(r, flags=flags) == _lib.RT_E_INVALID, flags
        assert b"rt_render_ao" in lib.rt_last_error(r._h)
        with pytest.raises(_lib.RtError) as e:
            r.render_ao_device(16, 0.1, None, None)
        assert e.value.code == _lib.RT_E_INVALID
        with pytest.raises(_lib.RtError):
            r.render_ao(3, 0.1)
        r.synchronize()
        torch.cuda.synchronize()
        assert (buf.cpu().numpy() == 0xAB).all()
        assert code(r) == _lib.RT_OK       # and the same arguments, valid, do write
        r.synchronize()
        assert not (buf.cpu().numpy() == 0xAB).all(axis=2).any()


def test_cli_ao_file_is_the_python_layer(gpu, tmp_path):
    """rt_cli --ao: a binary PGM of the frame's camera, 255 = open (the CLI's
    scene is generate_spheres(n, SEED) seen from scene_pose())."""
    import os
    import subprocess
    from raytracingstudy_amd.camera import scene_pose
    cli = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "raytracingstudy_amd", "rt_cli")
    w, h, rays, radius = 67, 45, 8, 0.25
    out = tmp_path / "ao.pgm"
    p = subprocess.run([cli, "--config", "c2", "--spheres", "1000", "--width", str(w), "--height", str(h),
                        "--frames", "1", "--ao", str(out), "--ao-rays", str(rays), "--ao-radius", str(radius),
                        "--test-poison"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    raw = out.read_bytes()
    head = f"P5\n{w} {h}\n255\n".encode()
    assert raw.startswith(head) and len(raw) == len(head) + w * h
    sp, al = rt.generate_spheres(1000, rt.SEED)
    with rt.KernelRenderer(w, h, mode="scene") as r:
        r.resize(w, h)
        r.setPosition(scene_pose())
        r.set_scene(sp, al, max_depth=7)
        res = r.render_ao(rays, radius, stats=True)
    grey = ((rays - res["occluded"].astype(np.int64)) * 255 // rays).astype(np.uint8)
    assert np.array_equal(np.frombuffer(raw[len(head):], np.uint8).reshape(h, w), grey)
    assert (f"ao: {int(res['occluded'].sum())} of {res['stats'].shadow_rays} rays occluded "
            f"({rays} rays a pixel, radius {radius:g})") in p.stdout
    assert 0 < res["occluded"].sum() < res["stats"].shadow_rays
