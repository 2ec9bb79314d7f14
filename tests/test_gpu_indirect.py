"""The one-bounce diffuse layer (rt_render_indirect) and the layer added into a
frame (rt_add_layer) against tests/indirect_ref.py, pixel by pixel.

The kernel walks pixel (x, y)'s centre ray like the G-buffer, builds rt_render_ao's
rays in registers, walks each to its nearest hit, shades that hit as a frame
does (a shadow walk along the handle's L for the lit ones) and sums the group's
colours in tree_sum's order, so every pixel's float4 (bit for bit), its count and
the four counters must equal the reference: oracle.Scene.trace per bounce and
shadow ray, the shading and the ordered sum restated in numpy float32.  Every
output buffer is pre-filled with 0xAB bytes and is one record longer than the
frame: an unwritten pixel and a write past the end both show.  The expectation
of a case is computed once and shared (indirect_ref.case_expected).
"""
import ctypes

import numpy as np
import pytest

import raytracingstudy_amd as rt
from raytracingstudy_amd import _lib

import ao_ref as ar
import filter_ref as fr
import gbuffer_ref
import indirect_ref as ir
import reproject_ref as rr

pytestmark = pytest.mark.gpu

NO_HIT = ir.NO_HIT
INF = float("inf")
OTHER_LIGHT, OTHER_AMBIENT = (-0.3, 0.8, 0.5), 0.35


def _renderer(oracle, case, **kw):
    scene, pname, w, h = ar.CASES[case]
    sp, al = ar.spheres(scene)
    r = rt.KernelRenderer(w, h, mode="scene", **kw)
    r.resize(w, h)
    r.setIntrinsic(ar.intrinsic(oracle, case))
    r.setPosition(ar.pose(pname))
    r.set_scene(sp, al, **ar.TREE)
    return r


def _run(r, w, h, rays, radius, salt=0, sky_scale=1.0, layer=True, occluded=True, stream=None, stats=False):
    """rt_render_indirect into 0xAB-filled buffers of w*h + 1 records; the guard
    record of each must come back untouched."""
    import torch
    n = w * h
    bufs = {k: torch.full((n + 1, size), 0xAB, dtype=torch.uint8, device="cuda")
            for k, on, size in (("layer", layer, 16), ("occluded", occluded, 4)) if on}
    if stream is None:
        torch.cuda.synchronize()
    ptr = {k: bufs[k].data_ptr() if k in bufs else None for k in ("layer", "occluded")}
    st = r.render_indirect_device(rays, radius, ptr["layer"], ptr["occluded"], salt, sky_scale, stream=stream,
                                  stats=stats)
    if stream is None:
        r.synchronize()
    out = {"stats": st}
    for k, b in bufs.items():
        raw = b.cpu().numpy()  # on a caller's stream: ordered after the launch
        assert (raw[n] == 0xAB).all(), k
        words = raw[:n].copy().view(np.uint32)
        out[k] = words.reshape(h, w, 4) if k == "layer" else words.reshape(h, w)   # layer: its bits
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_equal(got, exp, layer=True, occluded=True):
    if occluded:
        assert np.array_equal(got["occluded"], exp["occluded"])
    if layer:
        assert np.array_equal(got["layer"], _bits(exp["layer"]))   # bit for bit: a sentinel word never is one


def _assert_stats(st, exp, w, h):
    assert st.primary_rays == w * h and st.shadow_rays == exp["cast"]
    assert (st.nodes_visited, st.prims_tested) == (exp["nodes"], exp["prims"])
    assert st.samples_per_pixel == 0 and st.ms > 0.0


# ---- the main grid -------------------------------------------------------------------
@pytest.mark.parametrize("radius", ar.RADII)
@pytest.mark.parametrize("rays", [1, 4, 16, 64])
@pytest.mark.parametrize("case", ["main", "small"])
def test_layer_is_the_reference(gpu, oracle, case, rays, radius):
    """Both outputs together (a stats launch, then a plain one) and each alone."""
    _, _, w, h = ar.CASES[case]
    exp = ir.case_expected(oracle, case, rays, radius)
    with _renderer(oracle, case) as r:
        got = _run(r, w, h, rays, radius, stats=True)
        _assert_equal(got, exp)
        _assert_stats(got["stats"], exp, w, h)
        _assert_equal(_run(r, w, h, rays, radius), exp)
        for only in ("layer", "occluded"):
            sel = {k: k == only for k in ("layer", "occluded")}
            one = _run(r, w, h, rays, radius, **sel)
            assert only in one and len(one) == 2
            _assert_equal(one, exp, **sel)


def test_python_wrapper_and_every_ray_count(gpu, oracle):
    """render_indirect returns the same arrays; 2, 8 and 32 rays a pixel are the
    reference too (the other four counts: test_layer_is_the_reference)."""
    _, _, w, h = ar.CASES["small"]
    with _renderer(oracle, "small") as r:
        for rays in (2, 8, 32):
            exp = ir.case_expected(oracle, "small", rays, 0.1)
            res = r.render_indirect(rays, 0.1, stats=True)
            assert res["layer"].shape == (h, w, 4) and res["layer"].dtype == np.float32
            assert np.array_equal(res["occluded"], exp["occluded"])
            assert np.array_equal(_bits(res["layer"]), _bits(exp["layer"]))
            _assert_stats(res["stats"], exp, w, h)
        assert "stats" not in r.render_indirect(8, 0.1)


# ---- cross-checks --------------------------------------------------------------------
@pytest.mark.parametrize("rays,radius", [(16, 0.1), (4, INF), (64, 0.1)])
def test_w_and_the_counts_are_render_aos(gpu, oracle, rays, radius):
    _, _, w, h = ar.CASES["main"]
    with _renderer(oracle, "main") as r:
        got = _run(r, w, h, rays, radius, salt=3)
        ao = r.render_ao(rays, radius, salt=3)
        assert np.array_equal(got["layer"][..., 3], _bits(ao["ao"]))
        assert np.array_equal(got["occluded"], ao["occluded"])
        assert 0 < got["occluded"].sum() < rays * w * h


def test_same_bits_from_trace_rays_and_numpy(gpu, oracle):
    """No oracle in the comparison: the reference's bounce rays uploaded through
    trace_rays("nearest"), the lit hits' shadow rays through trace_rays("any"), the
    shading and the ordered sum in numpy."""
    _, _, w, h = ar.CASES["main"]
    sp, al = ar.spheres("cloud")
    L = ir.light_toward(ir.LIGHT)
    for rays, radius in ((16, 0.1), (4, INF)):
        exp = ir.case_expected(oracle, "main", rays, radius)
        with _renderer(oracle, "main") as r:
            got = _run(r, w, h, rays, radius)
            recs = exp["rays"].reshape(-1, 8)
            t, s = r.trace_rays(recs, "nearest")
            t = np.asarray(t, np.float32)
            hit = s != NO_HIT
            assert np.array_equal(s, exp["hit_sphere"].reshape(-1))
            o, d = recs[:, :3], recs[:, 4:7]
            rec = sp[s[hit]]
            q = o[hit] + t[hit][:, None] * d[hit]
            m = (q - rec[:, :3]) * (np.float32(1.0) / rec[:, 3])[:, None]
            ndl = (m[:, 0] * L[0] + m[:, 1] * L[1]) + m[:, 2] * L[2]
            lam = np.where(ndl > 0, ndl, np.float32(0.0)).astype(np.float32)
            want = ndl > 0
            srec = np.zeros((int(want.sum()), 8), np.float32)
            srec[:, :3] = q[want] + m[want] * ir.SHADOW_EPS
            srec[:, 4:7] = L
            srec[:, 7] = np.inf
            assert np.array_equal(_bits(srec), _bits(exp["shadow_rays"]))
            _, ss = r.trace_rays(srec, "any")
            lam[np.flatnonzero(want)[ss != NO_HIT]] = 0.0
            col = ir.sky_color(d, 1.0)
            col[hit] = ir.hit_color(al[s[hit]], ir.AMBIENT, lam)
            rgb = ir.mean_of(ir.tree_sum(col.reshape(-1, rays, 3))[:, 0, :], rays)
            layer = np.zeros((w * h, 4), np.float32)
            layer[:, 3] = 1.0
            layer[exp["pixel"], :3] = rgb
            layer[exp["pixel"], 3] = ir.open_share(rays, hit.reshape(-1, rays).sum(axis=1))
            assert np.array_equal(got["layer"], _bits(layer).reshape(h, w, 4))
            assert (ss != NO_HIT).any() and (ss == NO_HIT).any()


# ---- edge cases ------------------------------------------------------------------------
@pytest.mark.parametrize("case,rays,radius", [("inside", 16, 0.1), ("inside", 4, INF), ("away", 16, 0.1),
                                              ("empty", 16, 0.1), ("one", 16, 0.1), ("one", 64, INF),
                                              ("thin", 16, 0.1)])
def test_edge_cases(gpu, oracle, case, rays, radius):
    """A camera inside a sphere (every pixel hits the far root, and its bounce rays
    start inside the sphere), a camera that sees nothing and an empty scene
    ({0, 0, 0, 1} / 0 everywhere, nothing cast, nothing visited), one sphere (every
    bounce ray escapes: the sky's colour) and an image one pixel wide."""
    _, _, w, h = ar.CASES[case]
    exp = ir.case_expected(oracle, case, rays, radius)
    with _renderer(oracle, case) as r:
        got = _run(r, w, h, rays, radius, stats=True)
        _assert_equal(got, exp)
        _assert_stats(got["stats"], exp, w, h)
        _assert_equal(_run(r, w, h, rays, radius), exp)
    if case in ("away", "empty"):
        assert np.array_equal(got["layer"], _bits(np.broadcast_to(np.float32([0, 0, 0, 1]), (h, w, 4))))
        assert got["stats"].shadow_rays == 0 and got["stats"].prims_tested == 0
    if case in ("away", "empty", "one"):
        assert not got["occluded"].any()
    if case == "one":
        assert got["stats"].shadow_rays >= 8 * rays and got["stats"].shadow_rays % rays == 0
    if case == "inside":
        assert got["stats"].shadow_rays >= w * h * rays


# ---- parameters and handle settings --------------------------------------------------
@pytest.mark.parametrize("sky_scale", [0.0, 0.5, 1.0])
def test_sky_scale(gpu, oracle, sky_scale):
    _, _, w, h = ar.CASES["main"]
    exp = ir.case_expected(oracle, "main", 4, 0.1, sky_scale=sky_scale)
    with _renderer(oracle, "main") as r:
        got = _run(r, w, h, 4, 0.1, sky_scale=sky_scale, stats=True)
        _assert_equal(got, exp)
        _assert_stats(got["stats"], exp, w, h)
    one = ir.case_expected(oracle, "main", 4, 0.1, sky_scale=1.0)
    assert np.array_equal(exp["occluded"], one["occluded"])
    assert (sky_scale == 1.0) != bool((_bits(exp["layer"]) != _bits(one["layer"])).any())


def test_salts_differ_and_each_is_the_reference(gpu, oracle):
    _, _, w, h = ar.CASES["main"]
    with _renderer(oracle, "main") as r:
        layers = []
        for salt in (0, 1, 0xFFFFFFFF):
            exp = ir.case_expected(oracle, "main", 4, 0.1, salt)
            got = _run(r, w, h, 4, 0.1, salt, stats=True)
            _assert_equal(got, exp)
            _assert_stats(got["stats"], exp, w, h)
            layers.append(got["layer"])
        assert (layers[0] != layers[1]).any() and (layers[0] != layers[2]).any()


@pytest.mark.parametrize("kw", [dict(shadows=False), dict(light=OTHER_LIGHT, ambient=OTHER_AMBIENT),
                                dict(light=OTHER_LIGHT, ambient=0.0, shadows=False), dict(seed=0x1234567)])
def test_handle_settings(gpu, oracle, kw):
    """RT_FLAG_NO_SHADOWS, another light_dir and ambient, ambient 0, another seed."""
    _, _, w, h = ar.CASES["main"]
    exp = ir.case_expected(oracle, "main", 4, INF, **kw)
    base = ir.case_expected(oracle, "main", 4, INF)
    assert (_bits(exp["layer"]) != _bits(base["layer"])).any()
    ctor = {("light_dir" if k == "light" else k): v for k, v in kw.items()}
    with _renderer(oracle, "main", **ctor) as r:
        got = _run(r, w, h, 4, INF, stats=True)
        _assert_equal(got, exp)
        _assert_stats(got["stats"], exp, w, h)
        _assert_equal(_run(r, w, h, 4, INF), exp)
    if kw.get("shadows") is False:
        assert exp["cast"] == 4 * len(exp["pixel"]) and base["cast"] > exp["cast"]


# ---- calling conditions ----------------------------------------------------------------
@pytest.mark.parametrize("own_stream", [False, True])
def test_frames_are_undisturbed(gpu, oracle, own_stream):
    """A progressive renderer's frames 0 and 1, their running sums included, are
    byte-equal with and without indirect calls (a stats one included) between
    them, on the handle's stream and on a caller's; the stats frame after them
    counts the same, and the call leaves the internal framebuffer alone."""
    import torch
    _, _, w, h = ar.CASES["main"]
    exp = ir.case_expected(oracle, "main", 4, 0.1)
    s = torch.cuda.Stream() if own_stream else None

    def frames(with_calls):
        out = []
        with _renderer(oracle, "main", spp=2, progressive=True, radiance=True) as r:
            for _ in range(2):
                r.render()
                out.append((r.readback(), r.readback_radiance()))
                if with_calls:
                    if s is not None:
                        with torch.cuda.stream(s):
                            _assert_equal(_run(r, w, h, 4, 0.1, stream=s.cuda_stream), exp)
                        s.synchronize()
                    else:
                        _assert_equal(_run(r, w, h, 4, 0.1), exp)
                    _assert_equal(_run(r, w, h, 4, 0.1, stats=True), exp)
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


def test_multi_device_handle_answers_from_device_0(gpu, oracle):
    _, _, w, h = ar.CASES["main"]
    exp = ir.case_expected(oracle, "main", 4, 0.1)
    with _renderer(oracle, "main", devices=[0, 0], transport="peer") as r:
        r.render()
        got = _run(r, w, h, 4, 0.1, stats=True)
        _assert_equal(got, exp)          # the whole frame, not devices[0]'s tiles
        _assert_stats(got["stats"], exp, w, h)


def test_refused_calls_launch_nothing(gpu, oracle):
    """Every refused call returns its code and leaves 0xAB-filled buffers as they were."""
    import torch
    lib = _lib.load()
    scene, pname, w, h = ar.CASES["small"]
    buf = torch.full((w * h, 24), 0xAB, dtype=torch.uint8, device="cuda")   # a layer, counts and RGBA8 pixels
    torch.cuda.synchronize()
    a = buf.data_ptr()
    o, px = a + 16 * w * h, a + 20 * w * h

    def code(r, rays=4, radius=0.1, sky=1.0, flags=0, layer=a, occ=o, p=True, out=True):
        prm = _lib.RtIndirectParams(rays, radius, 0, sky, flags)
        dst = _lib.RtIndirectOut(layer, occ)
        return lib.rt_render_indirect(r._h, ctypes.byref(prm) if p else None, ctypes.byref(dst) if out else None,
                                      None, None)

    with rt.KernelRenderer(w, h, mode="scene") as r:
        r.resize(w, h)
        r.setPosition(ar.pose(pname))
        assert code(r) == _lib.RT_E_NOSCENE
        with pytest.raises(_lib.RtError) as e:
            r.render_indirect_device(4, 0.1, a, o)
        assert e.value.code == _lib.RT_E_NOSCENE
        sp, al = ar.spheres(scene)
        r.set_scene(sp, al, **ar.TREE)
        assert code(r, p=False) == _lib.RT_E_INVALID
        assert code(r, out=False) == _lib.RT_E_INVALID
        assert code(r, layer=None, occ=None) == _lib.RT_E_INVALID
        for rays in (0, 3, 5, 24, 65, 128, 0xFFFFFFFF):
            assert code(r, rays=rays) == _lib.RT_E_INVALID, rays
        for radius in (0.0, -0.0, -1.0, float("nan"), -INF):
            assert code(r, radius=radius) == _lib.RT_E_INVALID, radius
        for sky in (-1.0, -1e-30, float("nan"), INF, -INF):
            assert code(r, sky=sky) == _lib.RT_E_INVALID, sky
        for flags in (1, 2, 0x80000000):
            assert code(r, flags=flags) == _lib.RT_E_INVALID, flags
        assert b"rt_render_indirect" in lib.rt_last_error(r._h)
        for gain in (-1.0, -1e-30, float("nan"), INF, -INF):
            assert lib.rt_add_layer(r._h, px, a, None, gain, None) == _lib.RT_E_INVALID, gain
        assert lib.rt_add_layer(r._h, px, None, None, 1.0, None) == _lib.RT_E_INVALID
        assert b"rt_add_layer" in lib.rt_last_error(r._h)
        with pytest.raises(_lib.RtError) as e:
            r.render_indirect_device(4, 0.1, None, None)
        assert e.value.code == _lib.RT_E_INVALID
        with pytest.raises(_lib.RtError):
            r.render_indirect(3, 0.1)
        with pytest.raises(_lib.RtError):
            r.add_layer_device(a, -1.0, None, px)
        r.synchronize()
        torch.cuda.synchronize()
        assert (buf.cpu().numpy() == 0xAB).all()
        assert code(r) == _lib.RT_OK       # and the same arguments, valid, do write
        assert lib.rt_add_layer(r._h, px, a, None, 1.0, None) == _lib.RT_OK
        r.synchronize()
        raw = buf.cpu().numpy().reshape(-1)
        assert not (raw[:20 * w * h].reshape(-1, 4) == 0xAB).all(axis=1).any()
        assert (raw[20 * w * h:].reshape(-1, 4)[:, 3] == 0xAB).all()      # alpha kept


# ---- rt_add_layer --------------------------------------------------------------------
def _odd_layer(w, h, seed):
    """A float4 layer around the unit range with NaN, +-inf and negative values."""
    g = np.random.default_rng(seed)
    v = (g.random((h, w, 4)) * 1.5 - 0.25).astype(np.float32)
    n = max(1, (w * h) // 20)
    for val in (np.nan, np.inf, -np.inf, -3.0, 1e30):
        v.reshape(-1)[g.integers(0, v.size, n)] = val
    return v


@pytest.mark.parametrize("case", ["main", "small", "thin"])
def test_add_layer_is_the_reference(gpu, oracle, case):
    """Byte for byte against numpy with and without the G-buffer's albedo, on the
    internal framebuffer and on a caller's buffer (one pixel longer, its guard
    untouched), on layers holding NaN, infinite and negative values; alpha is kept."""
    import torch
    _, _, w, h = ar.CASES[case]
    n = w * h
    with _renderer(oracle, case) as r:
        d_alb = torch.empty((h, w), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        r.render_gbuffer_device(None, None, d_alb.data_ptr())
        r.synchronize()
        albedo = d_alb.cpu().numpy().view(np.uint32)
        assert np.array_equal(albedo, ar.case_expected(oracle, case, 1, 0.1)["gbuffer"]["albedo"])
        changed = 0
        for k, (gain, with_albedo) in enumerate([(1.0, True), (1.0, False), (0.5, True), (0.0, False), (2.5, True)]):
            layer = _odd_layer(w, h, 40 + k)
            d_layer = torch.from_numpy(layer).cuda()
            torch.cuda.synchronize()
            alb_ptr, alb = (d_alb.data_ptr(), albedo) if with_albedo else (None, None)
            # the internal framebuffer
            r.render()
            frame = r.readback()
            r.add_layer_device(d_layer.data_ptr(), gain, alb_ptr)
            got = r.readback()
            want = ir.add_layer(frame, layer, alb, gain)
            assert np.array_equal(got, want), (gain, with_albedo)
            assert np.array_equal(got[..., 3], frame[..., 3])
            if gain == 0.0:     # nothing is added where the layer is finite (0 * inf is a NaN: it stores 0)
                finite = np.isfinite(layer[..., :3]).all(axis=2)
                assert np.array_equal(got[finite], frame[finite]) and finite.sum() > (w * h) // 2
            changed += int((got != frame).any(axis=2).sum())
            # a caller's buffer, with alpha bytes of its own
            px = np.random.default_rng(90 + k).integers(0, 256, (h, w, 4)).astype(np.uint8)
            mine = torch.full((n + 1, 4), 0xAB, dtype=torch.uint8, device="cuda")
            mine[:n] = torch.from_numpy(px.reshape(n, 4)).cuda()
            torch.cuda.synchronize()
            r.add_layer_device(d_layer.data_ptr(), gain, alb_ptr, mine.data_ptr())
            r.synchronize()
            raw = mine.cpu().numpy()
            assert (raw[n] == 0xAB).all()
            assert np.array_equal(raw[:n].reshape(h, w, 4), ir.add_layer(px, layer, alb, gain)), (gain, with_albedo)
            assert np.array_equal(_bits(d_layer.cpu().numpy()), _bits(layer))     # the layer is only read
        assert changed > 0


def test_cli_indirect_file_is_the_python_calls(gpu, tmp_path):
    """rt_cli --indirect: a PPM of the last frame with the camera's one-bounce layer
    added under the G-buffer's albedo (the CLI's scene is generate_spheres(n, SEED)
    seen from scene_pose())."""
    import os
    import subprocess
    import torch
    from raytracingstudy_amd.camera import scene_pose
    cli = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "raytracingstudy_amd", "rt_cli")
    w, h, rays, radius = 67, 45, 4, 0.25
    out = tmp_path / "indirect.ppm"
    p = subprocess.run([cli, "--config", "c2", "--spheres", "1000", "--width", str(w), "--height", str(h),
                        "--frames", "1", "--indirect", str(out), "--indirect-rays", str(rays), "--indirect-radius",
                        str(radius), "--test-poison"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    raw = out.read_bytes()
    head = f"P6\n{w} {h}\n255\n".encode()
    assert raw.startswith(head) and len(raw) == len(head) + w * h * 3
    sp, al = rt.generate_spheres(1000, rt.SEED)
    with rt.KernelRenderer(w, h, mode="scene") as r:
        r.resize(w, h)
        r.setPosition(scene_pose())
        r.set_scene(sp, al, max_depth=7)
        d_alb = torch.empty((h, w), dtype=torch.int32, device="cuda")
        d_layer = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
        d_occ = torch.empty((h, w), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        r.render()
        frame = r.readback()
        r.render_gbuffer_device(None, None, d_alb.data_ptr())
        st = r.render_indirect_device(rays, radius, d_layer.data_ptr(), d_occ.data_ptr(), stats=True)
        r.add_layer_device(d_layer.data_ptr(), 1.0, d_alb.data_ptr())
        img = r.readback()
        hits = int(d_occ.cpu().numpy().sum())
    assert np.array_equal(np.frombuffer(raw[len(head):], np.uint8).reshape(h, w, 3), img[..., :3])
    assert not np.array_equal(img, frame)
    assert (f"indirect: {hits} bounce rays hit, {st.shadow_rays} bounce and shadow rays cast "
            f"({rays} rays a pixel, radius {radius:g})") in p.stdout
    assert 0 < hits < st.shadow_rays


# ---- the viewer's chain ----------------------------------------------------------------
def test_three_moving_frames_are_the_composed_references(gpu, oracle):
    """indirect -> reproject_layer(channels=4) -> filter_layer(channels=4) ->
    add_layer on the device, the device's own buffers carried from frame to frame,
    against indirect_ref, reproject_ref and filter_ref composed on the oracle's
    G-buffer: every stage bit for bit, the final frame byte for byte."""
    import torch
    scene, pname, w, h = ar.CASES["main"]
    sp, al = ar.spheres(scene)
    sc = ar.oracle_scene(oracle, scene)
    K = ar.intrinsic(oracle, "main")
    n = w * h
    hist = ref_hist = None
    took_total = 0
    with _renderer(oracle, "main") as r:
        for k, shift in enumerate([(0.0, 0.0, 0.0), (0.004, -0.003, 0.01), (0.008, -0.003, 0.02)]):
            P = ar.pose(pname).copy()
            P[3, :3] += np.asarray(shift, np.float32)
            r.setPosition(P)
            d = dict(hits=torch.empty((h, w, 2), dtype=torch.int32, device="cuda"),
                     nrm=torch.empty((h, w, 4), dtype=torch.float32, device="cuda"),
                     alb=torch.empty((h, w), dtype=torch.int32, device="cuda"),
                     layer=torch.empty((h, w, 4), dtype=torch.float32, device="cuda"),
                     out=torch.empty((h, w, 4), dtype=torch.float32, device="cuda"),
                     count=torch.empty((h, w), dtype=torch.float32, device="cuda"),
                     flt=torch.full((n + 1, 16), 0xAB, dtype=torch.uint8, device="cuda"))
            torch.cuda.synchronize()
            r.render_gbuffer_device(d["hits"].data_ptr(), d["nrm"].data_ptr(), d["alb"].data_ptr())
            r.render_indirect_device(4, 0.1, d["layer"].data_ptr(), None, salt=k)
            r.reproject_layer_device(d["hits"].data_ptr(), d["layer"].data_ptr(), d["out"].data_ptr(),
                                     d["count"].data_ptr(), hist, 4)
            r.filter_layer_device(d["out"].data_ptr(), d["flt"].data_ptr(), d["hits"].data_ptr(), d["nrm"].data_ptr(),
                                  3, 4)
            r.render()
            frame = r.readback()
            r.add_layer_device(d["flt"].data_ptr(), 1.5, d["alb"].data_ptr())
            got = r.readback()
            # the same on the host
            g = gbuffer_ref.expected(oracle, sc, sp, al, P, K, w, h)
            e = ir.expected(oracle, sc, sp, al, P, K, w, h, 4, 0.1, salt=k, g=g)
            o = np.asarray(P, np.float32).reshape(4, 4)[3, :3]
            w_out, w_count, took = rr.reproject(e["layer"], g["sphere"], g["t"], g["dirs"], o, ref_hist)
            flt = fr.filter_layer(w_out, g["sphere"], g["t"], g["normal"])
            assert np.array_equal(_bits(d["layer"].cpu().numpy()), _bits(e["layer"])), k
            assert np.array_equal(_bits(d["out"].cpu().numpy()), _bits(w_out)), k
            assert np.array_equal(_bits(d["count"].cpu().numpy()), _bits(w_count)), k
            raw = d["flt"].cpu().numpy()
            assert (raw[n] == 0xAB).all()
            assert np.array_equal(raw[:n].copy().view(np.uint32).reshape(h, w, 4), _bits(flt)), k
            assert np.array_equal(got, ir.add_layer(frame, flt, g["albedo"], 1.5)), k
            assert not np.array_equal(got, frame)
            took_total += int(took.sum()) if k else 0
            hist = dict(hits=d["hits"].data_ptr(), layer=d["out"].data_ptr(), count=d["count"].data_ptr(),
                        pose=P.reshape(16), K=K, keep=d)      # keep: the tensors stay alive for the next frame
            ref_hist = dict(sphere=g["sphere"], t=g["t"], layer=w_out, count=w_count, pose=P, K=K)
    assert took_total > n // 4      # the moved frames did take history
