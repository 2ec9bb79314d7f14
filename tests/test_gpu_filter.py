"""The guide-driven layer filter and the layer multiply (rt_filter_layer,
rt_apply_layer) against tests/filter_ref.py, bit for bit.

The guides are the handle's own G-buffer (rt_render_gbuffer is held to the
oracle in test_gpu_gbuffer.py): the reference filters the same layer under the
same guides in numpy float32, and every output word must equal it.  Every
output buffer is pre-filled with 0xAB bytes and is one pixel longer than the
frame: an unwritten element and a write past the end both show; the input is
compared with its upload after every call.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import raytracingstudy_amd as rt
from raytracingstudy_amd import _lib

import ao_ref as ar
import filter_ref as fr
import query_scaffold as qs

pytestmark = pytest.mark.gpu

NO_HIT = fr.NO_HIT
INF = float("inf")
SIZES = [(1, 1), (5, 3), (37, 29), (70, 9), (129, 65)]
# (passes, normal_power, depth_sigma): every value of each the filter is specified at
SETTINGS = [(p, n, s) for p in (1, 2, 3, 5) for n, s in ((5, 0.05), (0, INF), (0, 0.05), (5, INF))]
SENTINEL = 0xABABABAB


def _scene(name):
    """cloud: 300 generated spheres, their radii doubled (a third to a half of the
    frame hits, spheres span a few to a few dozen pixels); ao: the AO tests' cloud,
    which their `inside` and `away` cameras are made for."""
    if name == "ao":
        sp, al = ar.spheres("cloud")
        return sp, al, ar.TREE
    sp, al = rt.generate_spheres(300, rt.SEED)
    sp = sp.copy()
    sp[:, 3] *= np.float32(2.0)
    return sp, al, ar.TREE


def _renderer(w, h, scene="cloud", pose=None, **kw):
    r = qs.scene_renderer(scene, w, h, scene=_scene, **kw)
    if pose is not None:
        r.setPosition(ar.pose(pose))
    return r


class Guides:
    """The handle's G-buffer on the device and on the host."""

    def __init__(self, r):
        import torch
        w, h = r.width, r.height
        self.w, self.h = w, h
        self.d_hits = torch.empty((h, w, 2), dtype=torch.int32, device="cuda")
        self.d_nrm = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        r.render_gbuffer_device(self.d_hits.data_ptr(), self.d_nrm.data_ptr())
        r.synchronize()
        hits = self.d_hits.cpu().numpy()
        self.t = np.ascontiguousarray(hits[..., 0]).view(np.float32)
        self.sphere = np.ascontiguousarray(hits[..., 1]).view(np.uint32)
        self.normal = self.d_nrm.cpu().numpy()
        self.hit = self.sphere != NO_HIT

    def ref(self, layer, passes, npow, sigma):
        return fr.filter_layer(layer, self.sphere, self.t, self.normal, passes, sigma, npow)


def _ao_layer(r, rays=4, radius=0.1):
    """The handle's AO layer: (device tensor (h, w) float32, host copy)."""
    import torch
    d = torch.empty((r.height, r.width), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    r.render_ao_device(rays, radius, d.data_ptr())
    r.synchronize()
    return d, d.cpu().numpy()


def _random_layer(w, h, seed):
    """A seeded float4 layer with a few NaN and infinite values in it."""
    import torch
    g = np.random.default_rng(seed)
    v = (g.random((h, w, 4)) * 4.0 - 1.0).astype(np.float32)
    n = max(1, (w * h) // 40)
    for val in (np.nan, np.inf, -np.inf):
        v.reshape(-1)[g.integers(0, v.size, n)] = val
    d = torch.from_numpy(v).cuda()
    torch.cuda.synchronize()
    return d, v


def _run(r, g, d_in, host_in, passes=3, npow=5, sigma=0.05, stream=None, stats=False):
    """rt_filter_layer into a 0xAB-filled buffer one pixel longer than the layer ->
    the output's words in the layer's shape (and the stats)."""
    import torch
    channels = 1 if host_in.ndim == 2 else 4
    n = g.w * g.h
    out = torch.full(((n + 1) * channels,), SENTINEL - (1 << 32), dtype=torch.int32, device="cuda")
    if stream is None:
        torch.cuda.synchronize()
    st = r.filter_layer_device(d_in.data_ptr(), out.data_ptr(), g.d_hits.data_ptr(), g.d_nrm.data_ptr(), passes,
                               channels, sigma, npow, stream=stream, stats=stats)
    if stream is None:
        r.synchronize()
    raw = out.cpu().numpy().view(np.uint32)        # on a caller's stream: ordered after the launch
    assert (raw[n * channels:] == SENTINEL).all()
    assert np.array_equal(qs.bits(d_in.cpu().numpy()), qs.bits(host_in))       # dev_in is never written
    words = raw[:n * channels].reshape(host_in.shape)
    return (words, st) if stats else words


def _same(words, want):
    """Bit for bit; a NaN is a NaN whatever its payload (the layer's own NaNs and
    inf - inf of its infinities: the sign of a generated NaN is the platform's).
    The sentinel word is no NaN, so an unwritten element cannot pass as one."""
    got = words.view(np.float32)
    return bool(((words == qs.bits(want)) | (np.isnan(want) & np.isnan(got))).all())


@pytest.mark.parametrize("channels", [1, 4])
@pytest.mark.parametrize("w,h", SIZES)
def test_filter_is_the_reference(gpu, w, h, channels):
    """The AO layer of the frame (channels 1) or a random float4 layer with NaN and
    infinite values (channels 4), at every setting."""
    with _renderer(w, h) as r:
        g = Guides(r)
        d_in, v = _ao_layer(r) if channels == 1 else _random_layer(w, h, 100 * w + h)
        if (w, h) == (129, 65):     # the frame is what its name says: hits, misses, a graded layer
            assert 0.3 < g.hit.mean() < 0.95
            assert channels == 4 or len(np.unique(v[g.hit])) >= 4
        moved = 0
        for passes, npow, sigma in SETTINGS:
            words = _run(r, g, d_in, v, passes, npow, sigma)
            assert _same(words, g.ref(v, passes, npow, sigma)), (passes, npow, sigma)
            moved += int((words != qs.bits(v)).sum())
        assert moved > 0 or w * h <= 15 or not g.hit.any()


@pytest.mark.parametrize("pose,all_hit", [("inside", True), ("away", False)])
def test_all_hit_and_all_miss_frames(gpu, pose, all_hit):
    with _renderer(37, 29, "ao", pose) as r:
        g = Guides(r)
        assert g.hit.all() if all_hit else not g.hit.any()
        for d_in, v in (_ao_layer(r, 4, INF), _random_layer(37, 29, 9)):
            for passes, npow, sigma in ((3, 5, 0.05), (5, 0, INF)):
                words = _run(r, g, d_in, v, passes, npow, sigma)
                assert _same(words, g.ref(v, passes, npow, sigma))
                if not all_hit:     # every pixel copies its value, NaNs included
                    assert np.array_equal(words, qs.bits(v))


def test_garbage_guides_copy_the_value(gpu):
    """NaN depths under valid sphere indices: sw is a NaN, and sw > 0 is false."""
    import torch
    with _renderer(37, 29) as r:
        g = Guides(r)
        d_in, v = _ao_layer(r)
        bad = g.d_hits.clone()
        bad[..., 0] = torch.where(bad[..., 1] != -1, torch.full_like(bad[..., 0], 0x7FC00000), bad[..., 0])
        g.d_hits = bad
        assert np.array_equal(_run(r, g, d_in, v, 2), qs.bits(v))


def test_same_call_twice_a_callers_stream_and_stats(gpu):
    import torch
    with _renderer(70, 9) as r:
        g = Guides(r)
        d_in, v = _ao_layer(r)
        want = g.ref(v, 3, 5, 0.05)
        a = _run(r, g, d_in, v)
        b = _run(r, g, d_in, v)
        assert np.array_equal(a, b) and _same(a, want)
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            c = _run(r, g, d_in, v, stream=s.cuda_stream)
        s.synchronize()
        assert np.array_equal(a, c)
        d, st = _run(r, g, d_in, v, stats=True)
        assert np.array_equal(a, d)
        assert st.ms > 0.0 and (st.primary_rays, st.shadow_rays, st.nodes_visited, st.prims_tested,
                                st.samples_per_pixel) == (0, 0, 0, 0, 0)


def test_frames_are_undisturbed(gpu):
    """Progressive frames with the whole chain between them (G-buffer, AO, filter on
    one and four channels, the multiply into the internal framebuffer) are
    byte-equal to the frames without it: the next frame overwrites the multiply."""
    w, h = 37, 29

    def between(r):
        g = Guides(r)
        d_in, v = _ao_layer(r)
        words = _run(r, g, d_in, v, stats=True)[0]
        assert _same(words, g.ref(v, 3, 5, 0.05))
        d4, v4 = _random_layer(w, h, 3)
        assert _same(_run(r, g, d4, v4, 2), g.ref(v4, 2, 5, 0.05))
        before = r.readback()
        r.apply_layer_device(d_in.data_ptr(), 0.25)
        after = r.readback()
        assert np.array_equal(after, fr.apply_layer(before, v, 0.25)) and not np.array_equal(after, before)

    qs.assert_frames_undisturbed(lambda **kw: _renderer(w, h, **kw), between)


def test_scratch_follows_a_resize_up_and_down(gpu):
    with _renderer(37, 29) as r:
        for w, h in ((37, 29), (129, 65), (5, 3), (70, 9)):
            r.resize(w, h)
            g = Guides(r)
            d_in, v = _ao_layer(r)
            assert _same(_run(r, g, d_in, v, 3), g.ref(v, 3, 5, 0.05)), (w, h)
            d4, v4 = _random_layer(w, h, w)
            assert _same(_run(r, g, d4, v4, 2, 0, INF), g.ref(v4, 2, 0, INF)), (w, h)


def test_refused_calls_launch_nothing(gpu):
    """Every refused call returns RT_E_INVALID and leaves the 0xAB-filled output as it was."""
    import torch
    lib = _lib.load()
    w, h = 37, 29
    with _renderer(w, h) as r:
        g = Guides(r)
        d_in, v = _ao_layer(r)
        out = torch.full((w * h * 4,), SENTINEL - (1 << 32), dtype=torch.int32, device="cuda")
        px = torch.full((w * h,), SENTINEL - (1 << 32), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        hits, nrm, src, dst = g.d_hits.data_ptr(), g.d_nrm.data_ptr(), d_in.data_ptr(), out.data_ptr()

        def code(passes=3, channels=1, sigma=0.05, npow=5, flags=0, hits=hits, nrm=nrm, src=src, dst=dst, p=True,
                 gb=True):
            prm = _lib.RtFilterParams(passes, channels, sigma, npow, flags)
            gbuf = _lib.RtGBuffer(hits, nrm, None)
            return lib.rt_filter_layer(r._h, ctypes.byref(prm) if p else None, ctypes.byref(gbuf) if gb else None,
                                       src, dst, None, None)

        bad = [dict(p=False), dict(gb=False), dict(src=None), dict(dst=None), dict(hits=None), dict(nrm=None),
               dict(src=dst), dict(dst=src)]
        bad += [dict(passes=x) for x in (0, 6, 7, 0xFFFFFFFF)]
        bad += [dict(channels=x) for x in (0, 2, 3, 5, 16)]
        bad += [dict(sigma=x) for x in (0.0, -0.0, -1.0, float("nan"), -INF)]
        bad += [dict(npow=x) for x in (8, 9, 0xFFFFFFFF)]
        bad += [dict(flags=x) for x in (1, 2, 0x80000000)]
        for kw in bad:
            assert code(**kw) == _lib.RT_E_INVALID, kw
            assert b"rt_filter_layer" in lib.rt_last_error(r._h)
        with pytest.raises(_lib.RtError) as e:
            r.filter_layer_device(src, dst, hits, nrm, passes=6)
        assert e.value.code == _lib.RT_E_INVALID
        for kw in (dict(floor=float("nan")), dict(floor=-0.001), dict(floor=1.001), dict(floor=INF), dict(layer=None)):
            a = dict(floor=0.5, layer=src)
            a.update(kw)
            assert lib.rt_apply_layer(r._h, px.data_ptr(), a["layer"], a["floor"], None) == _lib.RT_E_INVALID, kw
            assert b"rt_apply_layer" in lib.rt_last_error(r._h)
        r.synchronize()
        torch.cuda.synchronize()
        assert (out.cpu().numpy().view(np.uint32) == SENTINEL).all()
        assert (px.cpu().numpy().view(np.uint32) == SENTINEL).all()
        assert np.array_equal(qs.bits(d_in.cpu().numpy()), qs.bits(v))
        assert code() == _lib.RT_OK        # and the same arguments, valid, do write
        assert lib.rt_apply_layer(r._h, px.data_ptr(), src, 0.5, None) == _lib.RT_OK
        r.synchronize()
        assert not (out.cpu().numpy().view(np.uint32)[:w * h] == SENTINEL).any()
        assert not (px.cpu().numpy().view(np.uint32) == SENTINEL).all()


def test_the_call_needs_no_scene(gpu):
    """A handle without a scene filters under guides it is given (here: another handle's)."""
    w, h = 37, 29
    with _renderer(w, h) as r:
        g = Guides(r)
        d_in, v = _ao_layer(r)
        with rt.KernelRenderer(w, h, mode="scene") as bare:
            bare.resize(w, h)
            assert _same(_run(bare, g, d_in, v), g.ref(v, 3, 5, 0.05))


@pytest.mark.parametrize("w,h", [(1, 7), (37, 29)])
def test_apply_layer_is_the_reference(gpu, w, h):
    """On the internal framebuffer and on a caller's buffer (one pixel longer,
    sentinel-filled), at floor 0, 0.25 and 1, byte for byte, alpha unchanged."""
    import torch
    with _renderer(w, h) as r:
        if w == 1:   # the 37-wide frame's focal length with the principal point on the single column (ao_ref's `thin`)
            K = rt.resize_intrinsic(37, h).reshape(9).copy()
            K[2] = np.float32(0.25)
            r.setIntrinsic(K)
        d_ao, ao = _ao_layer(r, 16)
        g = np.random.default_rng(w)
        layer = np.where(g.random((h, w)) < 0.5, ao, g.random((h, w)).astype(np.float32)).astype(np.float32)
        d_layer = torch.from_numpy(layer).cuda()
        mine = torch.zeros(w * h + 1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        for floor in (0.0, 0.25, 1.0):
            r.render()
            frame = r.readback()
            assert frame[..., :3].any() and (frame[..., 3] == 255).all()
            r.apply_layer_device(d_layer.data_ptr(), floor)
            got = r.readback()
            want = fr.apply_layer(frame, layer, floor)
            assert np.array_equal(got, want), floor
            assert np.array_equal(got[..., 3], frame[..., 3])
            assert (floor == 1.0) == np.array_equal(got, frame)
            # a caller's buffer, with random alpha; the internal framebuffer stays as it was
            px = g.integers(0, 256, (h, w, 4)).astype(np.uint8)
            mine[:w * h] = torch.from_numpy(px.view(np.int32).reshape(-1)).cuda()
            mine[w * h] = SENTINEL - (1 << 32)
            torch.cuda.synchronize()
            r.apply_layer_device(d_layer.data_ptr(), floor, mine.data_ptr())
            r.synchronize()
            raw = mine.cpu().numpy().view(np.uint32)
            assert raw[w * h] == SENTINEL
            assert np.array_equal(raw[:w * h].view(np.uint8).reshape(h, w, 4), fr.apply_layer(px, layer, floor)), floor
            assert np.array_equal(r.readback(), got)
        assert np.array_equal(qs.bits(d_layer.cpu().numpy()), qs.bits(layer))


def test_python_composites_are_the_separate_calls(gpu):
    """render_ao(filter_passes=...) returns the raw layer and the filtered one of
    render_gbuffer + render_ao + filter_layer; filter_layer (numpy in, numpy out) is
    the reference on one and on four channels."""
    w, h = 70, 9
    with _renderer(w, h) as r:
        gb = r.render_gbuffer(albedo=False)
        raw = r.render_ao(4, 0.1, salt=3)
        assert "ao_filtered" not in raw
        for passes, kw in ((3, {}), (2, dict(depth_sigma=INF, normal_power=0))):
            res = r.render_ao(4, 0.1, salt=3, filter_passes=passes, stats=True, **kw)
            assert np.array_equal(qs.bits(res["ao"]), qs.bits(raw["ao"]))
            assert np.array_equal(res["occluded"], raw["occluded"]) and res["stats"].shadow_rays > 0
            sep = r.filter_layer(raw["ao"], gb, passes, **kw)
            assert sep.shape == (h, w) and sep.dtype == np.float32
            assert np.array_equal(qs.bits(res["ao_filtered"]), qs.bits(sep))
            want = fr.filter_layer(raw["ao"], gb["sphere"], gb["t"], gb["normal"], passes,
                                   kw.get("depth_sigma", 0.05), kw.get("normal_power", 5))
            assert np.array_equal(qs.bits(sep), qs.bits(want))
        v4 = np.random.default_rng(4).random((h, w, 4)).astype(np.float32)
        out4 = r.filter_layer(v4, gb, 5)
        assert out4.shape == (h, w, 4)
        assert np.array_equal(qs.bits(out4), qs.bits(fr.filter_layer(v4, gb["sphere"], gb["t"], gb["normal"], 5)))
        with pytest.raises(ValueError):
            r.filter_layer(v4[:, :, :3], gb)
        with pytest.raises(_lib.RtError):
            r.render_ao(4, 0.1, filter_passes=6)


def test_multi_device_handle_answers_as_a_single_one(gpu):
    w, h = 37, 29
    with _renderer(w, h) as r:
        g = Guides(r)
        d_in, v = _ao_layer(r)
        single = _run(r, g, d_in, v)
    with _renderer(w, h, devices=[0, 0], transport="peer") as r:
        r.render()
        g2 = Guides(r)
        d2, v2 = _ao_layer(r)
        assert np.array_equal(qs.bits(v2), qs.bits(v)) and np.array_equal(g2.sphere, g.sphere)
        assert np.array_equal(_run(r, g2, d2, v2), single)
        frame = r.readback()
        r.apply_layer_device(d2.data_ptr(), 0.25)
        assert np.array_equal(r.readback(), fr.apply_layer(frame, v2, 0.25))


def test_cli_ao_filter_file_is_the_python_layer(gpu, tmp_path):
    """rt_cli --ao FILE --ao-filter 3: the PGM holds the filtered layer,
    (uint8)(value * 255) (the CLI's scene is generate_spheres(n, SEED) seen from
    scene_pose())."""
    from raytracingstudy_amd.camera import scene_pose
    cli = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "raytracingstudy_amd", "rt_cli")
    w, h, rays, radius = 67, 45, 4, 0.25
    out = tmp_path / "ao.pgm"
    p = subprocess.run([cli, "--config", "c2", "--spheres", "1000", "--width", str(w), "--height", str(h),
                        "--frames", "1", "--ao", str(out), "--ao-rays", str(rays), "--ao-radius", str(radius),
                        "--ao-filter", "3", "--test-poison"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    raw = out.read_bytes()
    head = f"P5\n{w} {h}\n255\n".encode()
    assert raw.startswith(head) and len(raw) == len(head) + w * h
    sp, al = rt.generate_spheres(1000, rt.SEED)
    with rt.KernelRenderer(w, h, mode="scene") as r:
        r.resize(w, h)
        r.setPosition(scene_pose())
        r.set_scene(sp, al, max_depth=7)
        res = r.render_ao(rays, radius, filter_passes=3)
    grey = np.clip(np.floor(res["ao_filtered"] * np.float32(255.0)), 0, 255).astype(np.uint8)
    assert np.array_equal(np.frombuffer(raw[len(head):], np.uint8).reshape(h, w), grey)
    plain = ((rays - res["occluded"].astype(np.int64)) * 255 // rays).astype(np.uint8)
    assert not np.array_equal(grey, plain)       # the file is not the unfiltered layer
    assert f"ao: {int(res['occluded'].sum())} of " in p.stdout and "ao-filter: 3 passes, " in p.stdout
