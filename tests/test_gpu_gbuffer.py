"""The first-hit G-buffer (rt_render_gbuffer) against the CPU oracle, pixel by pixel.

The kernel builds pixel (x, y)'s centre ray in registers and runs the frame
kernels' own walk in its generic mode, so every pixel's t (bit for bit),
sphere index and the summed node / prim counters must equal oracle.get_ray +
oracle.Scene.trace; the normal is restated here in numpy float32, one
rounding per operation (hit_shade's operations), and the albedo is gathered by
sphere index.  Every output buffer is pre-filled with 0xAB bytes and is one
record longer than the frame: an unwritten pixel and a write past the end
both show.  The expectation of a case is computed once and shared.
"""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import raytracingstudy_amd as rt
from raytracingstudy_amd import _lib
from raytracingstudy_amd.camera import scene_pose, translation_pose

import gbuffer_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "raytracingstudy_amd", "rt_cli")
NO_HIT = 0xFFFFFFFF
NO_ALBEDO = 0xFFCCCCCC
# test_gpu_query.py's two scenes.  A: 577 nodes, deepest leaf at depth 4.
# B: a deep tree of small leaves with many overlapping spheres.
SCENES = {"A": dict(n=1000, max_depth=7, leaf_capacity=8),
          "B": dict(n=20000, max_depth=12, leaf_capacity=2)}


def _away_pose():
    """Identity rotation above the cloud: +z is forward, away from the root box."""
    p = np.eye(4, dtype=np.float32)
    p[3, :3] = (0.64, 0.64, 2.2)
    return p


def _inside_pose():
    """Inside sphere 0 of scene B, a quarter radius off its centre on each axis."""
    c = _spheres("B")[0][0]
    return translation_pose(*(c[:3] + np.float32(0.25) * c[3]))


POSES = {"scene": scene_pose,                                    # outside, looking at the cloud
         "centre": lambda: translation_pose(0.64, 0.64, 0.64),   # inside the cloud: many pops
         "away": _away_pose,
         "inside": _inside_pose}


@functools.lru_cache(maxsize=None)
def _spheres(name):
    return rt.generate_spheres(SCENES[name]["n"], rt.SEED)


@functools.lru_cache(maxsize=None)
def _oracle_scene(name):
    import oracle
    sp, al = _spheres(name)
    return oracle.Scene(sp, al, max_depth=SCENES[name]["max_depth"],
                        leaf_capacity=SCENES[name]["leaf_capacity"])


def _intrinsic(w, h, custom):
    """The resize intrinsic, or one with unequal focal lengths and an off-centre
    principal point (flat indices as Camera::getRay reads them: 0, 4 focal, 2, 5 centre)."""
    import oracle
    K = oracle.resize_intrinsic(w, h).reshape(9).copy()
    if custom:
        K[0] *= np.float32(0.8)
        K[4] *= np.float32(1.3)
        K[2] += np.float32(3.25)
        K[5] -= np.float32(2.5)
    return K


@functools.lru_cache(maxsize=None)
def _expected(name, w, h, pose="scene", custom_k=False):
    """The oracle's G-buffer: t (h, w) f32, sphere (h, w) u32, normal (h, w, 4) f32,
    albedo (h, w) u32, and the summed node / prim counters."""
    import oracle
    sp, al = _spheres(name)
    return gbuffer_ref.expected(oracle, _oracle_scene(name), sp, al, POSES[pose](), _intrinsic(w, h, custom_k), w, h)


def _renderer(name, w, h, pose="scene", custom_k=False, albedo=True, **kw):
    sp, al = _spheres(name)
    r = rt.KernelRenderer(w, h, mode="scene", **kw)
    r.resize(w, h)
    if custom_k:
        r.setIntrinsic(_intrinsic(w, h, True))
    r.setPosition(POSES[pose]())
    r.set_scene(sp, al if albedo else None, max_depth=SCENES[name]["max_depth"],
                leaf_capacity=SCENES[name]["leaf_capacity"])
    return r


def _run(r, w, h, hits=True, normals=True, albedo=True, stream=None, stats=False, device="cuda"):
    """rt_render_gbuffer into 0xAB-filled buffers of w*h + 1 records; the guard
    record of each must come back untouched."""
    import torch
    n = w * h
    bufs = {k: torch.full((n + 1, size), 0xAB, dtype=torch.uint8, device=device)
            for k, size, on in (("hits", 8, hits), ("normals", 16, normals), ("albedo", 4, albedo)) if on}
    if stream is None:
        torch.cuda.synchronize()
    ptr = {k: bufs[k].data_ptr() if k in bufs else None for k in ("hits", "normals", "albedo")}
    st = r.render_gbuffer_device(ptr["hits"], ptr["normals"], ptr["albedo"], stream=stream, stats=stats)
    if stream is None:
        r.synchronize()
    out = {"stats": st}
    for k, b in bufs.items():
        raw = b.cpu().numpy()  # on a caller's stream: ordered after the launch
        assert (raw[n] == 0xAB).all(), k
        out[k] = raw[:n].copy()
    if hits:
        hv = out["hits"].view(np.uint32).reshape(h, w, 2)
        out["t"] = np.ascontiguousarray(hv[..., 0]).view(np.float32)
        out["sphere"] = np.ascontiguousarray(hv[..., 1])
    if normals:
        out["normal"] = out["normals"].view(np.float32).reshape(h, w, 4)
    if albedo:
        out["albedo"] = out["albedo"].view(np.uint32).reshape(h, w)
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _assert_equal(got, exp, hits=True, normals=True, albedo=True):
    if hits:
        assert np.array_equal(got["sphere"], exp["sphere"])
        assert np.array_equal(_bits(got["t"]), _bits(exp["t"]))        # bit for bit, a miss's +inf included
    if normals:
        assert np.array_equal(_bits(got["normal"]), _bits(exp["normal"]))  # a miss: four +0.0, not NaN
    if albedo:
        assert np.array_equal(got["albedo"], exp["albedo"])


def _assert_stats(st, exp, w, h):
    assert st.primary_rays == w * h
    assert st.nodes_visited == exp["nodes"] and st.prims_tested == exp["prims"]
    assert (st.shadow_rays, st.samples_per_pixel) == (0, 0)
    assert st.ms > 0.0


# 96x64: whole 16x16 blocks; 67x45: partial tiles on both edges; then a single
# pixel, one partial wave row and one partial wave column over five blocks
@pytest.mark.parametrize("w,h", [(96, 64), (67, 45), (1, 1), (8, 1), (1, 70)])
def test_shapes(gpu, oracle, w, h):
    exp = _expected("A", w, h)
    with _renderer("A", w, h) as r:
        got = _run(r, w, h, stats=True)
        _assert_equal(got, exp)
        _assert_stats(got["stats"], exp, w, h)
        # the Python convenience wrapper returns the same arrays
        res = r.render_gbuffer()
        assert res["t"].shape == (h, w) and res["normal"].shape == (h, w, 4)
        _assert_equal(res, exp)
        assert "stats" not in res and "normal" not in r.render_gbuffer(normals=False)


@pytest.mark.parametrize("cell_table", [None, 2, 3, 0])
def test_deep_scene_cell_tables_and_stats(gpu, oracle, cell_table):
    """Scene B with the auto cell table, depth-2 and depth-3 ones (jumps and
    re-entries) and none (descents and stack pops only): buffers and counters."""
    w, h = 67, 45
    exp = _expected("B", w, h)
    with _renderer("B", w, h, cell_table=cell_table) as r:
        got = _run(r, w, h, stats=True)
        _assert_equal(got, exp)
        _assert_stats(got["stats"], exp, w, h)
        _assert_equal(_run(r, w, h), exp)  # the plain launch (no counters) answers the same


@pytest.mark.parametrize("name,pose,custom_k", [("B", "scene", False), ("B", "centre", False),
                                                ("A", "centre", False), ("B", "scene", True),
                                                ("B", "away", False)])
def test_poses(gpu, oracle, name, pose, custom_k):
    w, h = 67, 45
    exp = _expected(name, w, h, pose, custom_k)
    with _renderer(name, w, h, pose, custom_k) as r:
        got = _run(r, w, h, stats=True)
        _assert_equal(got, exp)
        _assert_stats(got["stats"], exp, w, h)
        if pose == "away":  # no ray enters the root box
            assert (got["sphere"] == NO_HIT).all() and np.isposinf(got["t"]).all()
            assert not got["normals"].any() and not got["albedo"].any()
            assert got["stats"].nodes_visited == 0 and got["stats"].prims_tested == 0


def test_cases_are_not_vacuous(oracle):
    """A condition on the inputs, on the oracle's own answers: every case that
    looks at the cloud has at least 10% hits and 10% misses; the away pose none."""
    cases = [("A", 96, 64, "scene", False), ("A", 67, 45, "scene", False), ("B", 67, 45, "scene", False),
             ("A", 67, 45, "centre", False), ("B", 67, 45, "centre", False), ("B", 67, 45, "scene", True)]
    for c in cases:
        frac = float((_expected(*c)["sphere"] != NO_HIT).mean())
        assert 0.10 <= frac <= 0.90, (c, frac)
    assert not (_expected("B", 67, 45, "away")["sphere"] != NO_HIT).any()


def test_camera_inside_a_sphere_reports_the_far_root(gpu, oracle):
    """The camera sits inside sphere 0 of scene B, so every pixel hits (the 10%
    misses asked of the other cases cannot exist here).  Where sphere 0 itself is
    the nearest hit, t is its far root: the normal points along the ray."""
    w, h = 24, 17
    exp = _expected("B", w, h, "inside")
    assert (exp["sphere"] != NO_HIT).all() and (exp["t"] > 0).all()
    own = exp["sphere"] == 0
    assert own.sum() >= w * h // 10  # a condition on the inputs, on the oracle's answers
    assert ((exp["normal"][own][:, :3] * exp["dirs"][own]).sum(axis=1) > 0).all()
    with _renderer("B", w, h, "inside") as r:
        got = _run(r, w, h, stats=True)
        _assert_equal(got, exp)
        _assert_stats(got["stats"], exp, w, h)


def test_consistent_with_pick_trace_rays_and_the_frame(gpu, oracle):
    """No oracle in the comparisons: the hits buffer equals rt_pick pixel by
    pixel and rt_trace_rays on the same rays, and a 1-spp unjittered frame
    shows the miss colour (R = 200) exactly where the id buffer says no hit."""
    w, h = 96, 64
    exp = _expected("A", w, h)
    with _renderer("A", w, h, spp=1, jitter=False) as r:
        got = _run(r, w, h)
        g = np.random.default_rng(7)
        for x, y in zip(g.integers(0, w, 32), g.integers(0, h, 32)):
            hit, t, sphere, _ = r.pick(float(x), float(y))
            assert sphere == got["sphere"][y, x] and hit == (sphere != NO_HIT)
            assert np.float32(t).view(np.uint32) == got["t"][y, x].view(np.uint32)
        rays = np.zeros((w * h, 8), np.float32)
        rays[:, :3] = scene_pose()[3, :3]
        rays[:, 4:7] = exp["dirs"].reshape(-1, 3)
        rays[:, 7] = np.inf
        t, sphere = r.trace_rays(rays)
        assert np.array_equal(sphere.reshape(h, w), got["sphere"])
        assert np.array_equal(_bits(t).reshape(h, w), _bits(got["t"]))
        r.render()
        img = r.readback()
        assert np.array_equal(img[..., 0] == 200, got["sphere"] == NO_HIT)


def test_optional_buffers_and_errors(gpu, oracle):
    w, h = 67, 45
    exp = _expected("A", w, h)
    lib = _lib.load()
    with rt.KernelRenderer(w, h, mode="scene") as r:
        r.resize(w, h)
        r.setPosition(scene_pose())
        fb = r.framebuffer_ptr()  # any valid device address: the call must refuse before using it
        with pytest.raises(_lib.RtError) as e:  # no scene yet
            r.render_gbuffer_device(fb)
        assert e.value.code == _lib.RT_E_NOSCENE
        sp, al = _spheres("A")
        r.set_scene(sp, al, max_depth=7, leaf_capacity=8)
        with pytest.raises(_lib.RtError) as e:
            r.render_gbuffer_device(None, None, None)
        assert e.value.code == _lib.RT_E_INVALID
        assert lib.rt_render_gbuffer(r._h, None, None, None) == _lib.RT_E_INVALID
        full = _run(r, w, h)
        _assert_equal(full, exp)
        for only in ("hits", "normals", "albedo"):
            sel = {k: k == only for k in ("hits", "normals", "albedo")}
            got = _run(r, w, h, **sel)
            assert np.array_equal(got[only], full[only]), only
            _assert_equal(got, exp, **sel)
    # a scene set without albedo: the frames' default word on every hit pixel
    with _renderer("A", w, h, albedo=False) as r:
        got = _run(r, w, h)
        hit = exp["sphere"] != NO_HIT
        assert (got["albedo"][hit] == NO_ALBEDO).all() and not got["albedo"][~hit].any()
        _assert_equal(got, exp, albedo=False)


def test_frames_are_undisturbed(gpu):
    """A progressive renderer's frames 0 and 1 are byte-equal with and without
    G-buffer calls (a stats one included) between them, the stats frame after
    them counts the same, and the call leaves the internal framebuffer alone."""
    w, h = 67, 45

    def frames(with_gbuffer):
        out = []
        with _renderer("A", w, h, spp=2, progressive=True) as r:
            for _ in range(2):
                r.render()
                out.append(r.readback())
                if with_gbuffer:
                    _run(r, w, h)
                    _run(r, w, h, stats=True)
                    assert np.array_equal(r.readback(), out[-1])
            st = r.render(stats=True)
            out.append(r.readback())
        return out, (st.primary_rays, st.shadow_rays, st.nodes_visited, st.prims_tested,
                     st.samples_per_pixel)

    plain, st_plain = frames(False)
    mixed, st_mixed = frames(True)
    for a, b in zip(plain, mixed):
        assert np.array_equal(a, b)
    assert st_plain == st_mixed and st_plain[4] == 6
    assert not np.array_equal(plain[0], plain[1])  # the sums did accumulate


def test_device_pointers_on_a_torch_stream(gpu, oracle):
    import torch
    w, h = 67, 45
    exp = _expected("A", w, h)
    with _renderer("A", w, h) as r:
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            got = _run(r, w, h, stream=s.cuda_stream)  # fills, launch and copies all on s
            assert got["stats"] is None
            _assert_equal(got, exp)
        s.synchronize()
        r.synchronize()


def test_multi_device_handle_answers_from_device_0(gpu, oracle):
    w, h = 67, 45
    exp = _expected("A", w, h)
    with _renderer("A", w, h, devices=[0, 0], transport="peer") as r:
        r.render()
        got = _run(r, w, h, stats=True)
        _assert_equal(got, exp)          # the whole frame, not devices[0]'s tiles
        _assert_stats(got["stats"], exp, w, h)
        _assert_equal(r.render_gbuffer(), exp)


def test_cli_gbuffer_file_equals_the_python_result(gpu, tmp_path):
    """rt_cli --gbuffer: W*H raw rt_hit records of the frame's camera (the CLI's
    scene is generate_spheres(n, SEED) seen from scene_pose())."""
    w, h = 67, 45
    out = tmp_path / "hits.bin"
    p = subprocess.run([CLI, "--config", "c2", "--spheres", "1000", "--width", str(w), "--height", str(h),
                        "--frames", "1", "--gbuffer", str(out), "--test-poison"],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    raw = np.fromfile(out, np.uint8)
    assert raw.size == w * h * ctypes.sizeof(_lib.RtHit)
    with _renderer("A", w, h) as r:
        got = _run(r, w, h, normals=False, albedo=False)
    assert np.array_equal(raw, got["hits"].reshape(-1))
    n_hit = int((got["sphere"] != NO_HIT).sum())
    assert f"gbuffer: {n_hit} of {w * h} pixels hit a sphere" in p.stdout
