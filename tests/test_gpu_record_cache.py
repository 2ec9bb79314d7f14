"""The derived record arrays of one renderer across camera and scene changes.

A scene frame reads four device arrays derived from the scene's leaf
references: the camera-relative records (remade when the camera origin or the
scene changes), the image-plane records (origin, basis), the light-plane
records with the occluder lists (scene, light) and the albedo by reference
(scene).  rt_frame.cpp keeps each with the scene generation and the key it was
made for (DerivedRecords) and remakes it when either differs or the array was
reallocated.  A stale array shows as wrong pixels or counters, so ONE renderer
is walked through every kind of change, and every frame's RGBA8, radiance and
four counters are compared with the oracle as tests/test_gpu_parity.py does.
"""
import functools

import numpy as np
import pytest

import raytracingstudy_amd as rt
from raytracingstudy_amd.camera import display_pose, scene_pose, translation_pose

pytestmark = pytest.mark.gpu

SPP = 8
MOVED = (0.64 + 0.05, 0.64, 2.2)


@functools.lru_cache(maxsize=None)
def _scene(n):
    import oracle
    sp, al = rt.generate_spheres(n, rt.SEED)
    return sp, al, oracle.Scene(sp, al)


def _frame_equals_oracle(r, n, w, h, pose, step):
    sp, al, sc = _scene(n)
    r.setPosition(pose)
    r.render()
    img, rad = r.readback(), r.readback_radiance()
    st = r.render(stats=True)
    assert np.array_equal(r.readback(), img), step
    _, K = r.camera()
    ref8, ref32, cnt = sc.render(w, h, pose, K, spp=SPP)
    assert np.array_equal(img, ref8), step
    assert np.array_equal(rad, ref32), step
    assert (st.primary_rays, st.shadow_rays, st.nodes_visited, st.prims_tested) == tuple(
        int(c) for c in cnt), step


def test_records_follow_camera_scene_and_size(gpu, oracle):
    """Steps 1-7 on one renderer: a new origin (all camera records), a new
    rotation at the same origin (the image-plane records only), a larger scene
    (every array reallocates), a smaller one (no reallocation, a new scene
    generation), another frame size, and the first pose again."""
    w, h = 96, 64
    with rt.KernelRenderer(w, h, mode="scene", spp=SPP, radiance=True) as r:
        r.resize(w, h)
        r.set_scene(*_scene(1000)[:2])
        _frame_equals_oracle(r, 1000, w, h, scene_pose(), 1)
        _frame_equals_oracle(r, 1000, w, h, translation_pose(*MOVED), 2)
        yawed = display_pose(MOVED, 4.0, 0.0)
        assert np.array_equal(yawed[3], translation_pose(*MOVED)[3])
        _frame_equals_oracle(r, 1000, w, h, yawed, 3)
        r.set_scene(*_scene(4000)[:2])
        _frame_equals_oracle(r, 4000, w, h, yawed, 4)
        r.set_scene(*_scene(500)[:2])
        _frame_equals_oracle(r, 500, w, h, yawed, 5)
        r.resize(64, 96)
        _frame_equals_oracle(r, 500, 64, 96, yawed, 6)
        _frame_equals_oracle(r, 500, 64, 96, scene_pose(), 7)


def test_albedo_records_made_by_gbuffer_before_first_frame(gpu, oracle):
    """Step 8: the albedo by leaf reference is made by whichever of
    rt_render_gbuffer and the first frame comes first, and serves the other."""
    w, h = 96, 64
    sp, al, _ = _scene(1000)
    with rt.KernelRenderer(w, h, mode="scene", spp=SPP, radiance=True) as r:
        r.resize(w, h)
        r.setPosition(scene_pose())
        r.set_scene(sp, al)
        g = r.render_gbuffer(normals=False, albedo=True)
        hit = g["sphere"] != 0xFFFFFFFF
        assert hit.any() and not hit.all()
        assert np.array_equal(g["albedo"][hit], al[g["sphere"][hit]])
        assert not g["albedo"][~hit].any()
        _frame_equals_oracle(r, 1000, w, h, scene_pose(), 8)
