"""What test_gpu_query.py, test_gpu_multihit.py, test_gpu_overlap.py and
test_gpu_closest.py share: a renderer over a named test scene, a float's bits,
and the check that queries between frames leave the frames alone.
"""
import numpy as np

import raytracingstudy_amd as rt
from raytracingstudy_amd.camera import scene_pose

import overlap_ref as ov

CAM_W, CAM_H = 96, 64


def _overlap_ref_scene(name):
    return ov.spheres(name), None, ov.TREES[name]


def scene_renderer(name, w=CAM_W, h=CAM_H, scene=_overlap_ref_scene, **kw):
    """A scene-mode renderer at scene_pose() over scene(name) -> (spheres, albedo
    or None, set_scene's octree arguments); overlap_ref's scenes unless given."""
    sp, al, tree = scene(name)
    r = rt.KernelRenderer(w, h, mode="scene", **kw)
    r.resize(w, h)
    r.setPosition(scene_pose())
    r.set_scene(sp, al, **tree)
    return r


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_frames_undisturbed(make_renderer, between):
    """A progressive sequence of 3 frames with between(r) after each is byte-equal
    to the same frames without it, and a stats frame after them counts what it
    counts without them (accumulated samples included).  make_renderer(spp=2,
    progressive=True) -> the renderer."""
    def frames(query):
        out = []
        with make_renderer(spp=2, progressive=True) as r:
            for _ in range(3):
                r.render()
                out.append(r.readback())
                if query:
                    between(r)
            st = r.render(stats=True)
            out.append(r.readback())
        return out, (st.primary_rays, st.shadow_rays, st.nodes_visited, st.prims_tested,
                     st.samples_per_pixel)

    plain, st_plain = frames(False)
    mixed, st_mixed = frames(True)
    for a, b in zip(plain, mixed):
        assert np.array_equal(a, b)
    assert st_plain == st_mixed and st_plain[4] == 8
    assert not np.array_equal(plain[0], plain[2])  # the sums did accumulate
