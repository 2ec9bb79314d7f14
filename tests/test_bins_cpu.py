"""The screen-space bins' per-sphere arithmetic (csrc/rt_bins_math.h, DESIGN.md
5.1 round 10) on the CPU: tests/native/bins_math_dump.cpp, built with the
address and undefined-behaviour sanitizers, prints every sphere's class, pixel
rectangle and near bound for a camera; the oracle's primary hits must lie
inside them.
"""
import numpy as np
import pytest

import raytracingstudy_amd as rt
from raytracingstudy_amd.camera import display_pose, scene_pose, translation_pose

from bins_native import BINNED, DROPPED, WIDE, build_dump, cam_args as _cam_args, rects as _rects
from bins_oracle import look_at_pose, primary_hits


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    return build_dump(tmp_path_factory.mktemp("bin"))


POSES = {
    "scene": scene_pose(),
    "yaw_pitch": look_at_pose((0.1, 0.9, 2.0)),
    "steep": look_at_pose((1.9, 1.6, 1.9)),
    "inside_box": translation_pose(0.64, 0.64, 0.9),
    "close": look_at_pose((0.3, 0.5, 1.5), (0.7, 0.6, 0.6)),
    # a 16x focal length: spheres a few pixels across, as in the 1080p configs
    "zoom": scene_pose(),
}


@pytest.mark.parametrize("pose_name", list(POSES))
def test_oracle_primary_hits_lie_in_the_rectangles(dump, oracle, pose_name):
    """Every oracle primary hit (pixel, sphere, t): the pixel is inside the
    sphere's rectangle (or the sphere is wide) and t >= its near bound."""
    w, h, spp = 48, 32, 4
    sp, al = rt.generate_spheres(3000, rt.SEED)
    pose, K = POSES[pose_name], rt.resize_intrinsic(w, h)
    if pose_name == "zoom":
        K = np.array(K, np.float32).copy()
        K[0, 0] *= 16.0
        K[1, 1] *= 16.0
    cls, rect, near = _rects(dump, sp, pose, K, w, h)
    s = oracle.Scene(sp, al)
    x, y, j, t = primary_hits(oracle, s, pose, K, w, h, spp)
    assert x.shape[0] > 400
    assert np.all(cls[j] != DROPPED), "a hit sphere was dropped"
    b = cls[j] == BINNED
    r = rect[j]
    inside = (r[:, 0] <= x) & (x <= r[:, 2]) & (r[:, 1] <= y) & (y <= r[:, 3])
    assert np.all(inside[b]), f"{int((~inside[b]).sum())} hits outside their sphere's rectangle"
    assert np.all(t >= near[j]), "a hit nearer than its sphere's near bound"
    if pose_name == "zoom":
        # the rectangles are tight: the sphere's own few pixels, not the image
        area = (r[b, 2] - r[b, 0] + 1) * (r[b, 3] - r[b, 1] + 1)
        assert np.median(area) <= 64
        # negative control: rectangles from radii x 0.9 lose hits
        _, rect9, _ = _rects(dump, sp, pose, K, w, h, shrink=0.9)
        r9 = rect9[j]
        in9 = (r9[:, 0] <= x) & (x <= r9[:, 2]) & (r9[:, 1] <= y) & (y <= r9[:, 3])
        assert not np.all(in9[b]), "the check cannot see an unsound rectangle"
    s.close()


def test_classes_on_hand_made_spheres(dump):
    """Camera at the origin looking down +z (identity rotation)."""
    w, h = 64, 48
    pose = np.eye(4, dtype=np.float32)
    K = rt.resize_intrinsic(w, h)
    sp = np.array([
        [0.0, 0.0, 5.0, 0.5],      # 0 in front, on the axis: binned around the centre
        [0.0, 0.0, -5.0, 0.5],     # 1 wholly behind the camera plane: dropped
        [0.0, 0.0, 0.2, 0.5],      # 2 holds the camera: wide
        [3.0, 0.0, 0.1, 0.5],      # 3 straddles the camera plane beside the camera: wide
        [3.0, 0.0, -0.4999, 0.5],  # 4 touches the plane within the slack: wide
        [100.0, 0.0, 5.0, 0.5],    # 5 in front, far off the image: dropped
        [0.0, 0.0, 0.6, 0.5],      # 6 just in front: binned, covers the image
        [0.0, 0.0, 1e30, 1.0],     # 7 finite but absurdly far: binned at the centre
    ], np.float32)
    cls, rect, near = _rects(dump, sp, pose, K, w, h)
    assert list(cls) == [BINNED, DROPPED, WIDE, WIDE, WIDE, DROPPED, BINNED, BINNED]
    f = float(K.reshape(-1)[0])
    cx, cy = w // 2, h // 2
    half = f * 0.5 / np.sqrt(25.0 - 0.25)    # the tangent-line extent of sphere 0
    assert rect[0, 0] == int(np.floor(cx - half - 1 / 64)) and rect[0, 2] == int(np.floor(cx + half + 1 / 64))
    assert rect[0, 1] == int(np.floor(cy - half - 1 / 64)) and rect[0, 3] == int(np.floor(cy + half + 1 / 64))
    assert 4.49 < near[0] <= 4.5 and near[2] == 0.0 and near[3] == 0.0
    assert tuple(rect[6]) == (0, 0, w - 1, h - 1) and 0.09 < near[6] <= 0.1
    assert tuple(rect[7]) == (cx - 1, cy - 1, cx, cy)   # the centre +- the pixel slack


def test_camera_gate(dump):
    K = rt.resize_intrinsic(96, 64)
    assert dump("camok", *_cam_args(scene_pose(), K)).strip() == "1"
    assert dump("camok", *_cam_args(display_pose((0.1, 0.9, 2.0), 33.0, -17.0), K)).strip() == "1"
    sheared = np.array(scene_pose(), np.float32).copy()
    sheared[0, 1] = 0.01
    assert dump("camok", *_cam_args(sheared, K)).strip() == "0"
    scaled = np.array(scene_pose(), np.float32).copy()
    scaled[:3, :3] *= 1.001
    assert dump("camok", *_cam_args(scaled, K)).strip() == "0"
    K0 = np.array(K, np.float32).copy().reshape(-1)
    K0[0] = 0.0
    assert dump("camok", *_cam_args(scene_pose(), K0)).strip() == "0"
    nan = np.array(scene_pose(), np.float32).copy()
    nan[3, 0] = np.nan
    assert dump("camok", *_cam_args(nan, K)).strip() == "0"
