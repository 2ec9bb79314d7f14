"""The screen-space bins' per-sphere arithmetic (csrc/rt_bins_math.h, DESIGN.md
5.1 round 10) on the CPU: tests/native/bins_math_dump.cpp, built with the
address and undefined-behaviour sanitizers, prints every sphere's class, pixel
rectangle and near bound for a camera; the oracle's primary hits must lie
inside them.  The same program steps the host's build policy (when a dense
scene is probed again, how large the entry buffer is) through scripted frames.
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


# ---- the host's build policy (rt_bins_math.h: bin_dense_skip_step, bin_entries_wanted) ----

DENSE, CAPACITY, WIDE_FLAG = 4, 1, 2        # kBinFlagDense, kBinFlagCapacity, kBinFlagWide
SKIP = 15                                   # kBinDenseSkip


def _cadence(dump, frames):
    """frames: (scene generation, mirror frame word, mirror flag word) per plain
    frame 1, 2, ...; returns 'skip' | 'build' per frame."""
    return dump("cadence", *["%d,%d,%d" % f for f in frames]).split()


def test_dense_observation_skips_15_frames_then_builds(dump):
    """test_dense_skip_cadence's rule (test_gpu_bins.py) on the CPU: frame 1
    builds; frame 2 sees that build's words say "dense" and is the first of
    exactly kBinDenseSkip skipped frames; frame 17 probes (builds) again, and
    its own "dense" words start the next 15."""
    frames = [(1, 0, 0)] + [(1, 1, DENSE)] * 16 + [(1, 17, DENSE)] * 16
    got = _cadence(dump, frames)
    assert got == ["build"] + ["skip"] * SKIP + ["build"] + ["skip"] * SKIP + ["build"]


def test_stale_observation_is_ignored(dump):
    """Words whose frame id is not the last building frame's (the build's copy
    has not landed yet, or they are an older frame's) start no skip."""
    got = _cadence(dump, [(1, 0, 0), (1, 7, DENSE), (1, 1, DENSE), (1, 2, DENSE)])
    # every frame builds, so each sees the words of a frame before the last building one
    assert got == ["build", "build", "build", "build"]
    # frame 2's build lands late: frame 3 is the first to see it, and to skip
    got = _cadence(dump, [(1, 0, 0), (1, 0, DENSE), (1, 2, DENSE)] + [(1, 2, DENSE)] * SKIP)
    assert got == ["build", "build"] + ["skip"] * SKIP + ["build"]


def test_new_scene_generation_zeroes_the_count(dump):
    """A scene change in the middle of a skip: the next frame builds."""
    frames = [(1, 0, 0)] + [(1, 1, DENSE)] * 5 + [(2, 1, DENSE)] * 3
    got = _cadence(dump, frames)
    # (frame 7's words still name frame 1, which is used up: no new skip either)
    assert got == ["build"] + ["skip"] * 5 + ["build"] * 3


@pytest.mark.parametrize("flag", [0, CAPACITY, WIDE_FLAG, DENSE | CAPACITY, DENSE | WIDE_FLAG])
def test_only_the_dense_flag_alone_starts_a_skip(dump, flag):
    frames = [(1, 0, 0)] + [(1, i, flag) for i in range(1, 20)]   # every frame sees its predecessor's words
    assert _cadence(dump, frames) == ["build"] * 20


CLAMP = 0x7FFFFFFF // 4


def _want(dump, captest=0, n=0, mframe=0, mflag=0, mentries=0, lastframe=0, ent_n=0):
    return int(dump("want", captest, n, mframe, mflag, mentries, lastframe, ent_n))


@pytest.mark.parametrize("n", [0, 1, 1 << 24])
def test_entry_buffer_default_and_test_capacity(dump, n):
    assert _want(dump, n=n) == 6 * n + 65536
    assert _want(dump, captest=16, n=n) == 16


@pytest.mark.parametrize("n", [0, 1, 1 << 24])
@pytest.mark.parametrize("E", [17, 1 << 20, 0x7FFFFFFF])
def test_entry_buffer_grows_after_an_overflow(dump, n, E):
    """The last building frame (id 9) reported E entries that did not fit: at
    least E + E / 4 (0x7FFFFFFF reaches the clamp with no overflow of the
    size_t arithmetic: the sanitizer build would report one)."""
    for captest in (0, 16):
        base = captest or 6 * n + 65536
        got = _want(dump, captest=captest, n=n, mframe=9, mflag=CAPACITY, mentries=E, lastframe=9)
        assert got == min(max(base, E + E // 4), CLAMP)
        assert got >= min(E + E // 4, CLAMP)
        # with the dense or wide bit beside it the capacity bit still counts
        assert _want(dump, captest=captest, n=n, mframe=9, mflag=CAPACITY | DENSE, mentries=E,
                     lastframe=9) == got
        # not the last building frame's words, no building frame yet, or no overflow: ignored
        assert _want(dump, captest=captest, n=n, mframe=8, mflag=CAPACITY, mentries=E, lastframe=9) == base
        assert _want(dump, captest=captest, n=n, mframe=0, mflag=CAPACITY, mentries=E, lastframe=0) == base
        assert _want(dump, captest=captest, n=n, mframe=9, mflag=DENSE, mentries=E, lastframe=9) == base


@pytest.mark.parametrize("n", [0, 1, 1 << 24])
def test_entry_buffer_never_falls_below_half_the_current_one(dump, n):
    base = 6 * n + 65536
    for ent_n in (0, 2, 2 * base - 2, 2 * base, 2 * base + 2, 8 * base + 1, 2 * CLAMP, 2 * CLAMP + 2, 1 << 40):
        assert _want(dump, n=n, ent_n=ent_n) == min(max(base, ent_n // 2), CLAMP)
    # ... whatever the test capacity or an overflow report says
    assert _want(dump, captest=16, n=n, ent_n=4096) == 2048
    assert _want(dump, n=n, mframe=3, mflag=CAPACITY, mentries=17, lastframe=3, ent_n=8 * base) == 4 * base


def test_entry_buffer_clamp(dump):
    assert _want(dump, captest=1 << 24, n=1 << 24) == 1 << 24
    assert _want(dump, n=0xFFFFFFFF) == CLAMP
    assert _want(dump, n=1, mframe=1, mflag=CAPACITY, mentries=0xFFFFFFFF, lastframe=1, ent_n=(1 << 64) - 1) == CLAMP
