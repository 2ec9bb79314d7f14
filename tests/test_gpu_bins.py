"""Screen-space bins: plain wave-queue frames answer
their primary rays from per-frame lists of the spheres each 8x8-pixel bin's
samples can meet (csrc/screen_bins.hip builds them inside every frame,
csrc/rt_bins.h tests them).

Frames of the two algorithms (plain = bins, stats = walk) against each other
and the oracle, byte for byte; the lists' soundness against the oracle's
primary hits; the cameras that send spheres to the wide list or the frame to
the walk; a moving camera; the fallbacks and switches.

Scenes: test_gpu_occluders' "U" (3,000 generator spheres) and "K" (1,500 in
one dense cluster), and "S", U's first 300 spheres: sparse enough that a camera
inside the root box has only a few spheres across its camera plane.
"""
import numpy as np
import pytest

import raytracingstudy_amd as rt
from raytracingstudy_amd._lib import RtError
from raytracingstudy_amd.camera import scene_pose, translation_pose

from bins_oracle import look_at_pose, primary_hits
from test_gpu_occluders import SCENES as OCC_SCENES, _check_frames, _renderer

pytestmark = pytest.mark.gpu

WALK = 0xFFFFFFFF
BIN = 8
WIDE_CAP = 32     # kBinWideCap
SCENES = dict(OCC_SCENES)
SCENES["S"] = (OCC_SCENES["U"][0][:300].copy(), OCC_SCENES["U"][1][:300].copy())


@pytest.fixture
def hooks(monkeypatch):
    """Bins at every frame size and list length; K on occluder lists (as in
    test_gpu_occluders)."""
    def set_(scene="U", cap=None, capacity=None, shrink=False, mean="1000000"):
        monkeypatch.setenv("RT_TEST_BIN_MIN_SAMPLES", "0")
        # (3,000 spheres on a 96x64 frame: ~45 a bin and more; the product's
        # rule would send most of these frames walking)
        if mean is not None:
            monkeypatch.setenv("RT_TEST_BIN_MEAN", mean)
        if scene == "K":
            monkeypatch.setenv("RT_TEST_OCC_MEAN", "1e9")
        if cap is not None:
            monkeypatch.setenv("RT_TEST_BIN_CAP", str(cap))
        if capacity is not None:
            monkeypatch.setenv("RT_TEST_BIN_CAPACITY", str(capacity))
        if shrink:
            monkeypatch.setenv("RT_TEST_BIN_SHRINK", "1")
    return set_


@pytest.fixture(scope="module")
def oracle_scenes(oracle):
    ss = {k: oracle.Scene(*v) for k, v in SCENES.items()}
    yield ss
    for s in ss.values():
        s.close()


def _binned_frame(r):
    """A plain frame and its bin info: the frame must have used the bins."""
    r.render()
    bi = r.bin_info()
    assert bi["enabled"] == 1 and bi["reason"] == "on", bi
    assert bi["bin_size"] == BIN and bi["entries"] > 0 and bi["non_empty_bins"] > 0
    return bi


# ---- 1. frames ---------------------------------------------------------------

@pytest.mark.parametrize("scene,w,h,spp,cap,zoom", [
    # (U: about a third of its non-empty bins are over the cap of 64, so
    # binned and walking pixels mix in every U frame)
    ("U", 96, 64, 8, None, 1.0), ("U", 96, 64, 64, None, 1.0), ("U", 64, 48, 1, None, 1.0),
    ("U", 32, 24, 256, None, 1.0),   # the sorted path
    ("K", 96, 64, 8, None, 1.0),     # the cluster is four bins, all over the cap: they walk
    ("K", 96, 64, 8, 2, 1.0),
    ("K", 96, 64, 8, 2, 8.0),        # the cluster fills the frame: ten bins of one or two entries, 53 walk
    ("K", 96, 64, 8, None, 8.0),
    ("U", 100, 52, 64, None, 1.0),   # width and height no multiples of the bin
])
def test_frames_match_walk_and_oracle(gpu, hooks, oracle_scenes, scene, w, h, spp, cap, zoom):
    hooks(scene, cap)
    with _renderer(SCENES[scene], w, h, spp) as r:
        if zoom != 1.0:
            _zoomed(r, zoom)
        bi = _binned_frame(r)
        assert bi["bins"] == ((w + BIN - 1) // BIN) * ((h + BIN - 1) // BIN)
        assert bi["overflowed_bins"] > 0
        if zoom != 1.0 or scene == "U":
            assert bi["overflowed_bins"] < bi["non_empty_bins"]
        # plain (bins) == stats (walk) == oracle, and the stats frame's counters are the oracle's
        img, rad = _check_frames(r, oracle_scenes[scene], w, h, spp)
        assert r.bin_info()["reason"] == "kernel"   # the last frame was the stats frame: it walked
    with _renderer(SCENES[scene], w, h, spp, bins=False) as r:   # the A/B switch: identical bytes
        if zoom != 1.0:
            _zoomed(r, zoom)
        r.render()
        assert r.bin_info()["reason"] == "flag"
        assert np.array_equal(r.readback(), img) and np.array_equal(r.readback_radiance(), rad)


# ---- 2. the lists hold every sphere the oracle hits --------------------------

def _zoomed(r, zoom):
    _, K = r.camera()
    K = np.array(K, np.float32).copy()
    K[0, 0] *= zoom
    K[1, 1] *= zoom
    r.setIntrinsic(K)
    return K


def _unlisted(hits, hdr, idx, wide, w, n):
    """Of the oracle's primary hits, how many name a sphere that is neither in
    their pixel's bin list nor in the wide list.  A bin's entries run to the
    next bin's first entry (bins over the cap keep theirs)."""
    x, y, j, _ = hits
    nbx = (w + BIN - 1) // BIN
    off = np.concatenate([hdr[:, 0].astype(np.int64), [idx.shape[0]]])
    lens = np.diff(off)
    assert np.all(lens >= 0)
    listed = np.repeat(np.arange(hdr.shape[0], dtype=np.int64), lens) * n + idx.astype(np.int64)
    key = ((y // BIN) * nbx + x // BIN).astype(np.int64) * n + j
    ok = np.isin(key, listed) | np.isin(j, wide.astype(np.int64))
    return int((~ok).sum())


@pytest.mark.parametrize("scene,zoom", [("U", 1.0), ("K", 1.0), ("U", 6.0), ("K", 8.0)])
def test_oracle_primary_hits_are_listed(gpu, oracle, hooks, oracle_scenes, scene, zoom):
    """Every sample of a 96x64, 8 spp frame: the sphere the oracle's primary
    ray hits is in that pixel's exported list or in the wide list.  At the
    zoomed intrinsic (spheres several pixels across) the same check fails on
    lists built from radii x 0.9 (RT_TEST_BIN_SHRINK)."""
    w, h, spp = 96, 64, 8
    hooks(scene)
    sp, _ = SCENES[scene]
    with _renderer(SCENES[scene], w, h, spp) as r:
        K = _zoomed(r, zoom)
        pose, _ = r.camera()
        bi = _binned_frame(r)
        hdr, idx, wide = r.export_bins()
    assert hdr.shape[0] == bi["bins"] and idx.shape[0] == bi["entries"]
    cnt = hdr[:, 1]
    assert np.all((cnt == WALK) | (cnt <= 64))
    hits = primary_hits(oracle, oracle_scenes[scene], pose, K, w, h, spp)
    assert hits[0].shape[0] > (1000 if scene == "U" or zoom > 1.0 else 100)   # (K unzoomed: a few pixels)
    assert _unlisted(hits, hdr, idx, wide, w, sp.shape[0]) == 0
    if zoom > 1.0:
        hooks(scene, shrink=True)
        with _renderer(SCENES[scene], w, h, spp) as r:
            _zoomed(r, zoom)
            r.render()
            hdr9, idx9, wide9 = r.export_bins()
        assert _unlisted(hits, hdr9, idx9, wide9, w, sp.shape[0]) > 0, "the check cannot see an unsound list"


def test_lists_are_sorted_by_near_bound(gpu, hooks):
    """A bin's list is in ascending order of the spheres' near bound (restated
    in f64 here: distance - r'' with the product's slack), ties by index."""
    hooks("U")
    sp, _ = SCENES["U"]
    with _renderer(SCENES["U"]) as r:
        pose, _ = r.camera()
        _binned_frame(r)
        hdr, idx, _ = r.export_bins()
    o = np.asarray(pose, np.float32).reshape(4, 4)[3, :3].astype(np.float64)
    dist = np.linalg.norm(sp[:, :3].astype(np.float64) - o, axis=1)
    near = ((dist - (sp[:, 3].astype(np.float64) * (1 + 1e-6) + dist / 131072.0)) * (1 - 2.0 ** -20)).astype(np.float32)
    seen = 0
    for off, cnt in hdr:
        if cnt == WALK or cnt < 2:
            continue
        li = idx[off:off + cnt].astype(np.int64)
        k = near[li]
        assert np.all((k[:-1] < k[1:]) | ((k[:-1] == k[1:]) & (li[:-1] < li[1:])))
        assert np.unique(li).shape[0] == li.shape[0]
        seen += 1
    assert seen >= 20


# ---- 3. cameras --------------------------------------------------------------

def test_camera_inside_the_root_box(gpu, hooks, oracle_scenes):
    """S: a few spheres lie across the camera plane and go to the wide list,
    which every pixel tests.  U from the same place has more of them than the
    wide list holds: the frame walks and says so."""
    hooks()
    pose = translation_pose(0.64, 0.64, 1.0)
    with _renderer(SCENES["S"], pose=pose) as r:
        bi = _binned_frame(r)
        assert 1 <= bi["wide"] <= WIDE_CAP
        _check_frames(r, oracle_scenes["S"], 96, 64, 8)
    with _renderer(SCENES["U"], pose=pose) as r:
        r.render()
        bi = r.bin_info()
        assert bi["enabled"] == 0 and bi["reason"] == "wide" and bi["wide"] > WIDE_CAP
        _check_frames(r, oracle_scenes["U"], 96, 64, 8)


def test_camera_inside_a_sphere(gpu, hooks, oracle_scenes):
    hooks()
    sp, _ = SCENES["S"]
    pose = np.array(scene_pose(), np.float32).reshape(4, 4).copy()
    pose[3, :3] = sp[11, :3] + np.float32(0.3) * sp[11, 3]
    with _renderer(SCENES["S"], pose=pose) as r:
        bi = _binned_frame(r)
        assert bi["wide"] >= 1
        _check_frames(r, oracle_scenes["S"], 96, 64, 8)


def test_sphere_across_the_camera_plane(gpu, hooks, oracle_scenes):
    """The camera beside S's topmost sphere, at the depth of its centre, looking
    down at the rest: the sphere lies across the camera plane and fills one
    side of the image."""
    hooks()
    sp, _ = SCENES["S"]
    top = int(np.argmax(sp[:, 2]))
    c, rad = sp[top, :3], sp[top, 3]
    pose = translation_pose(float(c[0] + 1.5 * rad), float(c[1]), float(c[2]))
    with _renderer(SCENES["S"], pose=pose) as r:
        bi = _binned_frame(r)
        assert bi["wide"] >= 1
        img, _ = _check_frames(r, oracle_scenes["S"], 96, 64, 8)


@pytest.mark.parametrize("pos", [(0.1, 0.9, 2.0), (1.9, 1.6, 1.9), (-0.6, 0.2, 1.7)])
def test_yaw_pitch_poses(gpu, hooks, oracle_scenes, pos):
    hooks()
    with _renderer(SCENES["U"], pose=look_at_pose(pos)) as r:
        _binned_frame(r)
        _check_frames(r, oracle_scenes["U"], 96, 64, 8)


@pytest.mark.parametrize("scene,z", [("U", 3.0), ("U", 300.0), ("U", 3000.0), ("K", 300.0)])
def test_far_camera(gpu, hooks, oracle_scenes, scene, z):
    """test_gpu_occluders' far cameras with its zoom: the near bound and the
    rectangles carry a term in the camera's distance."""
    hooks(scene)
    w, h, spp = 96, 64, 8
    pose = np.array(scene_pose(), np.float32).reshape(4, 4).copy()
    pose[3, 2] = z
    with _renderer(SCENES[scene], w, h, spp, pose=pose) as r:
        _zoomed(r, (z - 0.64) / (2.2 - 0.64) * (8.0 if scene == "K" else 1.0))
        _binned_frame(r)
        _check_frames(r, oracle_scenes[scene], w, h, spp)


def test_pose_that_is_no_rotation_walks(gpu, hooks, oracle_scenes):
    hooks()
    pose = np.array(scene_pose(), np.float32).reshape(4, 4).copy()
    pose[:3, :3] *= np.float32(1.25)
    with _renderer(SCENES["U"], pose=pose) as r:
        r.render()
        assert r.bin_info()["reason"] == "camera"
        _check_frames(r, oracle_scenes["U"], 96, 64, 8)


def test_dense_frame_walks(gpu, oracle_scenes, hooks):
    """The product's rule: U on 32x24 pixels is hundreds of spheres a bin, so
    the builder stops after counting and the frame walks."""
    hooks(mean=None)
    with _renderer(SCENES["U"], 32, 24, 8) as r:
        r.render()
        bi = r.bin_info()
        assert bi["enabled"] == 0 and bi["reason"] == "dense" and bi["entries"] > 48 * bi["non_empty_bins"]
        _check_frames(r, oracle_scenes["U"], 32, 24, 8)


def test_dense_skip_cadence(gpu, oracle_scenes, hooks):
    """After a probe the device rule found dense, the next kBinDenseSkip = 15
    plain frames build no bins, then one probes again: "once in 16 frames"
    (csrc/rt_bins_math.h).  bin_info() after every frame synchronises, so each
    observation is deterministic.  A stats frame in between does not count, a
    pose change in the middle of the skip renders the new pose, and set_scene
    starts over; every frame's bytes are the oracle's."""
    hooks(mean=None)
    w, h, spp, skip = 32, 24, 8, 15
    moved = look_at_pose((0.1, 0.9, 2.0))
    with _renderer(SCENES["U"], w, h, spp) as r:
        _, K = r.camera()
        refs = {k: oracle_scenes["U"].render(w, h, p, K, spp=spp) for k, p in
                (("scene", scene_pose()), ("moved", moved))}

        def frame(pose="scene", stats=False):
            st = r.render(stats=stats)
            bi = r.bin_info()
            ref8, ref32, cnt = refs[pose]
            assert np.array_equal(r.readback(), ref8) and np.array_equal(r.readback_radiance(), ref32)
            if stats:
                assert (st.primary_rays, st.shadow_rays) == (int(cnt[0]), int(cnt[1]))
            return bi

        def probe(pose="scene"):
            bi = frame(pose)
            assert bi["enabled"] == 0 and bi["reason"] == "dense", bi
            assert bi["bins"] == 4 * 3 and bi["entries"] > 48 * bi["non_empty_bins"] > 0, bi

        def skipped(pose="scene"):
            bi = frame(pose)
            assert bi["enabled"] == 0 and bi["reason"] == "dense", bi
            assert bi["bins"] == 0 and bi["entries"] == 0, bi

        probe()
        for k in range(skip):
            if k == 4:      # a stats frame walks and does not advance the count
                assert frame(stats=True)["reason"] == "kernel"
            if k == 7:
                r.setPosition(moved)
            skipped("moved" if k >= 7 else "scene")
        probe("moved")
        skipped("moved")
        skipped("moved")
        r.setPosition(scene_pose())
        r.set_scene(*SCENES["U"])     # a new scene generation: the count starts over
        probe()
        for k in range(skip):
            skipped()
        probe()


# ---- 4. a moving camera ------------------------------------------------------

def test_moving_camera(gpu, hooks, oracle_scenes):
    """Six frames, a new pose each, every one the oracle's: bins left over
    from an earlier pose would show."""
    hooks()
    w, h, spp = 96, 64, 8
    with _renderer(SCENES["U"], w, h, spp) as r:
        _, K = r.camera()
        for k in range(6):
            a = 0.5 * k
            pose = look_at_pose((0.64 + 1.6 * np.sin(a), 0.64 + 0.2 * k, 0.64 + 1.6 * np.cos(a)))
            r.setPosition(pose)
            bi = _binned_frame(r)
            ref8, ref32, _ = oracle_scenes["U"].render(w, h, pose, K, spp=spp)
            assert np.array_equal(r.readback(), ref8), k
            assert np.array_equal(r.readback_radiance(), ref32), k
            assert bi["entries"] > 0


# ---- 5. capacity -------------------------------------------------------------

def test_entry_buffer_overflow_walks_then_grows(gpu, hooks, oracle_scenes):
    """A 16-entry buffer: the first frame's lists do not fit, so it walks (the
    device flag) and says why; the next frame has the buffer it asked for."""
    hooks(capacity=16)
    w, h, spp = 96, 64, 8
    with _renderer(SCENES["U"], w, h, spp) as r:
        pose, K = r.camera()
        ref8, ref32, _ = oracle_scenes["U"].render(w, h, pose, K, spp=spp)
        r.render()
        bi = r.bin_info()
        assert bi["enabled"] == 0 and bi["reason"] == "capacity"
        assert bi["capacity"] == 16 < bi["entries"]
        assert np.array_equal(r.readback(), ref8) and np.array_equal(r.readback_radiance(), ref32)
        with pytest.raises(RtError):
            r.export_bins()
        need = bi["entries"]
        bi = _binned_frame(r)
        assert bi["capacity"] >= need == bi["entries"]
        assert bi["bin_build_ms"] > 0.0     # timed from the first bin_info call on
        assert np.array_equal(r.readback(), ref8) and np.array_equal(r.readback_radiance(), ref32)


# ---- 6. other paths and switches ---------------------------------------------

def test_tiles_match_whole_frame(gpu, hooks):
    import torch
    hooks()
    w, h, ts = 96, 64, 64
    ids = np.arange(((w + ts - 1) // ts) * ((h + ts - 1) // ts), dtype=np.uint32)
    with _renderer(SCENES["U"]) as full, _renderer(SCENES["U"]) as tiled:
        packed = torch.zeros(len(ids) * ts * ts * 4, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        _binned_frame(full)
        tiled.render_tiles(ids, ts, packed.data_ptr())
        bi = tiled.bin_info()
        assert bi["enabled"] == 1 and bi["bins"] == 12 * 8    # the grid is the image's, not the tiles'
        tiled.unpack_tiles(packed.data_ptr(), ids, ts)
        assert np.array_equal(tiled.readback(), full.readback())


def test_progressive_second_frame(gpu, hooks, oracle_scenes):
    hooks()
    w, h, spp = 96, 64, 8
    acc = np.zeros((h, w, 4), np.float32)
    with _renderer(SCENES["U"], progressive=True) as r:
        pose, K = r.camera()
        for k in range(2):
            _binned_frame(r)
            img, rad, _ = oracle_scenes["U"].render(w, h, pose, K, spp=spp, frame=k, accum=acc)
            assert np.array_equal(r.readback(), img), k
            assert np.array_equal(r.readback_radiance(), rad), k


def test_bins_without_occluder_lists(gpu, hooks, oracle_scenes):
    hooks()
    with _renderer(SCENES["U"], occluders=False) as r:
        _binned_frame(r)
        assert r.scene_info()["occluder_lists_on"] == 0
        _check_frames(r, oracle_scenes["U"], 96, 64, 8)
