"""Tile words of the screen-space bins: the builder
leaves one 64-bit word per wave tile of every listed bin, bit k: the bin's
entry k overlaps the tile, and the frame kernels visit the set bits only.

The exported words against a numpy model built from the exported lists and the
CPU rectangles, for every wave-tile shape; frames byte for byte against the
same renderer walking (RT_FLAG_NO_BINS): plain, sorted rounds, progressive
pairs, packed tiles with edge tiles, a wide sphere; a bin of exactly the cap's
entries, one more, and a single entry.  Frames of 70x44 pixels: no side a
multiple of the bin.
"""
import numpy as np
import pytest

import bins_native
from bin_tiles_model import BIN, WALK, frame_tile_words
from raytracingstudy_amd.camera import translation_pose
from test_gpu_bins import SCENES
from test_gpu_occluders import _renderer

pytestmark = pytest.mark.gpu

W, H = 70, 44
SPPS = [64, 32, 24, 16, 8, 4, 2, 1]
SHAPE = {64: (1, 1), 32: (2, 1), 24: (2, 1), 16: (2, 2), 8: (4, 2), 4: (4, 4), 2: (8, 4), 1: (8, 8)}
ZOOM = 3.0      # S's spheres a few pixels across: rectangles that cut through bins and tiles


@pytest.fixture
def hooks(monkeypatch):
    def set_(cap=None):
        monkeypatch.setenv("RT_TEST_BIN_MIN_SAMPLES", "0")
        monkeypatch.setenv("RT_TEST_BIN_MEAN", "1000000")
        if cap is not None:
            monkeypatch.setenv("RT_TEST_BIN_CAP", str(cap))
    return set_


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    return bins_native.build_dump(tmp_path_factory.mktemp("bin_tiles_gpu"))


def _zoom(r, zoom=ZOOM):
    _, K = r.camera()
    K = np.array(K, np.float32).copy()
    K[0, 0] *= zoom
    K[1, 1] *= zoom
    r.setIntrinsic(K)


def _binned(r, frames=1):
    for _ in range(frames):
        r.render()
    bi = r.bin_info()
    assert bi["enabled"] == 1 and bi["reason"] == "on", bi
    return bi


def _same_as_walking(scene, spp, pose=None, zoom=ZOOM, frames=1, **kw):
    """The frame(s) with bins and with RT_FLAG_NO_BINS: identical bytes.
    Returns the binned renderer's last bin info."""
    out = []
    for bins in (True, False):
        with _renderer(scene, W, H, spp, pose=pose, bins=bins, **kw) as r:
            if zoom != 1.0:
                _zoom(r, zoom)
            if bins:
                bi = _binned(r, frames)
            else:
                for _ in range(frames):
                    r.render()
                assert r.bin_info()["reason"] == "flag"
            out.append((r.readback(), r.readback_radiance()))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    return bi


# ---- 1. the words ------------------------------------------------------------

@pytest.mark.parametrize("spp", SPPS)
def test_words_match_the_model(gpu, hooks, dump, spp):
    hooks()
    sp, _ = SCENES["S"]
    with _renderer(SCENES["S"], W, H, spp) as r:
        _zoom(r)
        pose, K = r.camera()
        bi = _binned(r)
        hdr, idx, _ = r.export_bins()
        (tw, th), words = r.export_bin_tiles()
    assert (tw, th) == SHAPE[spp]
    assert words.shape == (bi["bins"], 64 // (tw * th)) and bi["bins"] == 9 * 6
    cls, rect_px, _ = bins_native.rects(dump, sp, pose, K, W, H)
    listed = (hdr[:, 1] != WALK) & (hdr[:, 1] > 0)
    assert listed.sum() >= 20 and np.all(cls[idx] == bins_native.BINNED)
    want = frame_tile_words(hdr, idx, rect_px, W, tw, th)
    assert np.array_equal(words, want)
    # the model is no trivial one: words differ between the tiles of a bin
    # (but for the one 8x8 tile), and some entry misses some tile of its bin
    cnt = hdr[listed, 1].astype(np.uint64)
    full = (np.uint64(1) << cnt) - np.uint64(1)     # (no listed bin of S holds 64)
    assert np.all(cnt < 64)
    if tw * th < 64:
        assert np.any(words[listed] != full[:, None])
        assert np.any(words[listed].min(axis=1) != words[listed].max(axis=1))
    else:
        assert np.array_equal(words[listed][:, 0], full)


# ---- 2. frames ---------------------------------------------------------------

@pytest.mark.parametrize("spp", SPPS + [130, 128])     # 130, 128: sorted rounds
def test_frames_match_walking(gpu, hooks, spp):
    hooks()
    bi = _same_as_walking(SCENES["S"], spp)
    assert bi["non_empty_bins"] >= 20


@pytest.mark.parametrize("spp", [64, 8, 128])
def test_progressive_pairs(gpu, hooks, spp):
    hooks()
    _same_as_walking(SCENES["S"], spp, frames=2, progressive=True)


@pytest.mark.parametrize("spp", [64, 8, 1])
def test_packed_tiles_with_edge_tiles(gpu, hooks, spp):
    """64-pixel tiles of a 70x44 frame: the second tile holds six columns of
    the image, the rest of its wave tiles lie off it."""
    import torch
    hooks()
    ts = 64
    ids = np.arange(2, dtype=np.uint32)
    got = []
    for bins in (True, False):
        with _renderer(SCENES["S"], W, H, spp, bins=bins) as r:
            _zoom(r)
            packed = torch.zeros(len(ids) * ts * ts * 4, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            r.render_tiles(ids, ts, packed.data_ptr())
            bi = r.bin_info()
            assert bi["enabled"] == (1 if bins else 0) and (not bins or bi["bins"] == 9 * 6)
            r.unpack_tiles(packed.data_ptr(), ids, ts)
            got.append((packed.cpu().numpy().copy(), r.readback()))
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])


@pytest.mark.parametrize("spp", [64, 8])
def test_wide_sphere(gpu, hooks, spp):
    """The camera inside S's root box: a few spheres lie across the camera
    plane, and every tile tests them after its own bits."""
    hooks()
    bi = _same_as_walking(SCENES["S"], spp, pose=translation_pose(0.64, 0.64, 1.0), zoom=1.0)
    assert bi["wide"] >= 1


# ---- 3. a bin at the cap, over it, and of one entry ----------------------------

def _stack_scene(r, n, lone=True):
    """n spheres behind one another along the ray through pixel (36, 20), three
    pixels across: all in bin (4, 2) and nowhere else; and one sphere alone in
    bin (1, 4).  Built for r's camera."""
    pose, K = r.camera()
    P = np.asarray(pose, np.float64).reshape(4, 4)
    Kf = np.asarray(K, np.float64).reshape(-1)
    o, Rm = P[3, :3], P[:3, :3]

    def at(u, v, z, px):
        cam = np.array([(u - Kf[2]) / Kf[0] * z, (v - Kf[5]) / Kf[4] * z, z])
        return np.concatenate([o + cam @ Rm, [px * z / Kf[0]]])
    sp = [at(36.0, 20.0, 1.0 + 0.02 * k, 1.5) for k in range(n)]
    if lone:
        sp.append(at(12.0, 36.0, 1.5, 1.5))
    sp = np.array(sp, np.float32)
    al = np.full(sp.shape[0], 0xFF8040C0, np.uint32)
    return sp, al


@pytest.mark.parametrize("n,cap,spp", [(64, None, 64), (65, None, 64), (64, None, 4), (5, 5, 8), (6, 5, 8),
                                       (5, 5, 64)])
def test_bin_at_the_cap_and_over_it(gpu, hooks, dump, n, cap, spp):
    hooks(cap)
    limit = 64 if cap is None else cap
    with _renderer(SCENES["S"], W, H, spp) as r:
        scene = _stack_scene(r, n)
        r.set_scene(*scene)
        pose, K = r.camera()
        bi = _binned(r)
        hdr, idx, _ = r.export_bins()
        (tw, th), words = r.export_bin_tiles()
    cls, rect_px, _ = bins_native.rects(dump, scene[0], pose, K, W, H)
    assert np.all(cls == bins_native.BINNED)
    the_bin, lone_bin = 2 * 9 + 4, 4 * 9 + 1
    assert np.all(rect_px[:n, [0, 2]] // BIN == 4) and np.all(rect_px[:n, [1, 3]] // BIN == 2)
    assert np.count_nonzero(hdr[:, 1]) == 2
    if n <= limit:
        assert hdr[the_bin, 1] == n and bi["overflowed_bins"] == 0 and bi["longest"] == n
        assert int(np.bitwise_or.reduce(words[the_bin])) == (1 << n) - 1       # all n bits are used
        if th < 4:      # (four pixels of rows: the stack's rows 2 .. 5 reach every 4x4 tile)
            assert words[the_bin].min() == 0                                 # and some tile is empty
    else:
        assert hdr[the_bin, 1] == WALK and bi["overflowed_bins"] == 1
        assert not words[the_bin].any()
    assert hdr[lone_bin, 1] == 1 and words[lone_bin].max() == 1
    assert np.array_equal(words, frame_tile_words(hdr, idx, rect_px, W, tw, th))
    _same_as_walking(scene, spp, zoom=1.0)
