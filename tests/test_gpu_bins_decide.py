"""The words a frame's bin build reports (csrc/screen_bins.hip bins_decide,
DESIGN.md 5.1 round 19): the decision is taken by many blocks, a bin a thread,
whose partial results meet in device words; the block that arrives last writes
the frame's words.

bin_info() after a frame against a numpy model of the build made from the CPU
rectangles (tests/native/bins_math_dump.cpp) and checked against the exported
headers: total entries, non-empty bins, the longest list, bins over the cap,
the wide count and the flag.  One bin, 54 bins, 375 bins (two blocks, the
second partly filled); a lowered cap, each of the three flags; frames queued
back to back, whose builds must each re-arm the arrival counter.
"""
import numpy as np
import pytest

import bins_native
from raytracingstudy_amd.camera import display_pose, scene_pose, translation_pose
from test_gpu_bins import SCENES
from test_gpu_occluders import _renderer

pytestmark = pytest.mark.gpu

BIN, WALK, WIDE_CAP = 8, 0xFFFFFFFF, 32


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    return bins_native.build_dump(tmp_path_factory.mktemp("bins_decide"))


@pytest.fixture
def hooks(monkeypatch):
    def set_(cap=None, mean="1000000", capacity=None):
        monkeypatch.setenv("RT_TEST_BIN_MIN_SAMPLES", "0")
        monkeypatch.setenv("RT_TEST_BIN_MEAN", mean)
        if cap is not None:
            monkeypatch.setenv("RT_TEST_BIN_CAP", str(cap))
        if capacity is not None:
            monkeypatch.setenv("RT_TEST_BIN_CAPACITY", str(capacity))
    return set_


def _zoom(r, zoom):
    _, K = r.camera()
    K = np.array(K, np.float32).copy()
    K[0, 0] *= zoom
    K[1, 1] *= zoom
    r.setIntrinsic(K)


def _model(dump, sp, pose, K, w, h, cap, mean, capacity):
    """The build's words from the CPU rectangles: per-bin counts, then what
    bins_decide derives from them."""
    cls, rect, _ = bins_native.rects(dump, sp, pose, K, w, h)
    nbx, nby = (w + BIN - 1) // BIN, (h + BIN - 1) // BIN
    cnt = np.zeros((nby, nbx), np.int64)
    for x0, y0, x1, y1 in rect[cls == bins_native.BINNED]:
        cnt[y0 // BIN:y1 // BIN + 1, x0 // BIN:x1 // BIN + 1] += 1
    cnt = cnt.reshape(-1)
    wide = int((cls == bins_native.WIDE).sum())
    total, ne = int(cnt.sum()), int(np.count_nonzero(cnt))
    reason = ("capacity" if total > capacity else "wide" if wide > WIDE_CAP
              else "dense" if total > mean * ne else "on")
    words = {"bins": nbx * nby, "entries": total, "non_empty_bins": ne, "longest": int(cnt.max()),
             "overflowed_bins": int((cnt > cap).sum()), "wide": wide, "reason": reason,
             "enabled": 1 if reason == "on" else 0}
    return words, cnt


def _check(r, dump, sp, w, h, cap=64, mean=1000000):
    """The last frame's words against the model of its camera; the headers too
    where the frame kept its lists."""
    pose, K = r.camera()
    bi = r.bin_info()
    want, cnt = _model(dump, sp, pose, K, w, h, cap, mean, bi["capacity"])
    assert {k: bi[k] for k in want} == want
    if bi["enabled"]:
        hdr, _, wide = r.export_bins()
        assert np.array_equal(hdr[:, 0], np.concatenate([[0], np.cumsum(cnt)[:-1]]))
        assert np.array_equal(hdr[:, 1], np.where(cnt > cap, WALK, cnt))
        assert wide.shape[0] == want["wide"]
    return bi


@pytest.mark.parametrize("w,h,blocks", [(8, 8, 1), (70, 44, 1), (200, 120, 2)])
def test_words_match_the_model(gpu, hooks, dump, w, h, blocks):
    hooks()
    sp, _ = SCENES["U"]
    with _renderer(SCENES["U"], w, h, 4) as r:
        r.render()
        bi = _check(r, dump, sp, w, h)
    assert (bi["bins"] + 255) // 256 == blocks and bi["reason"] == "on"
    assert bi["bins"] == 1 or bi["bins"] % 256 != 0
    assert bi["entries"] > bi["non_empty_bins"] > 0 and bi["longest"] > 1


def test_bins_over_a_lowered_cap(gpu, hooks, dump):
    hooks(cap=2)
    with _renderer(SCENES["S"], 200, 120, 4) as r:
        r.render()
        bi = _check(r, dump, SCENES["S"][0], 200, 120, cap=2)
    assert 0 < bi["overflowed_bins"] < bi["non_empty_bins"] < bi["bins"] and bi["reason"] == "on"


def test_wide_spheres_are_counted(gpu, hooks, dump):
    hooks()
    with _renderer(SCENES["S"], 70, 44, 4, pose=translation_pose(0.64, 0.64, 1.0)) as r:
        r.render()
        bi = _check(r, dump, SCENES["S"][0], 70, 44)
    assert 1 <= bi["wide"] <= WIDE_CAP and bi["reason"] == "on"


def test_the_dense_flag(gpu, hooks, dump):
    hooks(mean="2")
    with _renderer(SCENES["U"], 200, 120, 4) as r:
        r.render()
        bi = _check(r, dump, SCENES["U"][0], 200, 120, mean=2)
    assert bi["reason"] == "dense" and bi["entries"] > 2 * bi["non_empty_bins"]


def test_the_capacity_flag(gpu, hooks, dump):
    """A first buffer of 16 entries: the first frame reports what it needs and
    walks, the next one has the room."""
    hooks(capacity=16)
    sp, _ = SCENES["S"]
    with _renderer(SCENES["S"], 200, 120, 4) as r:
        _zoom(r, 3.0)
        r.render()
        bi = _check(r, dump, sp, 200, 120)
        assert bi["reason"] == "capacity" and bi["capacity"] == 16 < bi["entries"]
        r.render()
        bi2 = _check(r, dump, sp, 200, 120)
        assert bi2["reason"] == "on" and bi2["capacity"] >= bi["entries"] == bi2["entries"]


def test_frames_back_to_back(gpu, hooks, dump):
    """Three, two and one frames of different cameras queued without a wait:
    the last one's words are its own camera's.  A build that left the arrival
    counter as the build before it did would never write them."""
    hooks()
    sp, _ = SCENES["U"]
    poses = [scene_pose(), display_pose((0.6, 0.7, 2.3), 5.0, -3.0), display_pose((0.3, 0.5, 2.0), -8.0, 4.0)]
    seen = []
    with _renderer(SCENES["U"], 200, 120, 4) as r:
        for k in (3, 2, 1):
            for p in poses[:k]:
                r.setPosition(p)
                r.render()
            bi = _check(r, dump, sp, 200, 120)
            seen.append((bi["entries"], bi["non_empty_bins"], bi["longest"]))
    assert len(set(seen)) == 3      # the cameras differ in every word compared
