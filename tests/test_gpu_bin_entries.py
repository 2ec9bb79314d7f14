"""The binned primary test (bin_entry) and the occluder loops of the pair and
the one-pixel path: an entry's accept and tie rule,
the camera origin in an entry's test, and each lane's way through its occluder
list.  Round 27 rewrote the pair path's occluder loop; its other two steps
(the accept rule as selects, entries that hold o - c) were measured and not
kept, and their cases stay here for whoever tries them again.

Frames of 71x45 and 70x44 at 64 spp (tests/test_gpu_pixel_pairs.py's sizes: an
odd and an even width, neither a multiple of 8), each rendered with pairs on,
with RT_FLAG_NO_PAIRS (the one-pixel path) and with RT_FLAG_NO_BINS (every
primary ray walks): bytes and radiance bits against the oracle, hence against
each other.
"""
import numpy as np
import pytest

import raytracingstudy_amd as rt
from raytracingstudy_amd.camera import translation_pose

from test_gpu_frame_chain import _E1, _L, _column_scene, _zoom
from test_gpu_occluders import _renderer

pytestmark = pytest.mark.gpu

WALK = 0xFFFFFFFF
PAIR, BINS, OCC, WAVEQ, TILES = 128, 64, 32, 8, 1
SIZES = [(71, 45), (70, 44)]
POSE = translation_pose(0.64, 0.64, 1.25)
FAR_POSE = translation_pose(640.3, -480.6, 1000.2)
FAR_SCALE = 1499.7
BIN_CAP = 5
SKY_R = np.float32(200.0) / np.float32(255.0)      # a sample that misses: red is 200/255, so is a mean of such

# the pixels the entry scene's spheres sit on
ROW, TIE, A_ONLY, B_ONLY = 10, 40, 20, 25
CORNER = (28.0, 36.0, 1.3)             # centre (a pixel corner) and radius in pixels


@pytest.fixture
def hooks(monkeypatch):
    def set_(bin_cap=BIN_CAP, occ_cap=None):
        monkeypatch.setenv("RT_TEST_BIN_MIN_SAMPLES", "0")
        monkeypatch.setenv("RT_TEST_BIN_MEAN", "1000000")
        if bin_cap is not None:
            monkeypatch.setenv("RT_TEST_BIN_CAP", str(bin_cap))
        if occ_cap is not None:
            monkeypatch.setenv("RT_TEST_OCC_CAP", str(occ_cap))
    return set_


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _placer(w, h, pose, scale=1.0):
    """at(u, v, z, px): the sphere whose centre the w x h camera at `pose`
    sees at image point (u, v) (pixel x covers [x, x + 1)), `z * scale` deep
    and `px` pixels in radius; off(c, r): one at camera offset c."""
    P = np.asarray(pose, np.float64).reshape(4, 4)
    Kf = np.asarray(rt.resize_intrinsic(w, h), np.float64).reshape(-1)
    o, Rm = P[3, :3], P[:3, :3]

    def at(u, v, z, px):
        z = z * scale
        cam = np.array([(u - Kf[2]) / Kf[0] * z, (v - Kf[5]) / Kf[4] * z, z])
        return np.concatenate([o + cam @ Rm, [px * z / Kf[0]]])

    def off(c, r):
        return np.concatenate([o + scale * np.asarray(c, np.float64) @ Rm, [scale * r]])
    return at, off


def _albedo(n):
    return (0xFF000000 | (np.arange(n) * 0x123457 + 0x405060) & 0xFFFFFF).astype(np.uint32)


def _entry_scene(w, h, pose=POSE, scale=1.0, inside=False, swap_tie=False):
    """Spheres placed by pixel: two equal ones over the pair at TIE (a tie in t
    in every lane, decided by the index; swap_tie lists them, and their
    albedos, in the other order); one within pixel A of a pair, one within B
    of another; one of 1.3 pixels about a pixel corner (its rectangle holds
    corner pixels no sample of which meets it, and edge pixels only some
    samples of which do); a bin of exactly BIN_CAP; a larger one (lit on one
    side: shadows wanted in some lanes only); one over the last columns; one
    across the camera plane (the wide list).  inside: one around the camera
    (wide too; the near root is behind every ray's origin, the far one counts)."""
    at, off = _placer(w, h, pose, scale)
    v = ROW + 0.5
    tie = [at(TIE + 1.0, v, 0.6, 0.9), at(TIE + 1.0, v, 0.6, 0.9)]
    sp = tie + [at(A_ONLY + 0.5, v, 0.6, 0.4), at(B_ONLY + 0.5, v, 0.6, 0.4), at(CORNER[0], CORNER[1], 0.6, CORNER[2])]
    sp += [at(12.0, 20.0, 0.5 + 0.01 * k, 1.5) for k in range(BIN_CAP)]
    sp += [at(52.0, 20.0, 0.6, 2.5), at(70.2, 30.5, 0.65, 1.2), off([0.45, 0.0, 0.04], 0.06)]
    if inside:
        sp += [off([0.01, 0.0, 0.0], 0.62)]
    sp = np.array(sp, np.float32)
    al = _albedo(sp.shape[0])
    if swap_tie:
        al[[0, 1]] = al[[1, 0]]
    return sp, al


def _three_ways(scene, w, h, pose, want, spp=64, zoom=None, **kw):
    """The frame with pairs, by the one-pixel path and with every primary ray
    walking, each against `want` = the oracle's (rgba8, radiance); the pair
    render's renderer state is returned by `probe(r)` if given."""
    probe = kw.pop("probe", None)
    seen = None
    for pairs, bins in ((True, True), (False, True), (True, False)):
        with _renderer(scene, w, h, spp, pose=pose, pairs=pairs, bins=bins, **kw) as r:
            if zoom is not None:
                _zoom(r, zoom)
            r.render()
            got = r.readback(), r.readback_radiance()
            assert (r.bin_info()["reason"] == "on") == bins, (pairs, bins)
            if bins and probe is not None and seen is None:
                seen = probe(r)
        assert np.array_equal(got[0], want[0]), (pairs, bins)
        assert np.array_equal(_bits(got[1]), _bits(want[1])), (pairs, bins)
    return seen


@pytest.fixture(scope="module")
def refs(oracle):
    """ref(key, scene, w, h, pose, K=None, **oracle arguments): the oracle's
    (rgba8, radiance), each computed once."""
    cache = {}

    def ref(key, scene, w, h, pose, K=None, spp=64, **kw):
        key = (key, w, h, spp, np.asarray(pose).tobytes(), tuple(sorted(kw.items())))
        if key not in cache:
            s = oracle.Scene(*scene)
            cache[key] = s.render(w, h, pose, rt.resize_intrinsic(w, h) if K is None else K, spp=spp, **kw)[:2]
            s.close()
        return cache[key]
    return ref


# ---------------------------------------------------------------------------
# accept and tie
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("inside", [False, True], ids=["outside", "inside"])
@pytest.mark.parametrize("swap_tie", [False, True], ids=["tie-01", "tie-10"])
@pytest.mark.parametrize("w,h", SIZES)
def test_accept_and_tie(gpu, hooks, refs, w, h, swap_tie, inside):
    hooks()
    scene = _entry_scene(w, h, inside=inside, swap_tie=swap_tie)
    want = refs(("entry", inside, swap_tie), scene, w, h, POSE)
    nbx = (w + 7) // 8

    def probe(r):
        assert r.last_instance() == WAVEQ | OCC | BINS | PAIR
        return r.export_bins(), r.export_bin_tiles(), r.bin_info()
    (hdr, idx, wide), ((tw, th), words), bi = _three_ways(scene, w, h, POSE, want, probe=probe)
    n = scene[0].shape[0]
    assert (tw, th) == (1, 1) and bi["wide"] == (2 if inside else 1)
    assert sorted(wide.tolist()) == list(range(n - bi["wide"], n))             # the wide list is tested
    assert hdr[:, 1].reshape(-1, nbx)[2, 1] == BIN_CAP                          # a bin at the cap, listed

    def word(x, y):
        return int(words[(y // 8) * nbx + x // 8, (y % 8) * 8 + x % 8])
    rad = want[1]
    # the tie: both entries in both pixels' words, the lower index's albedo wins
    assert bin(word(TIE, ROW)).count("1") == 2 and word(TIE, ROW) == word(TIE + 1, ROW)
    other = refs(("entry", inside, not swap_tie), _entry_scene(w, h, inside=inside, swap_tie=not swap_tie), w, h, POSE)
    assert not np.array_equal(want[0][ROW, TIE], other[0][ROW, TIE])
    if not inside:
        # an entry no lane meets (a corner pixel of the rectangle: every sample is sky) ...
        x0, y0 = int(CORNER[0]) - 2, int(CORNER[1]) - 2
        assert word(x0, y0) and rad[y0, x0, 0] == SKY_R
        # ... and one only some lanes meet (an edge pixel; the centre pixels are covered)
        assert word(x0, y0 + 2) and rad[y0 + 2, x0, 0] != SKY_R
        assert rad[y0 + 2, x0 + 1, 0] != SKY_R
        # a pair with an entry in A's word only, and one in B's only
        assert word(A_ONLY, ROW) and not word(A_ONLY + 1, ROW) and A_ONLY % 2 == 0
        assert word(B_ONLY, ROW) and not word(B_ONLY - 1, ROW) and B_ONLY % 2 == 1
    else:
        # every ray ends on the sphere around the camera or before it: no sky
        assert not (rad[..., 0] == SKY_R).any()


# ---------------------------------------------------------------------------
# camera-relative entries
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", SIZES)
def test_large_origin(gpu, hooks, refs, w, h):
    """The scene some 1500 times as large, about a camera some 1300 from the world's
    origin and 900 from the spheres, which lie near that origin (finer f32
    steps than the difference's): o - c is a rounded f32 difference for most
    spheres, and the binned test must round it as isect does."""
    hooks()
    scene = _entry_scene(w, h, pose=FAR_POSE, scale=FAR_SCALE)
    o = np.asarray(FAR_POSE, np.float32)[3, :3]
    c = scene[0][:, :3]
    inexact = (o[None] - c).astype(np.float64) != o[None].astype(np.float64) - c.astype(np.float64)
    assert inexact.any(axis=1).sum() > c.shape[0] // 2
    want = refs("far", scene, w, h, FAR_POSE)
    assert np.unique(want[0].reshape(-1, 4), axis=0).shape[0] > 8
    _three_ways(scene, w, h, FAR_POSE, want)


@pytest.mark.parametrize("pairs", [True, False], ids=["pairs", "one-pixel"])
def test_two_origins_back_to_back(gpu, oracle, hooks, pairs):
    """Two frames queued on one stream without a wait, from different origins:
    each frame's entries are its own origin's."""
    import torch
    hooks()
    w, h = SIZES[0]
    scene = _entry_scene(w, h)
    poses = [POSE, translation_pose(0.67, 0.62, 1.21)]
    bufs = [torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda") for _ in poses]
    torch.cuda.synchronize()
    with _renderer(scene, w, h, 64, pose=POSE, pairs=pairs) as r:
        for p, b in zip(poses, bufs):
            r.setPosition(p)
            r.render(dev_ptr=b.data_ptr())
        r.synchronize()
        assert r.bin_info()["reason"] == "on" and bool(r.last_instance() & PAIR) == pairs
        last = r.readback_radiance()
    s = oracle.Scene(*scene)
    frames = [s.render(w, h, p, rt.resize_intrinsic(w, h), spp=64)[:2] for p in poses]
    s.close()
    assert not np.array_equal(frames[0][0], frames[1][0])
    for b, f in zip(bufs, frames):
        assert np.array_equal(b.cpu().numpy(), f[0])
    assert np.array_equal(_bits(last), _bits(frames[1][1]))


def test_packed_tiles_with_an_edge_tile(gpu, hooks, refs):
    """64-pixel tiles of the 71x45 frame (Frame<105>): the second tile holds
    seven columns of the image, the rest of its wave tiles lie off it."""
    import torch
    hooks()
    w, h = SIZES[0]
    scene = _entry_scene(w, h)
    ts, ids = 64, np.arange(2, dtype=np.uint32)
    with _renderer(scene, w, h, 64, pose=POSE) as r:
        buf = torch.full((len(ids) * ts * ts * 4,), 0x5A, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        r.render_tiles(ids, ts, buf.data_ptr())
        assert r.last_instance() == TILES | WAVEQ | OCC | BINS
        r.unpack_tiles(buf.data_ptr(), ids, ts)
        assert np.array_equal(r.readback(), refs(("entry", False, False), scene, w, h, POSE)[0])


# ---------------------------------------------------------------------------
# the occluder loop
# ---------------------------------------------------------------------------

def _shadow_scene(w, h):
    """Pairs on row ROW whose two pixels' occluder lists differ: at FIRST_A
    pixel A's sphere has one candidate, which covers it from the light, and
    pixel B's has three that only graze its rays (B runs to its list's end);
    at FIRST_B the reverse; a covered sphere on the last column (on the odd
    width its pair's B is off the image); a larger sphere lit on one side."""
    at, _ = _placer(w, h, POSE)
    to_light = -np.asarray(_L, np.float64)
    v = ROW + 0.5

    def covered(u, vv=v):
        s = at(u, vv, 0.6, 0.42)
        return [s, np.concatenate([s[:3] + 5.0 * s[3] * to_light, [1.3 * s[3]]])]

    def grazed(u):
        s = at(u, v, 0.6, 0.42)
        return [s] + [np.concatenate([s[:3] + (4.0 + 3.0 * k) * s[3] * to_light + (-1.0) ** k * 1.9 * s[3] * _E1, [s[3]]])
                      for k in range(3)]
    sp = covered(FIRST_A + 0.5) + grazed(FIRST_A + 1.5) + grazed(FIRST_B + 0.5) + covered(FIRST_B + 1.5)
    sp += covered(70.5, 30.5) + [at(44.0, 26.0, 0.6, 2.5)]
    sp = np.array(sp, np.float32)
    return sp, np.full(sp.shape[0], 0xFFD0B090, np.uint32)      # one albedo: pixels compare like for like


FIRST_A, FIRST_B = 20, 40
# sphere indices in _shadow_scene: covered = [sphere, cover], grazed = [sphere, 3 candidates]
S_A_COV, S_A_GRZ, S_B_GRZ, S_B_COV, S_LAST = 0, 2, 6, 10, 12


@pytest.mark.parametrize("w,h", SIZES)
def test_occluder_loop_each_pixel_to_its_own_end(gpu, hooks, refs, w, h):
    hooks(bin_cap=None)
    scene = _shadow_scene(w, h)
    want = refs("shadow", scene, w, h, POSE)

    def probe(r):
        assert r.last_instance() == WAVEQ | OCC | BINS | PAIR and r.scene_info()["occluder_lists_on"] == 1
        return r.export_occluders()[1]
    cnt = _three_ways(scene, w, h, POSE, want, probe=probe)
    # the lists: the cover, the three grazing candidates; none walks
    for cov, grz in ((S_A_COV, S_A_GRZ), (S_B_COV, S_B_GRZ)):
        assert cnt[cov] >= 1 and cnt[grz] >= 3
    assert cnt[S_LAST] >= 1 and (cnt != WALK).all()
    # what the shadow rays took away (against the frame without them): much
    # of the covered spheres' light, little of the grazed ones' (each sphere
    # lies within its pixel, so the pixels are the spheres')
    lit, rad = refs("shadow", scene, w, h, POSE, shadows=False)[1], want[1]
    assert (lit[ROW, [FIRST_A, FIRST_A + 1, FIRST_B, FIRST_B + 1], 0] != SKY_R).all()
    lost = (lit - rad)[..., :3].sum(axis=-1)
    for cov, grz in ((FIRST_A, FIRST_A + 1), (FIRST_B + 1, FIRST_B)):
        assert lost[ROW, cov] > 0.0 and lost[ROW, grz] < 0.5 * lost[ROW, cov]
    if w % 2:
        assert lost[30, w - 1] > 0.0                  # pixel A of the last pair; its B is off the image


@pytest.mark.parametrize("w,h", SIZES)
def test_shadows_off(gpu, hooks, refs, w, h):
    """No shadow rays: no occluder lists, so not a pair instance; the binned
    one-pixel path."""
    hooks(bin_cap=None)
    scene = _shadow_scene(w, h)

    def probe(r):
        assert r.last_instance() & (PAIR | OCC) == 0 and r.last_instance() & BINS
        return True
    _three_ways(scene, w, h, POSE, refs("shadow", scene, w, h, POSE, shadows=False), shadows=False, probe=probe)


@pytest.mark.parametrize("occ_cap", [None, 2], ids=["lists", "walk-headers"])
@pytest.mark.parametrize("w,h", SIZES)
def test_lists_of_every_length(gpu, oracle, hooks, w, h, occ_cap):
    """The column scene: lists of 0, 1, ... the cap; under a cap of 2, lists of
    0, 1 and the cap with walk headers beside them, so pairs fall back."""
    from bins_oracle import look_at_pose
    hooks(bin_cap=None, occ_cap=occ_cap)
    scene = _column_scene()
    c, a = scene[0][2, :3].astype(np.float64), np.radians(176.0)
    pose = look_at_pose(c + 0.5 * (np.cos(a) * _L + np.sin(a) * _E1), c)
    with _renderer(scene, w, h, 64, pose=pose) as r:
        K = _zoom(r, 6.0)
    s = oracle.Scene(*scene)
    ref8, ref32, cnts = s.render(w, h, pose, K, spp=64)
    s.close()
    assert int(cnts[1]) > 100                         # shadow rays were cast

    def probe(r):
        assert r.last_instance() & PAIR
        return r.export_occluders()[1], r.render_gbuffer(normals=False, albedo=False)["sphere"]
    cnt, g = _three_ways(scene, w, h, pose, (ref8, ref32), zoom=6.0, probe=probe)
    n = scene[0].shape[0]
    seen = set(g[g != WALK].tolist())
    if occ_cap is None:
        assert cnt.tolist() == list(range(n)) and {0, 1, 2, 3} <= seen
    else:
        assert cnt.tolist() == [0, 1, 2] + [WALK] * (n - 3) and {0, 1, 2, 3} <= seen
