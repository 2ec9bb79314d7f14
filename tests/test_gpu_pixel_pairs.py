"""Pixel pairs: a binned plain frame of 33 .. 64 spp
shades the pixels (x, y) and (x + 1, y), x even, of a ticket in one wave pass.

Frames of 71x45 and 70x44 (an odd and an even width, neither a multiple of 8:
the last pair of an odd row has its second pixel off the image, and the
right-hand blocks are edge blocks), byte for byte and the float radiance bit
for bit against the oracle and against the same scene with pairs switched off
(RT_FLAG_NO_PAIRS).
"""
import numpy as np
import pytest

from raytracingstudy_amd.camera import translation_pose

from bins_oracle import look_at_pose
from test_gpu_frame_chain import _E1, _L, _column_scene, _zoom
from test_gpu_occluders import _renderer

pytestmark = pytest.mark.gpu

WALK = 0xFFFFFFFF
PAIR, BINS, OCC, WAVEQ, TILES = 128, 64, 32, 8, 1
SIZES = [(71, 45), (70, 44)]
POSE = translation_pose(0.64, 0.64, 1.25)
BIN_CAP = 5


@pytest.fixture
def hooks(monkeypatch):
    def set_(bin_cap=BIN_CAP, occ_cap=None, bin_mean=1000000):
        monkeypatch.setenv("RT_TEST_BIN_MIN_SAMPLES", "0")
        monkeypatch.setenv("RT_TEST_BIN_MEAN", str(bin_mean))
        if bin_cap is not None:
            monkeypatch.setenv("RT_TEST_BIN_CAP", str(bin_cap))
        if occ_cap is not None:
            monkeypatch.setenv("RT_TEST_OCC_CAP", str(occ_cap))
    return set_


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# pixel pairs (A = the even pixel) on row 10 that the scene's small spheres sit on
A_ONLY, B_ONLY, BOTH, EDGE, TIE = 20, 24, 30, 36, 40
ROW = 10


def _pair_scene(w, h, inside=False):
    """For the FOV-80 camera of a w x h frame at POSE, spheres placed by pixel:
    one within pixel A of a pair, one within pixel B of another, one over both
    pixels of a pair, one whose edge runs between A and B, and two equal
    spheres (a tie in t in every sample, decided by the index) over a pair; a
    bin of exactly BIN_CAP spheres, one of BIN_CAP + 1 (it walks) beside a
    listed bin; a sphere over the last columns (its pair's B is off a 71-wide
    image); a sphere across the camera plane (wide: every pixel tests it).
    inside: also a sphere around the camera (wide as well)."""
    import raytracingstudy_amd as rt
    P = np.asarray(POSE, np.float64).reshape(4, 4)
    Kf = np.asarray(rt.resize_intrinsic(w, h), np.float64).reshape(-1)
    o, Rm = P[3, :3], P[:3, :3]

    def at(u, v, z, px):
        cam = np.array([(u - Kf[2]) / Kf[0] * z, (v - Kf[5]) / Kf[4] * z, z])
        return np.concatenate([o + cam @ Rm, [px * z / Kf[0]]])
    v = ROW + 0.5
    sp = [at(A_ONLY + 0.5, v, 0.6, 0.4), at(B_ONLY + 1.5, v, 0.6, 0.4), at(BOTH + 1.0, v, 0.6, 0.9),
          at(EDGE + 0.05, v, 0.6, 0.95), at(TIE + 1.0, v, 0.6, 0.9), at(TIE + 1.0, v, 0.6, 0.9)]
    sp += [at(12.0, 20.0, 0.5 + 0.01 * k, 1.5) for k in range(BIN_CAP)]          # bin (1, 2): the cap
    sp += [at(36.0, 20.0, 0.5 + 0.01 * k, 1.5) for k in range(BIN_CAP + 1)]      # bin (4, 2): over it
    sp += [at(44.0, 20.0, 0.6, 1.5), at(20.0, 36.0, 0.75, 2.5), at(70.2, 30.5, 0.65, 1.2)]
    sp += [np.concatenate([o + np.array([0.45, 0.0, 0.04]) @ Rm, [0.06]])]
    if inside:
        sp += [np.concatenate([o + np.array([0.01, 0.0, 0.0]) @ Rm, [0.62]])]
    sp = np.array(sp, np.float32)
    al = (0xFF000000 | (np.arange(sp.shape[0]) * 0x123457 + 0x405060) & 0xFFFFFF).astype(np.uint32)
    return sp, al


@pytest.fixture(scope="module")
def refs(oracle):
    """ref(w, h, spp, **oracle arguments) -> the oracle's (rgba8, radiance) of
    the pair scene, each computed once."""
    import raytracingstudy_amd as rt
    cache, scenes = {}, {}

    def ref(w, h, spp, inside=False, pose=POSE, **kw):
        key = (w, h, spp, inside, np.asarray(pose).tobytes(), tuple(sorted(kw.items())))
        if key not in cache:
            if (w, h, inside) not in scenes:
                scenes[(w, h, inside)] = oracle.Scene(*_pair_scene(w, h, inside))
            cache[key] = scenes[(w, h, inside)].render(w, h, pose, rt.resize_intrinsic(w, h), spp=spp, **kw)[:2]
        return cache[key]
    yield ref
    for s in scenes.values():
        s.close()


def _frame(r):
    r.render()
    return r.readback(), r.readback_radiance()


def _same(got, want, what):
    assert np.array_equal(got[0], want[0]), what
    assert np.array_equal(_bits(got[1]), _bits(want[1])), what


def test_the_pair_scene_has_the_cases(gpu, hooks):
    hooks()
    w, h = SIZES[0]
    scene = _pair_scene(w, h)
    with _renderer(scene, w, h, 64, pose=POSE) as r:
        r.render()
        assert r.last_instance() == WAVEQ | OCC | BINS | PAIR
        bi = r.bin_info()
        hdr, idx, wide = r.export_bins()
        (tw, th), words = r.export_bin_tiles()
    nbx = (w + 7) // 8
    assert bi["reason"] == "on" and (tw, th) == (1, 1) and wide.tolist() == [scene[0].shape[0] - 1]
    cnt = hdr[:, 1].reshape(-1, nbx)
    assert cnt[2, 1] == BIN_CAP and cnt[2, 4] == WALK and cnt[2, 5] == 1      # the cap, over it, listed
    assert cnt[2, 2] == 0 and cnt[2, 3] == 0                                 # empty bins

    def word(x, y=ROW):
        return int(words[(y // 8) * nbx + x // 8, (y % 8) * 8 + x % 8])
    assert word(A_ONLY) and not word(A_ONLY + 1)
    assert not word(B_ONLY) and word(B_ONLY + 1)
    assert word(BOTH) and word(BOTH) == word(BOTH + 1)
    assert word(EDGE)
    assert bin(word(TIE)).count("1") == 2 and word(TIE) == word(TIE + 1)
    assert word(70, 30) and w == 71                                          # the last pair: B off the image


@pytest.mark.parametrize("ticket_bits", [1, 2, 3])            # tickets of 1, 2, 4 wave tiles
@pytest.mark.parametrize("spp", [64, 48, 33])
@pytest.mark.parametrize("w,h", SIZES)
def test_pairs_against_oracle_and_one_pixel_path(gpu, hooks, refs, w, h, spp, ticket_bits):
    hooks()
    scene, want, out = _pair_scene(w, h), refs(w, h, spp), []
    for pairs in (True, False):
        with _renderer(scene, w, h, spp, pose=POSE, pairs=pairs, opt_off=ticket_bits << 4) as r:
            out.append(_frame(r))
            assert r.bin_info()["reason"] == "on"
            # (a ticket of one tile never pairs: the instance has the path and takes the other)
            assert r.last_instance() == WAVEQ | OCC | BINS | (PAIR if pairs else 0)
        _same(out[-1], want, (pairs, "oracle"))
    _same(out[0], out[1], "pairs on / off")


@pytest.mark.parametrize("spp", [32, 65])
def test_other_sample_counts_do_not_pair(gpu, hooks, refs, spp):
    """32 spp: two pixels a wave already; 65: two rounds (sorted rounds)."""
    hooks()
    w, h = SIZES[0]
    with _renderer(_pair_scene(w, h), w, h, spp, pose=POSE) as r:
        got = _frame(r)
        assert r.last_instance() & PAIR == 0 and r.last_instance() & WAVEQ
    _same(got, refs(w, h, spp), spp)


def test_swapped_columns_are_seen(gpu, hooks, refs):
    """Negative control: the oracle's frame with columns 2k and 2k + 1 swapped
    is not the GPU's frame, nor is its radiance."""
    hooks()
    w, h = SIZES[1]
    with _renderer(_pair_scene(w, h), w, h, 64, pose=POSE) as r:
        got = _frame(r)
    ref8, ref32 = refs(w, h, 64)
    swap = np.arange(w).reshape(-1, 2)[:, ::-1].reshape(-1)
    assert not np.array_equal(got[0], ref8[:, swap])
    assert not np.array_equal(_bits(got[1]), _bits(ref32[:, swap]))
    # ... in the pairs the scene was built for, and in plain sky (the miss colour follows the ray)
    # (in the radiance: two neighbouring sky pixels round to one RGBA8)
    for x in (A_ONLY, B_ONLY, EDGE, 2):
        assert not np.array_equal(_bits(got[1][ROW, x]), _bits(ref32[ROW, x + 1])), x
    for x in (A_ONLY, B_ONLY):
        assert not np.array_equal(got[0][ROW, x], ref8[ROW, x + 1]), x


@pytest.mark.parametrize("w,h", SIZES)
def test_a_dense_frame_walks(gpu, hooks, refs, w, h):
    """The builder's flag raised (a mean list length over the rule's): the pair
    instance runs and every pixel walks, by the one-pixel path."""
    hooks(bin_mean=0)
    with _renderer(_pair_scene(w, h), w, h, 64, pose=POSE) as r:
        got = _frame(r)
        assert r.bin_info()["reason"] == "dense" and r.last_instance() & PAIR
    _same(got, refs(w, h, 64), "dense")


@pytest.mark.parametrize("w,h", SIZES)
def test_camera_inside_a_sphere(gpu, hooks, refs, w, h):
    """Two wide spheres: each entry of the wide list against both pixels."""
    hooks()
    scene = _pair_scene(w, h, inside=True)
    out = []
    for pairs in (True, False):
        with _renderer(scene, w, h, 64, pose=POSE, pairs=pairs) as r:
            out.append(_frame(r))
            assert r.bin_info()["reason"] == "on" and r.bin_info()["wide"] == 2
            assert bool(r.last_instance() & PAIR) == pairs
        _same(out[-1], refs(w, h, 64, inside=True), pairs)
    assert np.unique(out[0][0].reshape(-1, 4), axis=0).shape[0] > 8


@pytest.mark.parametrize("kw", [{"shadows": False}, {"jitter": False}, {"shadows": False, "jitter": False}],
                         ids=["no-shadows", "no-jitter", "neither"])
def test_shadows_off_and_jitter_off(gpu, hooks, refs, kw):
    hooks()
    w, h = SIZES[0]
    with _renderer(_pair_scene(w, h), w, h, 48, pose=POSE, **kw) as r:
        got = _frame(r)
        # (without shadow rays a frame uses no occluder lists: not a pair instance)
        assert bool(r.last_instance() & PAIR) == kw.get("shadows", True)
    _same(got, refs(w, h, 48, **kw), kw)


@pytest.mark.parametrize("occ_cap", [None, 2])
def test_occluder_lists_of_a_pair(gpu, oracle, hooks, occ_cap):
    """Lists of 0, 1, 2, ...; under a cap of 2 the visible lists are of 0, 1
    and exactly the cap, with walk headers beside them: a pair whose A has a
    list and whose B walks, and the reverse."""
    hooks(bin_cap=None, occ_cap=occ_cap)
    w, h = SIZES[0]
    scene = _column_scene()
    # from the light's side, 4 degrees off the column's axis, facing sphere 2,
    # zoomed until a sphere is a few pixels wide: spheres 0 .. 2 (lists under a
    # cap of 2 as well) have spheres 3, 4, .. (walk headers) on both sides
    c, a = scene[0][2, :3].astype(np.float64), np.radians(176.0)
    pose = look_at_pose(c + 0.5 * (np.cos(a) * _L + np.sin(a) * _E1), c)
    out = []
    for pairs in (True, False):
        with _renderer(scene, w, h, 64, pose=pose, pairs=pairs) as r:
            K = _zoom(r, 6.0)
            out.append(_frame(r))
            assert r.bin_info()["reason"] == "on" and bool(r.last_instance() & PAIR) == pairs
            if pairs:
                assert r.scene_info()["occluder_lists_on"] == 1
                _, cnt, _, _ = r.export_occluders()
                g = r.render_gbuffer(normals=False, albedo=False)["sphere"]
    n = scene[0].shape[0]
    if occ_cap is None:
        assert cnt.tolist() == list(range(n))                 # 0, 1, ... exactly the cap
        assert {0, 1, 2, 3} <= set(g[g != WALK].tolist())     # seen: lists of 0, 1 and longer
    else:
        assert cnt.tolist() == [0, 1, 2] + [WALK] * (n - 3)
        assert {0, 1, 2} <= set(g[g != WALK].tolist())        # seen: lists of 0, 1 and exactly the cap
        hit = g != WALK
        walks = np.where(hit, cnt[np.where(hit, g, 0)] == WALK, False)
        lists = hit & ~walks
        even = slice(0, w - 1, 2)
        odd = slice(1, w, 2)
        assert (lists[:, even] & walks[:, odd]).any() and (walks[:, even] & lists[:, odd]).any()
    ref8, ref32, cnts = oracle.Scene(*scene).render(w, h, pose, K, spp=64)
    assert int(cnts[1]) > 100                                 # shadow rays were cast
    for got in out:
        _same(got, (ref8, ref32), occ_cap)


def test_packed_tiles_with_an_edge_tile(gpu, hooks, refs):
    """64-pixel tiles of the 71x45 frame: the second holds seven columns of the
    image, the rest of its wave tiles lie off it.  Packed tiles keep the
    one-pixel path with or without the switch."""
    import torch
    hooks()
    w, h = SIZES[0]
    ts, ids = 64, np.arange(2, dtype=np.uint32)
    packed = []
    for pairs in (True, False):
        with _renderer(_pair_scene(w, h), w, h, 64, pose=POSE, pairs=pairs) as r:
            buf = torch.full((len(ids) * ts * ts * 4,), 0x5A, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            r.render_tiles(ids, ts, buf.data_ptr())
            assert r.last_instance() == TILES | WAVEQ | OCC | BINS      # (packed tiles do not pair)
            r.unpack_tiles(buf.data_ptr(), ids, ts)
            assert np.array_equal(r.readback(), refs(w, h, 64)[0]), pairs
            packed.append(buf.cpu().numpy().copy())
    assert np.array_equal(packed[0], packed[1])


def test_three_frames_back_to_back(gpu, oracle, hooks):
    """Frames of three cameras queued on one stream without a wait."""
    import torch
    import raytracingstudy_amd as rt
    hooks()
    w, h = SIZES[0]
    scene = _pair_scene(w, h)
    poses = [POSE, translation_pose(0.65, 0.635, 1.24), translation_pose(0.63, 0.645, 1.26)]
    bufs = [torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda") for _ in poses]
    torch.cuda.synchronize()
    with _renderer(scene, w, h, 64, pose=POSE) as r:
        for p, b in zip(poses, bufs):
            r.setPosition(p)
            r.render(dev_ptr=b.data_ptr())
        r.synchronize()
        assert r.last_instance() & PAIR
    s = oracle.Scene(*scene)
    for p, b in zip(poses, bufs):
        assert np.array_equal(b.cpu().numpy(), s.render(w, h, p, rt.resize_intrinsic(w, h), spp=64)[0])
    s.close()
