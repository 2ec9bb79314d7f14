"""The plain frame's per-pixel chain: the bins'
constants read once per wave and the shading records requested together; the
occluder lists' loop and the round's sum, which that round tried to reorder
and left as they were, are pinned here all the same.

Frames byte for byte against the oracle and against the same renderer with
RT_FLAG_NO_BINS / RT_FLAG_NO_OCCLUDERS:
* tickets of 1, 2 and 4 wave tiles of every shape over a scene whose
  neighbouring bins differ in kind (empty, listed, over the cap) and that has a
  wide sphere; as packed tiles with an edge tile; frames queued back to back;
* occluder lists of 0, 1, 2, 3 and exactly the cap, and "walk" headers beside
  lists in one wave;
* the float radiance of 1 .. 130 samples a pixel bit for bit: RGBA8 alone
  would hide a reordered sum.
"""
import numpy as np
import pytest

from raytracingstudy_amd.camera import translation_pose

from bins_oracle import look_at_pose
from test_gpu_bins import SCENES
from test_gpu_occluders import _renderer

pytestmark = pytest.mark.gpu

WALK = 0xFFFFFFFF
W, H = 70, 44                       # 9 x 6 bins, partial edge bins
POSE = translation_pose(0.64, 0.64, 1.25)       # inside the root box: a sphere can lie across its plane
BIN_CAP = 5


@pytest.fixture
def hooks(monkeypatch):
    def set_(bin_cap=None, occ_cap=None):
        monkeypatch.setenv("RT_TEST_BIN_MIN_SAMPLES", "0")
        monkeypatch.setenv("RT_TEST_BIN_MEAN", "1000000")
        if bin_cap is not None:
            monkeypatch.setenv("RT_TEST_BIN_CAP", str(bin_cap))
        if occ_cap is not None:
            monkeypatch.setenv("RT_TEST_OCC_CAP", str(occ_cap))
    return set_


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- 1. tickets across bins ----------------------------------------------------

def _ticket_scene(w=W, h=H, pose=POSE):
    """For the FOV-80 camera of a w x h frame at `pose`: a stack of BIN_CAP + 1
    spheres in bin (4, 2) (over the lowered cap: its tiles walk) beside one
    sphere in bin (5, 2); one sphere in bin (2, 4) beside the empty bin (3, 4);
    a sphere in the corner bin (8, 5), a partial one; and a sphere across the
    camera plane, off to the side: wide, tested by every tile."""
    import raytracingstudy_amd as rt
    P = np.asarray(pose, np.float64).reshape(4, 4)
    Kf = np.asarray(rt.resize_intrinsic(w, h), np.float64).reshape(-1)
    o, Rm = P[3, :3], P[:3, :3]

    def at(u, v, z, px):
        cam = np.array([(u - Kf[2]) / Kf[0] * z, (v - Kf[5]) / Kf[4] * z, z])
        return np.concatenate([o + cam @ Rm, [px * z / Kf[0]]])
    sp = [at(36.0, 20.0, 0.5 + 0.01 * k, 1.5) for k in range(BIN_CAP + 1)]
    sp += [at(44.0, 20.0, 0.6, 1.5), at(20.0, 36.0, 0.75, 1.5), at(67.5, 42.0, 0.65, 1.0)]
    wide = np.concatenate([o + np.array([0.45, 0.0, 0.04]) @ Rm, [0.06]])
    sp = np.array(sp + [wide], np.float32)
    al = (0xFF000000 | (np.arange(sp.shape[0]) * 0x123457 + 0x405060) & 0xFFFFFF).astype(np.uint32)
    return sp, al


@pytest.fixture(scope="module")
def ticket_refs(oracle):
    """The oracle's frames of the ticket scene, one per spp (shared)."""
    import raytracingstudy_amd as rt
    scene = _ticket_scene()
    s = oracle.Scene(*scene)
    K = rt.resize_intrinsic(W, H)
    refs = {spp: s.render(W, H, POSE, K, spp=spp)[:2] for spp in (64, 16, 4, 1)}
    s.close()
    return scene, refs


def test_the_ticket_scene_has_the_neighbours(gpu, hooks, ticket_refs):
    hooks(bin_cap=BIN_CAP)
    scene, _ = ticket_refs
    with _renderer(scene, W, H, 1, pose=POSE) as r:
        r.render()
        bi = r.bin_info()
        hdr, _, wide = r.export_bins()
    assert bi["reason"] == "on" and bi["bins"] == 9 * 6 and wide.tolist() == [scene[0].shape[0] - 1]
    cnt = hdr[:, 1].reshape(6, 9)
    # aligned pairs of one row: a ticket of two or four tiles holds both
    assert cnt[2, 4] == WALK and cnt[2, 5] == 1 and bi["overflowed_bins"] == 1
    assert cnt[4, 2] == 1 and cnt[4, 3] == 0
    assert cnt[5, 8] == 1 and np.count_nonzero(cnt) == 4


@pytest.mark.parametrize("ticket_bits", [1, 2, 3])          # tickets of 1, 2, 4 wave tiles
@pytest.mark.parametrize("spp", [64, 16, 4, 1])             # wave tiles of 1x1, 2x2, 4x4, 8x8 pixels
def test_tickets_across_bins(gpu, hooks, ticket_refs, spp, ticket_bits):
    hooks(bin_cap=BIN_CAP)
    scene, refs = ticket_refs
    ref8, ref32 = refs[spp]
    for bins in (True, False):
        with _renderer(scene, W, H, spp, pose=POSE, bins=bins, opt_off=ticket_bits << 4) as r:
            r.render()
            assert r.bin_info()["reason"] == ("on" if bins else "flag")
            assert np.array_equal(r.readback(), ref8), bins
            assert np.array_equal(_bits(r.readback_radiance()), _bits(ref32)), bins


@pytest.mark.parametrize("spp", [64, 4, 1])
def test_packed_tiles_with_an_edge_tile(gpu, hooks, ticket_refs, spp):
    """64-pixel tiles of the 70x44 frame: the second tile holds six columns of
    the image (the corner bin's sphere among them), the rest of its wave tiles
    lie off it."""
    import torch
    hooks(bin_cap=BIN_CAP)
    scene, refs = ticket_refs
    ts, ids = 64, np.arange(2, dtype=np.uint32)
    packed = []
    for bins in (True, False):
        with _renderer(scene, W, H, spp, pose=POSE, bins=bins) as r:
            buf = torch.zeros(len(ids) * ts * ts * 4, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            r.render_tiles(ids, ts, buf.data_ptr())
            assert r.bin_info()["enabled"] == (1 if bins else 0)
            r.unpack_tiles(buf.data_ptr(), ids, ts)
            assert np.array_equal(r.readback(), refs[spp][0]), bins
            packed.append(buf.cpu().numpy().copy())
    assert np.array_equal(packed[0], packed[1])


@pytest.mark.parametrize("frames", [2, 3])
def test_frames_back_to_back(gpu, oracle, hooks, ticket_refs, frames):
    """Frames of different cameras queued without a wait, each into its own
    buffer: every one is its camera's oracle frame."""
    import torch
    import raytracingstudy_amd as rt
    hooks(bin_cap=BIN_CAP)
    scene, _ = ticket_refs
    poses = [POSE, translation_pose(0.65, 0.635, 1.24), translation_pose(0.63, 0.645, 1.26)][:frames]
    bufs = [torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda") for _ in poses]
    torch.cuda.synchronize()
    with _renderer(scene, W, H, 16, pose=POSE) as r:
        for p, b in zip(poses, bufs):
            r.setPosition(p)
            r.render(dev_ptr=b.data_ptr())
        r.synchronize()
        assert r.bin_info()["reason"] == "on"
    s = oracle.Scene(*scene)
    for p, b in zip(poses, bufs):
        assert np.array_equal(b.cpu().numpy(), s.render(W, H, p, rt.resize_intrinsic(W, H), spp=16)[0])
    s.close()


# ---- 2. occluder lists -----------------------------------------------------------

OCC_CAP = 32                                  # kOccCap
OW, OH, OZOOM = 64, 48, 3.0
_L = np.array([1.0, 1.0, -1.0]) / np.sqrt(3.0)     # away from the light (the kernel's L is its negative)
_E1 = np.array([1.0, -1.0, 0.0]) / np.sqrt(2.0)
_E2 = np.cross(_L, _E1)


def _column_scene():
    """OCC_CAP + 1 equal spheres in a column away from the light, each pushed
    0.9 r off the axis in turning directions: every pair's discs overlap in the
    light plane, so sphere k's list holds the k spheres before it (0 .. the
    cap), and a shadow ray may pass some of them."""
    n, r = OCC_CAP + 1, 0.008
    k = np.arange(n)
    c = np.array([0.3, 0.3, 1.0])[None] + (k * 4.5 * r)[:, None] * _L[None] + \
        0.9 * r * (np.cos(2.4 * k)[:, None] * _E1[None] + np.sin(2.4 * k)[:, None] * _E2[None])
    sp = np.concatenate([c, np.full((n, 1), r)], 1).astype(np.float32)
    al = (0xFF000000 | (k * 0x0B0704 + 0x304050) & 0xFFFFFF).astype(np.uint32)
    return sp, al


def _column_camera(sp):
    """From the light's side, 8 degrees off the column's axis, facing sphere 2:
    the first spheres (lists of 0, 1, 2: lists under a cap of 2 as well) and
    the ones behind them (walk headers under that cap) share pixels."""
    c = sp[2, :3].astype(np.float64)
    a = np.radians(172.0)
    return look_at_pose(c + 0.5 * (np.cos(a) * _L + np.sin(a) * _E1), c)


def _zoom(r, zoom):
    _, K = r.camera()
    K = np.array(K, np.float32).copy()
    K[0, 0] *= zoom
    K[1, 1] *= zoom
    r.setIntrinsic(K)
    return K


@pytest.mark.parametrize("spp", [64, 4])
@pytest.mark.parametrize("occ_cap", [None, 2])
def test_occluder_lists(gpu, oracle, hooks, occ_cap, spp):
    hooks(occ_cap=occ_cap)
    scene = _column_scene()
    pose = _column_camera(scene[0])
    out = []
    for lists in (True, False):
        with _renderer(scene, OW, OH, spp, pose=pose, occluders=lists) as r:
            K = _zoom(r, OZOOM)
            r.render()
            out.append((r.readback(), r.readback_radiance()))
            if lists:
                assert r.scene_info()["occluder_lists_on"] == 1
                _, cnt, _, _ = r.export_occluders()
                g = r.render_gbuffer(normals=False, albedo=False)["sphere"]
    n = scene[0].shape[0]
    if occ_cap is None:
        assert cnt.tolist() == list(range(n))              # 0, 1, 2, 3, ... exactly the cap
    else:
        assert cnt.tolist() == [0, 1, 2] + [WALK] * (n - 3)
        # a wave (a pixel's 64 samples, or 4x4 pixels of 4) holds both kinds:
        # from the G-buffer's first hits at the pixel centres, tile by tile
        t = 1 if spp == 64 else 4
        hit = g != WALK
        kind = np.where(hit, cnt[np.where(hit, g, 0)] == WALK, False)
        lst = hit & ~kind
        if t > 1:
            both = [kind[y:y + t, x:x + t].any() and lst[y:y + t, x:x + t].any()
                    for y in range(0, OH, t) for x in range(0, OW, t)]
            assert any(both)
    ref8, ref32, cnts = oracle.Scene(*scene).render(OW, OH, pose, K, spp=spp)
    assert int(cnts[1]) > 100                               # shadow rays were cast
    for img, rad in out:
        assert np.array_equal(img, ref8) and np.array_equal(_bits(rad), _bits(ref32))


# ---- 3. round sums ------------------------------------------------------------------

SW, SH = 24, 16


@pytest.fixture(scope="module")
def sum_scene(oracle):
    s = oracle.Scene(*SCENES["S"])
    yield s
    s.close()


@pytest.mark.parametrize("progressive", [False, True])
@pytest.mark.parametrize("spp", [1, 2, 3, 4, 5, 8, 16, 32, 48, 64, 65, 130])
def test_round_sums(gpu, hooks, sum_scene, spp, progressive):
    """The float radiance equals the oracle's bit for bit: the round's pairwise
    sum in tree_sum's pairing, the rounds added in order; progressive frames
    onto the stored sums."""
    hooks()
    acc = np.zeros((SH, SW, 4), np.float32)
    for bins in (True, False):
        acc[:] = 0
        with _renderer(SCENES["S"], SW, SH, spp, progressive=progressive, bins=bins) as r:
            K = _zoom(r, 3.0)
            pose, _ = r.camera()
            for k in range(2 if progressive else 1):
                r.render()
                # (progressive frames below 8 spp run the block-tile queue, which reads no bins)
                assert r.bin_info()["reason"] == ("flag" if not bins else
                                                  "kernel" if progressive and spp < 8 else "on")
                ref8, ref32, _ = sum_scene.render(SW, SH, pose, K, spp=spp, frame=k,
                                                  accum=acc if progressive else None)
                assert np.array_equal(_bits(r.readback_radiance()), _bits(ref32)), (bins, k)
                assert np.array_equal(r.readback(), ref8), (bins, k)
    assert np.unique(_bits(ref32)[..., :3]).shape[0] > 50     # hits, shadows and sky: not one colour
