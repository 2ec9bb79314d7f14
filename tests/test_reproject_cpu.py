"""CPU tests of a layer carried across camera motion (rt_reproject_layer; DESIGN.md
5.17): the header's arithmetic and its whole-image host loop
(csrc/rt_reproject_math.h through tests/native/reproject_math_dump.cpp) against
tests/reproject_ref.py bit for bit; the reference's own properties; whether the
accumulated layer does what it is for (the plain mean at rest, nearer a converged
layer than the frame's own while the camera moves); and the surface (header,
ctypes mirror, the error path with no renderer, the C++ wrapper).  The kernel runs
in test_gpu_reproject.py.
"""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from raytracingstudy_amd import _lib

import ao_ref as ar
import gbuffer_ref
import reproject_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
NO_HIT = rr.NO_HIT
INF = np.float32(np.inf)
NAN = np.float32(np.nan)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _hex(x):
    return "%08x" % _bits(np.float32(x)).reshape(-1)[0]


def _same(got_words, want):
    """Bit for bit; every NaN is one value (its payload is the platform's)."""
    got = np.asarray(got_words, np.uint32).view(np.float32).reshape(np.shape(want))
    return bool(((_bits(got) == _bits(want)) | (np.isnan(got) & np.isnan(want))).all())


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    """tests/native/reproject_math_dump.cpp, a stand-alone program built with the
    address and undefined-behaviour sanitizers; a sanitizer report fails the test."""
    d = tmp_path_factory.mktemp("reproject_math")
    exe = str(d / "reproject_math_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "reproject_math_dump.cpp")])

    def run(*args):
        r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, r.stderr
        return r.stdout
    run.dir = d
    return run


# ---- cameras and random frames -----------------------------------------------------
def _rot(axis, angle):
    c, s = np.cos(angle), np.sin(angle)
    m = np.eye(3)
    a, b = [(1, 2), (0, 2), (0, 1)][axis]
    m[a, a], m[a, b], m[b, a], m[b, b] = c, -s, s, c
    return m


def _pose(origin=(0.64, 0.64, 2.2), rot=None, flip=True):
    """A pose (4, 4) float32 in the renderer's layout: rows 0..2 the rotation's columns, row 3 the origin."""
    p = np.zeros((4, 4), np.float64)
    p[:3, :3] = np.diag([1.0, -1.0, -1.0]) if flip else np.eye(3)
    if rot is not None:
        p[:3, :3] = p[:3, :3] @ rot
    p[3, :3] = origin
    p[3, 3] = 1.0
    return p.astype(np.float32)


def _K(w, h, f=None, fy=None):
    """{fx, 0, cx, 0, fy, cy, 0, 0, 1}: the nine floats as Camera::getRay reads them."""
    f = float(max(w, h)) if f is None else f
    return np.array([f, 0, w / 2.0, 0, f if fy is None else fy, h / 2.0, 0, 0, 1], np.float32)


def _ray(pose, K, x, y):
    """Camera::getRay in float32, source order (the oracle's get_ray restated for tests that need no oracle)."""
    P, K = np.asarray(pose, np.float32).reshape(16), np.asarray(K, np.float32).reshape(9)
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    dx, dy, dz = (x - K[2]) / K[0], (y - K[5]) / K[4], np.float32(1.0)
    w = [P[k] * dx + P[4 + k] * dy + P[8 + k] * dz for k in range(3)]
    ln = np.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    return np.stack([c / ln for c in w], axis=-1).astype(np.float32)


def _frame(h, w, seed, pose, K, channels=1, miss_share=0.3, ids=12):
    """A random frame under a camera: sphere ids in blobs, depths around 1.5, a layer and counts."""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    sphere = ((xx // 3 + 2 * (yy // 2)) % ids).astype(np.uint32)
    sphere[g.random((h, w)) < miss_share] = NO_HIT
    t = np.where(sphere != NO_HIT, (1.5 + 0.01 * g.random((h, w))).astype(np.float32), INF).astype(np.float32)
    layer = g.random((h, w) if channels == 1 else (h, w, 4)).astype(np.float32)
    count = g.integers(1, 40, (h, w)).astype(np.float32)
    dirs = _ray(pose, K, xx, yy)
    return dict(sphere=sphere, t=t, layer=layer, count=count, dirs=dirs, pose=pose, K=K,
                o=np.asarray(pose, np.float32).reshape(4, 4)[3, :3])


def _image(dump, cur, hist, channels, max_count=32.0, depth_tol=0.05, tag="img"):
    """reproject_pixel over every pixel through the dump program -> (out words, count words)."""
    h, w = cur["sphere"].shape
    path = str(dump.dir / f"{tag}_{w}_{h}_{channels}.bin")
    with open(path, "wb") as f:
        np.array([w, h, channels, 0 if hist is None else 1], np.uint32).tofile(f)
        np.array([max_count, depth_tol, *cur["o"]], np.float32).tofile(f)
        for a in (cur["dirs"], cur["sphere"], cur["t"], cur["layer"]):
            np.ascontiguousarray(a).tofile(f)
        if hist is not None:
            np.asarray(hist["pose"], np.float32).reshape(16).tofile(f)
            np.asarray(hist["K"], np.float32).reshape(9).tofile(f)
            for a in (hist["sphere"], hist["t"], hist["layer"], hist["count"]):
                np.ascontiguousarray(a).tofile(f)
    words = np.array([int(x, 16) for x in dump("image", path).split()], np.int64).astype(np.uint32)
    n = w * h
    assert len(words) == n * channels + n
    return words[:n * channels].reshape(cur["layer"].shape), words[n * channels:].reshape(h, w)


def _ref(cur, hist, **kw):
    return rr.reproject(cur["layer"], cur["sphere"], cur["t"], cur["dirs"], cur["o"], hist, **kw)


# ---- the header's arithmetic -----------------------------------------------------
def _point_grid():
    """Records {pose, K, o, d, t, W, H}: previous cameras (the same, shifted, rotated,
    zoomed, a negated focal length, facing away, a pose that is no rotation, a NaN
    entry) x rays of a 24x17 frame and a few extreme ones x hit distances."""
    W, H = 24, 17
    cur_pose, cur_K = _pose(), _K(W, H)
    poses = [(_pose(), _K(W, H)), (_pose((0.66, 0.63, 2.2)), _K(W, H)), (_pose(rot=_rot(1, 0.02)), _K(W, H)),
             (_pose(rot=_rot(2, 0.3)), _K(W, H, 40.0)), (_pose(), _K(W, H, -24.0)), (_pose(), _K(W, H, 24.0, -24.0)),
             (_pose(flip=False), _K(W, H)), (_pose((0.64, 0.64, -2.0)), _K(W, H)),
             (_pose(rot=_rot(0, np.pi / 2)), _K(W, H)), (_pose(rot=_rot(1, np.pi / 2)), _K(W, H))]
    skew = _pose()
    skew[0, :3] = (1.5, 0.25, 0.0)
    skew[2, :3] = (0.1, 0.0, -0.5)
    poses.append((skew, _K(W, H)))
    bad = _pose()
    bad[2, 2] = np.nan
    poses.append((bad, _K(W, H)))
    far = _pose((0.64, 0.64, 1e30))
    poses.append((far, _K(W, H, 1e30)))
    yy, xx = np.mgrid[0:H, 0:W]
    dirs = _ray(cur_pose, cur_K, xx, yy).reshape(-1, 3)
    dirs = np.concatenate([dirs, [[0, 0, -1], [1, 0, 0], [0, 0, 1], [np.nan, 0, -1]]]).astype(np.float32)
    ts = np.array([1.5, 0.0, 2.2, 1e-30, 3e38, np.inf, 2.0 + 2.0 ** -20], np.float32)
    rec = np.zeros(len(poses) * len(dirs) * len(ts), np.dtype([("pose", np.float32, 16), ("K", np.float32, 9),
                                                               ("o", np.float32, 3), ("d", np.float32, 3),
                                                               ("t", np.float32), ("W", np.uint32), ("H", np.uint32)]))
    assert rec.dtype.itemsize == 136
    k = 0
    for pose, K in poses:
        for d in dirs:
            for t in ts:
                rec[k] = (pose.reshape(16), K, cur_pose[3, :3], d, t, W, H)
                k += 1
    # exact projections (f = 32, a power of two): the point 2 * ((x - cx) / f, (cy - y) / f, -1) lands on
    # pixel (x, y) with a = b = 0
    ex = np.zeros(6, rec.dtype)
    for n, (x, y) in enumerate([(0, 0), (23, 16), (12, 8), (24, 17), (-1, 5), (5, -1)]):
        d = np.array([(x - 12.0) / 32.0, -(y - 8.5) / 32.0, -1.0], np.float32)
        ex[n] = (_pose((0, 0, 0)).reshape(16), _K(W, H, 32.0), (0, 0, 0), d, 2.0, W, H)
    return np.concatenate([rec, ex])


def test_header_projection_is_the_reference_bit_for_bit(dump):
    rec = _point_grid()
    path = str(dump.dir / "points.bin")
    rec.tofile(path)
    lines = dump("points", path).splitlines()
    assert len(lines) == len(rec) >= 20000
    got = np.array([[int(x, 16) for x in ln.split()[:5] + ln.split()[6:]] for ln in lines], np.int64).astype(np.uint32)
    flags = np.array([[int(c) for c in ln.split()[5]] for ln in lines], bool)
    want = np.zeros((len(rec), 9), np.float32)
    want_flags = np.zeros((len(rec), 5), bool)
    # per previous camera (the records of one camera are contiguous): vectorised over its points
    keys = [r["pose"].tobytes() + r["K"].tobytes() for r in rec]
    start = 0
    while start < len(rec):
        end = start
        while end < len(rec) and keys[end] == keys[start]:
            end += 1
        s = slice(start, end)
        u0, v0, a, b, dist, front = rr.project(rec["pose"][start], rec["K"][start], rec["o"][start], rec["d"][s],
                                               rec["t"][s])
        want[s, :5] = np.stack([u0, v0, a, b, dist], axis=1)
        want[s, 5:] = np.stack([rr.weight(i, j, a, b) for j in range(2) for i in range(2)], axis=1)
        W, H = int(rec["W"][start]), int(rec["H"][start])
        want_flags[s] = np.stack([front, rr.inside(u0, W), rr.inside(u0 + np.float32(1), W), rr.inside(v0, H),
                                  rr.inside(v0 + np.float32(1), H)], axis=1)
        start = end
    assert _same(got, want)
    assert np.array_equal(flags, want_flags)
    # the grid reaches what it names
    u0, a, front = want[:, 0], want[:, 2], want_flags[:, 0]
    assert (~front).sum() >= 1000 and front.sum() >= 1000
    assert np.isnan(u0).sum() >= 100                                  # c_z a NaN or 0 / 0
    assert (front & (np.abs(u0) > 1e6)).sum() >= 10                   # far outside the image, in front
    assert (front & want_flags[:, 1] & (a == 0)).sum() >= 3           # a = 0: the tap i = 1 weighs 0
    assert (want_flags[:, 1] & ~want_flags[:, 2]).sum() >= 1          # u0 = W - 1: only the left column inside
    assert (~want_flags[:, 1] & want_flags[:, 2]).sum() >= 1          # u0 = -1: only the right column inside
    ex = want[-6:]
    assert np.array_equal(ex[:3, :4], np.array([[0, 0, 0, 0], [23, 16, 0, 0], [12, 8, 0, 0]], np.float32))
    assert np.array_equal(want_flags[-3:, 1:], np.array([[0, 0, 0, 0], [0, 1, 1, 1], [1, 1, 0, 1]], bool))


def test_header_tap_acceptance_is_the_reference(dump):
    s = np.array([0, 7, 7, 0xFFFFFFFE, NO_HIT], np.uint32)
    dists = np.array([1.0, 1.04, 1.05, 1.0500001, 1.06, 0.0, 1e-30, 3e38, np.inf, np.nan], np.float32)
    ts = np.array([1.0, 0.0, -0.0, 1e-30, 3e38, np.inf, np.nan, -1.0, 0.95, 1.05], np.float32)
    tols = np.array([0.05, 1e-6, 1.0, np.inf], np.float32)
    rows = [(a, b, d, t, tol) for a in s for b in s for d in dists for t in ts for tol in tols]
    rec = np.zeros(len(rows), np.dtype([("s", np.uint32), ("sh", np.uint32), ("dist", np.float32), ("t", np.float32),
                                        ("tol", np.float32)]))
    for name, col in zip(rec.dtype.names, zip(*rows)):
        rec[name] = np.array(col)
    assert rec.dtype.itemsize == 20
    path = str(dump.dir / "taps.bin")
    rec.tofile(path)
    got = np.array([int(x) for x in dump("taps", path).split()], bool)
    want = rr.accepted(rec["s"], rec["sh"], rec["dist"], rec["t"], rec["tol"])
    assert len(got) == len(rec) and np.array_equal(got, want)
    same = rec["s"] == rec["sh"]
    assert not want[~same].any() and want[same].sum() >= 100
    # depth_tol = +inf accepts every finite distance against t' > 0, and t' = 0 never: inf * 0 is a NaN
    wide = same & (rec["tol"] == INF)
    assert want[wide & (rec["t"] > 0) & np.isfinite(rec["dist"])].all()
    assert not want[wide & (rec["t"] == 0)].any()
    # t' = 0 under a finite tolerance accepts dist = 0 alone; a negative t' nothing
    zero = same & (rec["t"] == 0) & np.isfinite(rec["tol"])
    assert np.array_equal(want[zero], rec["dist"][zero] == 0)
    assert not want[same & (rec["t"] < 0)].any() and not want[same & np.isnan(rec["t"])].any()


def test_header_validity_table(dump):
    def valid(channels=1, max_count=32.0, tol=0.05, flags=0):
        got = dump("valid", channels, _hex(max_count), _hex(tol), flags).strip()
        want = rr.params_ok(channels, max_count, tol, flags)
        assert got == "".join(str(int(x)) for x in want), (channels, max_count, tol, flags)
        return got
    assert valid() == "1111" and valid(channels=4) == "1111"
    for channels in (0, 2, 3, 5, 8, 0xFFFFFFFF):
        assert valid(channels=channels) == "0011", channels
    for m, ok in ((1.0, 1), (2.5, 1), (32.0, 1), (3e38, 1), (0.99999994, 0), (0.0, 0), (-1.0, 0), (np.inf, 0),
                  (-np.inf, 0), (np.nan, 0)):
        assert valid(max_count=m) == ("1111" if ok else "0101"), m
    for tol, ok in ((0.05, 1), (np.inf, 1), (1e-45, 1), (0.0, 0), (-0.0, 0), (-1.0, 0), (-np.inf, 0), (np.nan, 0)):
        assert valid(tol=tol) == ("1111" if ok else "0110"), tol
    for flags in (1, 2, 0x80000000):
        assert valid(flags=flags) == "0111", flags


CAMERA_PAIRS = {
    "same": lambda w, h: ((_pose(), _K(w, h)), (_pose(), _K(w, h))),
    "shift": lambda w, h: ((_pose(), _K(w, h)), (_pose((0.66, 0.63, 2.25)), _K(w, h))),
    "rotate_zoom": lambda w, h: ((_pose(rot=_rot(2, 0.1)), _K(w, h, 1.2 * max(w, h))), (_pose(rot=_rot(1, 0.03)), _K(w, h))),
}


@pytest.mark.parametrize("pair", sorted(CAMERA_PAIRS))
@pytest.mark.parametrize("channels", [1, 4])
@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (24, 17)])
def test_header_host_loop_is_the_reference(dump, w, h, channels, pair):
    """reproject_pixel over every pixel equals the reference's words on random frames:
    the tap order, the skipped taps, the copies and the counts."""
    (p0, k0), (p1, k1) = CAMERA_PAIRS[pair](w, h)
    hist = _frame(h, w, 10 * w + h, p0, k0, channels)
    cur = _frame(h, w, 10 * w + h, p1, k1, channels, miss_share=0.2)      # the same blobs of ids, other misses
    cur["layer"] = np.random.default_rng(w + 7).random(cur["layer"].shape).astype(np.float32)
    taken = 0
    for max_count, tol in ((32.0, 0.05), (1.0, np.inf), (2.5, np.inf)):
        out, count = _image(dump, cur, hist, channels, max_count, tol, tag=pair)
        w_out, w_count, took = _ref(cur, hist, max_count=max_count, depth_tol=tol)
        assert _same(out, w_out) and _same(count, w_count)
        assert (w_count[took] <= max_count).all() and (w_count[~took] == 1).all()
        if max_count == 1.0:       # the smallest memory: alpha = 1, the history is weighed out up to a rounding
            assert np.abs(w_out - cur["layer"]).max() <= 2.0 ** -22
        taken += int(took.sum())
    assert taken > 0 or w * h <= 15


def test_no_history_and_an_all_miss_frame_copy(dump):
    w, h = 24, 17
    hist = _frame(h, w, 1, _pose(), _K(w, h), 4)
    cur = _frame(h, w, 2, _pose(), _K(w, h), 4)
    cur["layer"].reshape(-1)[::7] = np.nan
    cur["layer"].reshape(-1)[3::11] = np.inf
    for c, hs in ((cur, None), (dict(cur, sphere=np.full((h, w), NO_HIT, np.uint32), t=np.full((h, w), INF)), hist)):
        out, count = _image(dump, c, hs, 4, tag="copy")
        assert np.array_equal(out, _bits(c["layer"]))
        assert np.array_equal(count, _bits(np.ones((h, w), np.float32)))
        w_out, w_count, took = _ref(c, hs)
        assert np.array_equal(_bits(w_out), out) and np.array_equal(_bits(w_count), count) and not took.any()


def test_foreign_sphere_ids_give_counts_of_one(dump):
    w, h = 24, 17
    hist = _frame(h, w, 3, _pose(), _K(w, h), 1, miss_share=0.0)
    cur = _frame(h, w, 3, _pose(), _K(w, h), 1, miss_share=0.0)
    hist["sphere"] = hist["sphere"] + np.uint32(100)
    out, count = _image(dump, cur, hist, 1, 32.0, np.inf, tag="foreign")
    assert np.array_equal(out, _bits(cur["layer"])) and (count.view(np.float32) == 1).all()
    assert not _ref(cur, hist, depth_tol=np.inf)[2].any()
    # ... and with the ids back every pixel takes its history
    hist["sphere"] = cur["sphere"]
    assert _ref(cur, hist, depth_tol=np.inf)[2].all()


@pytest.mark.parametrize("channels", [1, 4])
def test_a_constant_layer_comes_back(dump, channels):
    """History and frame hold the constant c under any counts: hv = sv / sw and the
    blend return c up to the arithmetic's roundings.  The header's host loop is held
    to the reference's words; how far they stray from c is printed."""
    w, h = 24, 17
    (p0, k0), (p1, k1) = CAMERA_PAIRS["shift"](w, h)
    hist = _frame(h, w, 4, p0, k0, channels, miss_share=0.1)
    cur = _frame(h, w, 4, p1, k1, channels, miss_share=0.1)
    for c in (0.3, 1.0, 7.0e-3):
        hist["layer"] = np.full_like(hist["layer"], c)
        cur["layer"] = np.full_like(cur["layer"], c)
        out, count = _image(dump, cur, hist, channels, 32.0, np.inf, tag="const")
        w_out, w_count, took = _ref(cur, hist, depth_tol=np.inf)
        assert took.sum() >= 100
        assert _same(out, w_out) and _same(count, w_count)
        print("constant", c, "largest deviation", float(np.abs(w_out.astype(np.float64) - np.float32(c)).max()))


# ---- what the call is for: the oracle's frames ---------------------------------------
W, H, RADIUS = 24, 17, 0.1


def _oracle_frame(orc, pose, rays, salt, g=None):
    sp, al = ar.spheres("cloud")
    sc = ar.oracle_scene(orc, "cloud")
    K = orc.resize_intrinsic(W, H).reshape(9).copy()
    if g is None:
        g = gbuffer_ref.expected(orc, sc, sp, al, pose, K, W, H)
    e = ar.expected(orc, sc, sp, al, pose, K, W, H, rays, RADIUS, salt, g=g)
    return g, e["ao"], K


def _step(g, ao, pose, K, hist, **kw):
    out, count, took = rr.reproject(ao, g["sphere"], g["t"], g["dirs"], np.asarray(pose, np.float32)[3, :3], hist, **kw)
    return dict(sphere=g["sphere"], t=g["t"], layer=out, count=count, pose=pose, K=K), took


def test_at_rest_the_result_is_the_mean_of_the_layers(oracle, dump):
    """scene_pose, 6 frames of 4-ray layers over salts 0..5: from frame 1 on every hit
    pixel accepts history, its count is exactly k + 1, and the layer is within
    6 * 2^-23 * 6 of the float64 mean (at most 6 roundings a frame on values in [0, 1]).
    Every frame of the chain also goes through the header's host loop, which must
    give the reference's words: the properties hold for the header, not the reference alone."""
    pose = ar.pose("scene")
    g, _, K = _oracle_frame(oracle, pose, 4, 0)
    hit = g["sphere"] != NO_HIT
    assert 0.4 < hit.mean() < 0.8
    hist, layers = None, []
    for k in range(6):
        _, ao, _ = _oracle_frame(oracle, pose, 4, k, g)
        layers.append(ao.astype(np.float64))
        cur = dict(sphere=g["sphere"], t=g["t"], layer=ao, dirs=g["dirs"], o=np.asarray(pose, np.float32)[3, :3])
        h_out, h_count = _image(dump, cur, hist, 1, tag=f"rest{k}", **rr.DEFAULTS)
        hist, took = _step(g, ao, pose, K, hist, **rr.DEFAULTS)
        assert _same(h_out, hist["layer"]) and _same(h_count, hist["count"]), k
        if k:
            assert np.array_equal(took, hit), k
        assert (hist["count"][hit] == k + 1).all() and (hist["count"][~hit] == 1).all(), k
        err = float(np.abs(hist["layer"].astype(np.float64) - np.mean(layers, axis=0))[hit].max())
        print("frame", k, "largest distance from the float64 mean", err)
        assert err <= 6 * 2.0 ** -23 * 6, k


def test_moving_the_accumulated_layer_is_nearer_the_converged_one(oracle, dump):
    """The camera shifts 0.004 in x per frame, 5 frames, max_count 32.  On the fifth
    frame's hit pixels the accumulated layer's mean absolute error against that
    frame's 64-ray layer is strictly below the raw 4-ray layer's, and at least half
    of the hit pixels accepted history."""
    hist = None
    for k in range(5):
        pose = ar.pose("scene").copy()
        pose[3, 0] = np.float32(pose[3, 0] + np.float32(0.004) * np.float32(k))
        g, ao, K = _oracle_frame(oracle, pose, 4, k)
        cur = dict(sphere=g["sphere"], t=g["t"], layer=ao, dirs=g["dirs"], o=np.asarray(pose, np.float32)[3, :3])
        h_out, h_count = _image(dump, cur, hist, 1, 32.0, 0.05, tag=f"move{k}")
        hist, took = _step(g, ao, pose, K, hist, max_count=32.0, depth_tol=0.05)
        assert _same(h_out, hist["layer"]) and _same(h_count, hist["count"]), k    # the header's host loop too
    hit = g["sphere"] != NO_HIT
    target = _oracle_frame(oracle, pose, 64, 0, g)[1].astype(np.float64)
    err_raw = float(np.abs(ao.astype(np.float64) - target)[hit].mean())
    err_acc = float(np.abs(hist["layer"].astype(np.float64) - target)[hit].mean())
    share = float(took[hit].mean())
    print("hit pixels", int(hit.sum()), "accepted history", share, "MAE raw", err_raw, "accumulated", err_acc)
    assert hit.sum() >= 100 and err_raw > 0.0
    assert err_acc < err_raw
    assert share >= 0.5


# ---- surface -----------------------------------------------------------------------
def _header():
    src = open(os.path.join(INCLUDE, "rt.h")).read()
    return " ".join(re.sub(r"/\*.*?\*/", "", src, flags=re.S).split())


def test_header_declares_the_call():
    src = _header()
    assert ("typedef struct rt_history { const void* dev_hits; const void* dev_layer; const void* dev_count; "
            "float pose[16]; float K[9]; } rt_history;") in src
    assert ("typedef struct rt_reproject_params { uint32_t channels; float max_count; float depth_tol; "
            "uint32_t flags; } rt_reproject_params;") in src
    assert "void rt_reproject_params_default(rt_reproject_params*);" in src
    assert ("int rt_reproject_layer(rt_renderer* r, const rt_reproject_params* p, const void* dev_hits, "
            "const rt_history* hist, const void* dev_cur, void* dev_out, void* dev_count_out, void* stream, "
            "rt_stats* stats);") in src
    assert re.search(r"#define RT_ABI_VERSION 4\b", src)  # additive: the version stays


def test_ctypes_mirror_and_defaults():
    lib = _lib.load()
    assert lib.rt_abi_version() == 4
    assert ctypes.sizeof(_lib.RtReprojectParams) == 16
    assert [f[0] for f in _lib.RtReprojectParams._fields_] == ["channels", "max_count", "depth_tol", "flags"]
    assert ctypes.sizeof(_lib.RtHistory) == 3 * ctypes.sizeof(ctypes.c_void_p) + 25 * 4 + 4   # padded to a pointer
    assert [f[0] for f in _lib.RtHistory._fields_] == ["dev_hits", "dev_layer", "dev_count", "pose", "K"]
    assert _lib.RtHistory.pose.offset == 24 and _lib.RtHistory.K.offset == 88
    res, args = _lib.SIGNATURES["rt_reproject_layer"]
    assert res is ctypes.c_int and len(args) == 9
    assert args[1]._type_ is _lib.RtReprojectParams and args[3]._type_ is _lib.RtHistory
    p = _lib.RtReprojectParams(9, 9.0, 9.0, 9)
    lib.rt_reproject_params_default(ctypes.byref(p))
    assert (p.channels, p.max_count, p.flags) == (1, 32.0, 0)
    assert _bits(np.float32(p.depth_tol)) == _bits(np.float32(0.05))
    assert (p.max_count, float(np.float32(p.depth_tol))) == (rr.DEFAULTS["max_count"],
                                                             float(np.float32(rr.DEFAULTS["depth_tol"])))
    lib.rt_reproject_params_default(None)   # tolerated


def test_a_call_without_a_renderer_is_an_error_not_a_crash():
    lib = _lib.load()
    p = _lib.RtReprojectParams(1, 32.0, 0.05, 0)
    assert lib.rt_reproject_layer(None, ctypes.byref(p), None, None, None, None, None, None, None) == _lib.RT_E_INVALID
    assert b"rt_reproject_layer" in lib.rt_last_error(None)


def test_cpp_wrapper_with_the_call_compiles(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "no C++ compiler"
    src = tmp_path / "use_reproject.cpp"
    src.write_text('#include <cmath>\n#include "rt_renderer.hpp"\n'
                   "float use(rtamd::KernelRenderer& r, const void* hits, const void* cur, void* out, void* count,\n"
                   "          const rt_history& hist, void* stream) {\n"
                   "    rt_stats st;\n"
                   "    r.reprojectLayer(hits, nullptr, cur, out, count);\n"
                   "    r.reprojectLayer(hits, &hist, cur, out, count, 4u, 8.0f, INFINITY, stream, &st);\n"
                   "    rt_reproject_params p;\n"
                   "    rt_reproject_params_default(&p);\n"
                   "    static_assert(sizeof(rt_reproject_params) == 16, \"the ABI's size\");\n"
                   "    static_assert(sizeof(rt_history) == 3 * sizeof(void*) + 25 * sizeof(float) + 4, \"the ABI's size\");\n"
                   "    return st.ms + p.depth_tol;\n"
                   "}\n")
    r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", INCLUDE, str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
