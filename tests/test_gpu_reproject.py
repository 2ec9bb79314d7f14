"""A layer carried across camera motion (rt_reproject_layer)
against tests/reproject_ref.py, bit for bit.

The guides are the handle's own G-buffer (rt_render_gbuffer is held to the oracle
in test_gpu_gbuffer.py), rendered at the previous pose and then at the current
one; the reference takes the same hits, layers and counts and gets its rays from
oracle.get_ray.  Every output buffer is pre-filled with 0xAB bytes and is one
pixel longer than the frame: an unwritten element and a write past the end both
show; this frame's layer and the history's three buffers are compared with their
uploads after every call.
"""
import ctypes

import numpy as np
import pytest

import raytracingstudy_amd as rt
from raytracingstudy_amd import _lib

import ao_ref as ar
import filter_ref as fr
import query_scaffold as qs
import reproject_ref as rr

pytestmark = pytest.mark.gpu

NO_HIT = rr.NO_HIT
INF = float("inf")
SIZES = [(1, 1), (5, 3), (37, 29), (70, 9), (129, 65)]
SETTINGS = [(m, d) for m in (1.0, 2.5, 32.0) for d in (0.05, INF)]
SENTINEL = 0xABABABAB
_RAYS = {}


def _scene(name):
    sp, al = ar.spheres("cloud")
    return sp, al, ar.TREE


def _renderer(w, h, **kw):
    return qs.scene_renderer("cloud", w, h, scene=_scene, **kw)


def _fill(n):
    import torch
    return torch.full((n,), SENTINEL - (1 << 32), dtype=torch.int32, device="cuda")


# ---- cameras -------------------------------------------------------------------------
def _rot_y(angle):
    c, s = np.cos(angle), np.sin(angle)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def _pose(shift=(0, 0, 0), rot=None):
    p = ar.pose("scene").astype(np.float64)
    if rot is not None:
        p[:3, :3] = p[:3, :3] @ rot
    p[3, :3] += shift
    return p.astype(np.float32)


def _K(w, h, zoom=1.0, flip=False):
    K = rt.resize_intrinsic(w, h).reshape(9).copy()
    if w == 1:      # the 37-wide frame's focal length with the principal point on the single column
        K[:] = rt.resize_intrinsic(37, h).reshape(9)
        K[2] = np.float32(0.25)
    K[0] *= np.float32(-zoom if flip else zoom)
    K[4] *= np.float32(zoom)
    return K


def _pairs(w, h):
    """name -> ((previous pose, K), (current pose, K))."""
    rest = (_pose(), _K(w, h))
    skew = _pose()
    skew[0, :3] = (1.25, 0.25, 0.0)
    skew[2, :3] = (0.125, 0.0, -0.75)
    return {"same": (rest, rest),
            "shifted": (rest, (_pose((0.004, -0.003, 0.01)), _K(w, h))),
            "rotated": (rest, (_pose(rot=_rot_y(0.01)), _K(w, h))),
            "zoomed": (rest, (_pose(), _K(w, h, 1.1))),
            "negated_focal": ((_pose(), _K(w, h, flip=True)), rest),
            "away": ((ar.pose("away"), _K(w, h)), rest),
            "no_rotation": ((skew, _K(w, h)), rest)}


def _rays(oracle, pose, K, w, h):
    key = (np.asarray(pose, np.float32).tobytes(), np.asarray(K, np.float32).tobytes(), w, h)
    if key not in _RAYS:
        d = rr.rays(oracle, pose, K, w, h)
        d.setflags(write=False)
        _RAYS[key] = d
    return _RAYS[key]


# ---- frames ----------------------------------------------------------------------------
def _random_layer(w, h, seed):
    g = np.random.default_rng(seed)
    v = (g.random((h, w, 4)) * 4.0 - 1.0).astype(np.float32)
    n = max(1, (w * h) // 40)
    for val in (np.nan, np.inf, -np.inf):
        v.reshape(-1)[g.integers(0, v.size, n)] = val
    return v


def _random_count(w, h, seed):
    g = np.random.default_rng(seed)
    return np.where(g.random((h, w)) < 0.5, g.integers(1, 40, (h, w)), 1.0 + 30.0 * g.random((h, w))).astype(np.float32)


def _frame(r, oracle, cam, channels, salt=0, count=None, move=True):
    """The handle's G-buffer hits under `cam` and a layer of that frame (channels 1:
    the 4-ray AO layer of `salt`; 4: a seeded float4 layer with NaN and infinite
    values), on the device and on the host, with counts for when it serves as a history.
    move=False: `cam` is the handle's camera already (setting a pose restarts a progressive mean)."""
    import torch
    w, h = r.width, r.height
    pose, K = cam
    if move:
        r.setPosition(pose)
        r.setIntrinsic(K)
    d_hits = torch.empty((h, w, 2), dtype=torch.int32, device="cuda")
    d_ao = torch.empty((h, w), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    r.render_gbuffer_device(d_hits.data_ptr())
    if channels == 1:
        r.render_ao_device(4, 0.1, d_ao.data_ptr(), salt=salt)
    r.synchronize()
    hits = d_hits.cpu().numpy()
    f = dict(d_hits=d_hits, pose=np.asarray(pose, np.float32), K=np.asarray(K, np.float32),
             t=np.ascontiguousarray(hits[..., 0]).view(np.float32), o=np.asarray(pose, np.float32).reshape(4, 4)[3, :3],
             sphere=np.ascontiguousarray(hits[..., 1]).view(np.uint32), dirs=_rays(oracle, pose, K, w, h))
    f["layer"] = d_ao.cpu().numpy() if channels == 1 else _random_layer(w, h, 100 * w + h + salt)
    f["d_layer"] = d_ao if channels == 1 else torch.from_numpy(f["layer"]).cuda()
    f["count"] = _random_count(w, h, w + salt) if count is None else count
    f["d_count"] = torch.from_numpy(f["count"]).cuda()
    torch.cuda.synchronize()
    return f


def _history(f):
    return dict(hits=f["d_hits"].data_ptr(), layer=f["d_layer"].data_ptr(), count=f["d_count"].data_ptr(),
                pose=f["pose"], K=f["K"])


def _run(r, cur, hist, max_count=32.0, depth_tol=0.05, stream=None, stats=False, move=True):
    """rt_reproject_layer under cur's camera into 0xAB-filled buffers one pixel longer
    than the frame -> (the layer's words, the counts' words[, the stats])."""
    import torch
    channels = 1 if cur["layer"].ndim == 2 else 4
    n = r.width * r.height
    out, cnt = _fill((n + 1) * channels), _fill(n + 1)
    if move:
        r.setPosition(cur["pose"])
        r.setIntrinsic(cur["K"])
    if stream is None:
        torch.cuda.synchronize()
    st = r.reproject_layer_device(cur["d_hits"].data_ptr(), cur["d_layer"].data_ptr(), out.data_ptr(), cnt.data_ptr(),
                                  None if hist is None else _history(hist), channels, max_count, depth_tol,
                                  stream=stream, stats=stats)
    if stream is None:
        r.synchronize()
    raw, raw_c = out.cpu().numpy().view(np.uint32), cnt.cpu().numpy().view(np.uint32)
    assert (raw[n * channels:] == SENTINEL).all() and raw_c[n] == SENTINEL
    for f in (cur,) if hist is None else (cur, hist):      # nothing the call reads is written
        assert np.array_equal(qs.bits(f["d_layer"].cpu().numpy()), qs.bits(f["layer"]))
        assert np.array_equal(qs.bits(f["d_count"].cpu().numpy()), qs.bits(f["count"]))
        assert np.array_equal(f["d_hits"].cpu().numpy()[..., 1].view(np.uint32), f["sphere"])
        assert np.array_equal(qs.bits(f["d_hits"].cpu().numpy()[..., 0].view(np.float32)), qs.bits(f["t"]))
    words = (raw[:n * channels].reshape(cur["layer"].shape), raw_c[:n].reshape(cur["sphere"].shape))
    return words + (st,) if stats else words


def _ref(cur, hist, max_count=32.0, depth_tol=0.05):
    return rr.reproject(cur["layer"], cur["sphere"], cur["t"], cur["dirs"], cur["o"], hist, max_count, depth_tol)


def _same(words, want):
    """Bit for bit; a NaN is a NaN whatever its payload.  The sentinel word is no
    NaN, so an unwritten element cannot pass as one."""
    got = words.view(np.float32)
    return bool(((words == qs.bits(want)) | (np.isnan(want) & np.isnan(got))).all())


def _check(r, cur, hist, max_count=32.0, depth_tol=0.05, **kw):
    got = _run(r, cur, hist, max_count, depth_tol, **kw)
    want = _ref(cur, hist, max_count, depth_tol)
    assert _same(got[0], want[0]) and _same(got[1], want[1]), (max_count, depth_tol)
    return got, want


# ---- against the reference -----------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 4])
@pytest.mark.parametrize("w,h", SIZES)
def test_reproject_is_the_reference(gpu, oracle, w, h, channels):
    """Every camera pair at the defaults and at one other setting, the shifted pair at
    every setting; the history's counts are seeded, whole and fractional."""
    took_any = {}
    with _renderer(w, h) as r:
        for name, (prev, now) in _pairs(w, h).items():
            hist = _frame(r, oracle, prev, channels, salt=1)
            cur = _frame(r, oracle, now, channels, salt=2)
            for max_count, tol in (SETTINGS if name == "shifted" else ((32.0, 0.05), (2.5, INF))):
                _, (_, w_count, took) = _check(r, cur, hist, max_count, tol)
                assert (w_count[~took] == 1).all() and (w_count[took] <= max_count).all()
                took_any[name] = took_any.get(name, 0) + int(took.sum())
            if name == "away":      # the previous camera looks the other way: c_z <= 0 everywhere
                assert took_any[name] == 0
        _check(r, cur, None)
    if (w, h) == (129, 65):     # the pairs are what their names say
        hit = cur["sphere"] != NO_HIT
        assert 0.3 < hit.mean() < 0.95
        for name in ("same", "shifted", "rotated", "zoomed"):
            assert took_any[name] > hit.sum(), name


def test_no_history_and_an_all_miss_frame_copy(gpu, oracle):
    w, h = 37, 29
    with _renderer(w, h) as r:
        rest = _pairs(w, h)["same"][0]
        away = (ar.pose("away"), _K(w, h))
        for channels in (1, 4):
            hist = _frame(r, oracle, rest, channels)
            for cur, hs in ((_frame(r, oracle, rest, channels, 3), None), (_frame(r, oracle, away, channels, 3), hist)):
                (out, count), _ = _check(r, cur, hs)
                assert hs is None or not (cur["sphere"] != NO_HIT).any()
                assert np.array_equal(out, qs.bits(cur["layer"]))
                assert np.array_equal(count, qs.bits(np.ones((h, w), np.float32)))


def test_garbage_history_is_the_reference(gpu, oracle):
    """Random sphere ids and depths, NaN and infinite counts, counts of 0 and 1e30."""
    import torch
    w, h = 37, 29
    with _renderer(w, h) as r:
        prev, now = _pairs(w, h)["shifted"]
        g = np.random.default_rng(31)
        for channels in (1, 4):
            cur = _frame(r, oracle, now, channels, 1)
            hist = _frame(r, oracle, prev, channels, 2)
            live = cur["sphere"][cur["sphere"] != NO_HIT]
            hist["sphere"] = np.where(g.random((h, w)) < 0.5, hist["sphere"], g.choice(live, (h, w))).astype(np.uint32)
            hist["t"] = np.where(g.random((h, w)) < 0.7, hist["t"],
                                 g.choice(np.array([0.0, -1.0, np.nan, np.inf, 1e-30], np.float32), (h, w)))
            hist["count"] = g.choice(np.array([0.0, 1.0, 1e30, np.nan, np.inf, 7.5], np.float32), (h, w))
            hits = np.stack([hist["t"].view(np.uint32), hist["sphere"]], axis=-1).view(np.int32)
            hist["d_hits"] = torch.from_numpy(np.ascontiguousarray(hits)).cuda()
            hist["d_count"] = torch.from_numpy(hist["count"]).cuda()
            torch.cuda.synchronize()
            took = capped = 0
            for max_count, tol in ((32.0, 0.05), (32.0, INF), (1.0, INF)):
                _, (_, w_count, t) = _check(r, cur, hist, max_count, tol)
                took += int(t.sum())
                capped += int((w_count[t] == max_count).sum())
                assert not np.isnan(w_count).any()      # fminf(NaN, max_count) = max_count: a NaN count restarts at the cap
            assert took > 50 and capped > 50


PATH = [((0, 0, 0), None, 1.0), ((0, 0, 0), None, 1.0), ((0.004, 0, 0), None, 1.0), ((0.008, -0.003, 0.01), None, 1.0),
        ((0.008, -0.003, 0.01), 0.01, 1.0), ((0.012, -0.003, 0.01), 0.02, 1.1)]


def _chain(r, oracle, channels, max_count):
    """Six frames along PATH on one handle, the device's own outputs fed back as the
    history -> the last (device frame, reference history); every frame is compared."""
    import torch
    w, h = r.width, r.height
    hist = ref_hist = None
    for k, (shift, angle, zoom) in enumerate(PATH):
        cam = (_pose(shift, None if angle is None else _rot_y(angle)), _K(w, h, zoom))
        cur = _frame(r, oracle, cam, channels, salt=k)
        out, count = _run(r, cur, hist, max_count)
        w_out, w_count, took = _ref(cur, ref_hist, max_count)
        assert _same(out, w_out) and _same(count, w_count), k
        if k == 1 and channels == 1:    # at rest: every hit pixel took its history, and counts 2
            assert np.array_equal(took, cur["sphere"] != NO_HIT) and (w_count[took] == 2).all()
        ref_hist = dict(sphere=cur["sphere"], t=cur["t"], layer=w_out, count=w_count, pose=cur["pose"], K=cur["K"])
        # the device's own words go back in as the next history
        hist = dict(cur, layer=out.view(np.float32), count=count.view(np.float32),
                    d_layer=torch.from_numpy(out.view(np.int32)).cuda().view(torch.float32),
                    d_count=torch.from_numpy(count.view(np.int32)).cuda().view(torch.float32))
        torch.cuda.synchronize()
    assert w_count.max() >= min(max_count, 3.0) and took.sum() > 0
    return hist, ref_hist


@pytest.mark.parametrize("channels,max_count", [(1, 32.0), (4, 2.5)])
def test_a_chain_of_frames_is_the_reference_chain(gpu, oracle, channels, max_count):
    """A one-bit error in one frame would compound through the fed-back history and show."""
    with _renderer(70, 41) as r:
        _chain(r, oracle, channels, max_count)


def test_chain_then_filter_then_apply_is_the_composed_references(gpu, oracle):
    import torch
    w, h = 37, 29
    with _renderer(w, h) as r:
        hist, ref_hist = _chain(r, oracle, 1, 32.0)
        d_nrm = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
        d_flt = _fill(w * h + 1)
        torch.cuda.synchronize()
        r.render_gbuffer_device(None, d_nrm.data_ptr())
        r.filter_layer_device(hist["d_layer"].data_ptr(), d_flt.data_ptr(), hist["d_hits"].data_ptr(), d_nrm.data_ptr())
        r.render()
        frame = r.readback()
        r.apply_layer_device(d_flt.data_ptr(), 0.25)
        got = r.readback()
        flt = fr.filter_layer(ref_hist["layer"], hist["sphere"], hist["t"], d_nrm.cpu().numpy())
        assert np.array_equal(d_flt.cpu().numpy().view(np.uint32)[:w * h].reshape(h, w), qs.bits(flt))
        assert np.array_equal(got, fr.apply_layer(frame, flt, 0.25)) and not np.array_equal(got, frame)


# ---- the call's surface ----------------------------------------------------------------
def test_same_call_twice_a_callers_stream_and_stats(gpu, oracle):
    import torch
    w, h = 70, 9
    with _renderer(w, h) as r:
        prev, now = _pairs(w, h)["shifted"]
        hist, cur = _frame(r, oracle, prev, 1, 1), _frame(r, oracle, now, 1, 2)
        (a, ac), _ = _check(r, cur, hist)
        b, bc = _run(r, cur, hist)
        assert np.array_equal(a, b) and np.array_equal(ac, bc)
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            c, cc = _run(r, cur, hist, stream=s.cuda_stream)
        s.synchronize()
        assert np.array_equal(a, c) and np.array_equal(ac, cc)
        d, dc, st = _run(r, cur, hist, stats=True)
        assert np.array_equal(a, d) and np.array_equal(ac, dc)
        assert st.ms > 0.0 and (st.primary_rays, st.shadow_rays, st.nodes_visited, st.prims_tested,
                                st.samples_per_pixel) == (0, 0, 0, 0, 0)


def test_frames_are_undisturbed(gpu, oracle):
    """Progressive frames with the call between them (one and four channels, with and
    without stats) are byte-equal to the frames without it, the sums untouched."""
    w, h = 37, 29

    def between(r):
        pose, K = r.camera()
        rest = (pose, K.reshape(9))
        for channels in (1, 4):
            hist = _frame(r, oracle, rest, channels, 1, move=False)
            cur = _frame(r, oracle, rest, channels, 2, move=False)
            got = _run(r, cur, hist, stats=channels == 4, move=False)
            want = _ref(cur, hist)
            assert _same(got[0], want[0]) and _same(got[1], want[1])

    qs.assert_frames_undisturbed(lambda **kw: _renderer(w, h, **kw), between)


def test_refused_calls_launch_nothing(gpu, oracle):
    """Every refused call returns RT_E_INVALID and leaves the 0xAB-filled outputs as they were."""
    import torch
    lib = _lib.load()
    w, h = 37, 29
    with _renderer(w, h) as r:
        prev, now = _pairs(w, h)["shifted"]
        hist, cur = _frame(r, oracle, prev, 1, 1), _frame(r, oracle, now, 1, 2)
        out, cnt = _fill(w * h * 4), _fill(w * h)
        torch.cuda.synchronize()
        ptr = dict(hits=cur["d_hits"].data_ptr(), cur=cur["d_layer"].data_ptr(), out=out.data_ptr(), cnt=cnt.data_ptr(),
                   h_hits=hist["d_hits"].data_ptr(), h_layer=hist["d_layer"].data_ptr(),
                   h_count=hist["d_count"].data_ptr())

        def code(channels=1, max_count=32.0, tol=0.05, flags=0, p=True, with_hist=True, **kw):
            a = dict(ptr)
            a.update(kw)
            prm = _lib.RtReprojectParams(channels, max_count, tol, flags)
            hs = _lib.RtHistory(a["h_hits"], a["h_layer"], a["h_count"], (ctypes.c_float * 16)(*hist["pose"].reshape(16).tolist()),
                                (ctypes.c_float * 9)(*hist["K"].reshape(9).tolist()))
            return lib.rt_reproject_layer(r._h, ctypes.byref(prm) if p else None, a["hits"],
                                          ctypes.byref(hs) if with_hist else None, a["cur"], a["out"], a["cnt"], None, None)

        bad = [dict(p=False), dict(hits=None), dict(cur=None), dict(out=None), dict(cnt=None), dict(h_hits=None),
               dict(h_layer=None), dict(h_count=None), dict(out=ptr["cur"]), dict(cur=ptr["out"]),
               dict(out=ptr["h_layer"]), dict(h_layer=ptr["out"]), dict(cnt=ptr["h_count"]), dict(h_count=ptr["cnt"]),
               dict(out=ptr["cur"], with_hist=False)]
        bad += [dict(channels=x) for x in (0, 2, 3, 5, 16)]
        bad += [dict(max_count=x) for x in (0.0, 0.5, 0.99999994, -1.0, float("nan"), INF, -INF)]
        bad += [dict(tol=x) for x in (0.0, -0.0, -1.0, float("nan"), -INF)]
        bad += [dict(flags=x) for x in (1, 2, 0x80000000)]
        for kw in bad:
            assert code(**kw) == _lib.RT_E_INVALID, kw
            assert b"rt_reproject_layer" in lib.rt_last_error(r._h)
        with pytest.raises(_lib.RtError) as e:
            r.reproject_layer_device(ptr["hits"], ptr["cur"], ptr["out"], ptr["cnt"], max_count=0.5)
        assert e.value.code == _lib.RT_E_INVALID
        r.synchronize()
        torch.cuda.synchronize()
        assert (out.cpu().numpy().view(np.uint32) == SENTINEL).all()
        assert (cnt.cpu().numpy().view(np.uint32) == SENTINEL).all()
        assert np.array_equal(qs.bits(cur["d_layer"].cpu().numpy()), qs.bits(cur["layer"]))
        assert code() == _lib.RT_OK and code(with_hist=False) == _lib.RT_OK     # the same arguments, valid, do write
        assert code(tol=INF, max_count=1.0) == _lib.RT_OK
        r.synchronize()
        assert not (out.cpu().numpy().view(np.uint32)[:w * h] == SENTINEL).any()
        assert not (cnt.cpu().numpy().view(np.uint32) == SENTINEL).any()


def test_the_call_needs_no_scene_and_the_tensor_wrapper_is_the_call(gpu, oracle):
    """A handle without a scene reprojects under hits it is given (another handle's);
    reproject_layer on torch tensors returns what the pointer call writes."""
    w, h = 37, 29
    with _renderer(w, h) as r:
        prev, now = _pairs(w, h)["rotated"]
        with rt.KernelRenderer(w, h, mode="scene") as bare:
            bare.resize(w, h)
            for channels in (1, 4):
                hist, cur = _frame(r, oracle, prev, channels, 1), _frame(r, oracle, now, channels, 2)
                (out, count), _ = _check(bare, cur, hist, 8.0, INF)
                t_out, t_count = bare.reproject_layer(cur["d_layer"], cur["d_hits"],
                                                      dict(hits=hist["d_hits"], layer=hist["d_layer"],
                                                           count=hist["d_count"], pose=hist["pose"], K=hist["K"]),
                                                      max_count=8.0, depth_tol=INF)
                assert t_out.shape == cur["d_layer"].shape and t_count.shape == (h, w)
                assert np.array_equal(qs.bits(t_out.cpu().numpy()), out)
                assert np.array_equal(qs.bits(t_count.cpu().numpy()), count)
                first, ones = bare.reproject_layer(cur["d_layer"], cur["d_hits"])
                assert np.array_equal(qs.bits(first.cpu().numpy()), qs.bits(cur["layer"])) and bool((ones == 1).all())
            # what would make the kernel read past a buffer is refused before anything runs
            import torch
            hist_t = dict(hits=hist["d_hits"], layer=hist["d_layer"], count=hist["d_count"], pose=hist["pose"],
                          K=hist["K"])
            one = cur["d_layer"][..., 0].contiguous()
            bad = [(cur["d_layer"][..., :3].contiguous(), cur["d_hits"], None),          # 3 channels
                   (cur["d_layer"], cur["d_hits"][:-1].contiguous(), None),              # a shorter G-buffer
                   (cur["d_layer"], cur["d_hits"][..., :1].contiguous(), None),
                   (cur["d_layer"], cur["d_hits"].to(torch.int64), None),
                   (cur["d_layer"].double(), cur["d_hits"], None),
                   (cur["d_layer"].transpose(0, 1), cur["d_hits"], None),                # not contiguous, wrong shape
                   (cur["d_layer"].cpu(), cur["d_hits"], None),                          # not on the device
                   (cur["d_layer"], cur["d_hits"].cpu(), None),
                   (one, cur["d_hits"], hist_t),                                         # a 4-channel history under 1 channel
                   (cur["d_layer"], cur["d_hits"], dict(hist_t, layer=one)),
                   (cur["d_layer"], cur["d_hits"], dict(hist_t, count=hist["d_count"][:-1].contiguous())),
                   (cur["d_layer"], cur["d_hits"], dict(hist_t, hits=hist["d_hits"][:, :-1].contiguous())),
                   (cur["d_layer"], cur["d_hits"], dict(hist_t, count=hist["d_count"].cpu())),
                   (cur["d_layer"], cur["d_hits"], dict(hist_t, hits=hist["d_hits"].view(torch.float32))),
                   (cur["d_layer"], cur["d_hits"], dict(hist_t, pose=hist["pose"].reshape(16)[:12])),
                   (cur["d_layer"], cur["d_hits"], dict(hist_t, K=hist["K"][:4]))]
            for layer, hits, hs in bad:
                with pytest.raises(ValueError):
                    bare.reproject_layer(layer, hits, hs)
            bare.resize(w + 1, h)      # buffers kept from before a resize
            with pytest.raises(ValueError):
                bare.reproject_layer(cur["d_layer"], cur["d_hits"], hist_t)


def test_multi_device_handle_answers_as_a_single_one(gpu, oracle):
    w, h = 37, 29
    prev, now = _pairs(w, h)["shifted"]
    with _renderer(w, h) as r:
        hist, cur = _frame(r, oracle, prev, 1, 1), _frame(r, oracle, now, 1, 2)
        (single, single_c), _ = _check(r, cur, hist)
    with _renderer(w, h, devices=[0, 0], transport="peer") as r:
        r.render()
        hist2, cur2 = _frame(r, oracle, prev, 1, 1), _frame(r, oracle, now, 1, 2)
        assert np.array_equal(qs.bits(cur2["layer"]), qs.bits(cur["layer"]))
        assert np.array_equal(cur2["sphere"], cur["sphere"])
        (multi, multi_c), _ = _check(r, cur2, hist2)
        assert np.array_equal(multi, single) and np.array_equal(multi_c, single_c)
