"""GPU ray queries (rt_trace_rays, rt_pick) against the CPU oracle, ray by ray.

The query kernel runs the frame kernels' own walk in its generic mode, so
every ray's hit flag, t (bit for bit), sphere index and the summed node / prim
counters must equal oracle.Scene.trace, for nearest and for any-hit queries,
including rays no camera generates: origins on sphere surfaces, inside
spheres, outside the root box, tmin / tmax windows, axis-parallel and
degenerate directions.  The oracle's answers are computed once per scene and
kind and shared by the tests.
"""
import ctypes
import functools

import numpy as np
import pytest

import raytracingstudy_amd as rt
from raytracingstudy_amd import _lib
from raytracingstudy_amd.camera import scene_pose

from query_scaffold import CAM_H, CAM_W, assert_frames_undisturbed, scene_renderer

pytestmark = pytest.mark.gpu

NO_HIT = 0xFFFFFFFF
INF = np.float32(np.inf)
# A: 577 nodes, deepest leaf at depth 4.  B: a deep tree of small leaves with
# many overlapping spheres: multi-level pops, long leaf-to-leaf walks.
SCENES = {"A": dict(n=1000, max_depth=7, leaf_capacity=8),
          "B": dict(n=20000, max_depth=12, leaf_capacity=2)}
N_SURFACE, N_CAMERA, N_OUTSIDE = 2048, 1024, 1061  # 4133 rays: the largest size tested


@functools.lru_cache(maxsize=None)
def _spheres(name):
    return rt.generate_spheres(SCENES[name]["n"], rt.SEED)


@functools.lru_cache(maxsize=None)
def _oracle_scene(name):
    import oracle
    sp, al = _spheres(name)
    return oracle.Scene(sp, al, max_depth=SCENES[name]["max_depth"],
                        leaf_capacity=SCENES[name]["leaf_capacity"])


def _unit(g, n):
    d = g.normal(size=(n, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _rays(name):
    """(4133, 8) float32 in rt_ray layout: surface rays, camera rays, outside origins."""
    import oracle
    sp, _ = _spheres(name)
    g = np.random.default_rng(20240 + len(sp))
    rays = np.zeros((N_SURFACE + N_CAMERA + N_OUTSIDE, 8), np.float32)
    # origins just off random spheres' surfaces, random directions, a short window
    k = g.integers(0, len(sp), N_SURFACE)
    s = rays[:N_SURFACE]
    s[:, :3] = sp[k, :3] + np.float32(1.001) * sp[k, 3:4] * _unit(g, N_SURFACE)
    s[:, 3] = 1e-5
    s[:, 4:7] = _unit(g, N_SURFACE)
    s[:, 7] = 0.5
    # the frame's own camera rays
    pose, K = scene_pose(), oracle.resize_intrinsic(CAM_W, CAM_H)
    c = rays[N_SURFACE:N_SURFACE + N_CAMERA]
    px = g.integers(0, CAM_W * CAM_H, N_CAMERA)
    c[:, :3] = pose[3, :3]
    c[:, 3] = 0.0
    for i, p in enumerate(px):
        c[i, 4:7] = oracle.get_ray(pose, K, float(p % CAM_W), float(p // CAM_W))
    c[:, 7] = INF
    # origins anywhere around the root box [0, 1.28]^3, also outside it
    o = rays[N_SURFACE + N_CAMERA:]
    o[:, :3] = g.uniform(-0.5, 1.78, (N_OUTSIDE, 3))
    o[:, 3] = 0.0
    o[:, 4:7] = _unit(g, N_OUTSIDE)
    o[:, 7] = INF
    rays.setflags(write=False)
    return rays


def _oracle_trace(scene, rays, any_hit):
    """hit (n,) bool, t (n,) float32 (a miss: the ray's tmax), sphere (n,) uint32 (a miss:
    NO_HIT), and per-ray node / prim counts."""
    n = len(rays)
    hit = np.zeros(n, bool)
    t = np.zeros(n, np.float32)
    sphere = np.full(n, NO_HIT, np.uint32)
    nodes = np.zeros(n, np.uint64)
    prims = np.zeros(n, np.uint64)
    for i, r in enumerate(rays):
        h, th, idx, cnt = scene.trace(r[0:3], r[4:7], r[3], r[7], any_hit=any_hit)
        hit[i], t[i], sphere[i] = h, (th if h else r[7]), (idx if h else NO_HIT)
        nodes[i], prims[i] = cnt[2], cnt[3]
    return hit, t, sphere, nodes, prims


@functools.lru_cache(maxsize=None)
def _expected(name, kind):
    out = _oracle_trace(_oracle_scene(name), _rays(name), kind == "any")
    for a in out:
        a.setflags(write=False)
    return out


def _scene(name):
    tree = {k: SCENES[name][k] for k in ("max_depth", "leaf_capacity")}
    return (*_spheres(name), tree)


_renderer = functools.partial(scene_renderer, scene=_scene)


def _assert_equal(t, sphere, exp, n=None):
    hit, et, es = exp[0][:n], exp[1][:n], exp[2][:n]
    assert np.array_equal(sphere != NO_HIT, hit)
    assert np.array_equal(sphere, es)
    assert np.array_equal(t.view(np.uint32), et.view(np.uint32))  # bit-equal, NaN included


def test_ray_mix_is_not_vacuous(gpu, oracle):
    """The shared ray set exercises hits and misses, the any-hit order differs
    from the nearest sphere on some rays, and the oracle's walk agrees with
    brute force over all spheres (nearest) on it."""
    for name in SCENES:
        hit_n, _, sph_n, _, _ = _expected(name, "nearest")
        hit_a, _, sph_a, _, _ = _expected(name, "any")
        assert np.array_equal(hit_n, hit_a)
        surf = hit_n[:N_SURFACE]
        assert 0.25 * N_SURFACE < surf.sum() < 0.75 * N_SURFACE
        assert hit_n[N_SURFACE:N_SURFACE + N_CAMERA].any() and hit_n[N_SURFACE + N_CAMERA:].any()
        assert (sph_n != sph_a).sum() > 10
    sc, rays = _oracle_scene("A"), _rays("A")
    _, t_n, sph_n, _, _ = _expected("A", "nearest")
    for i in range(0, len(rays), 7):
        r = rays[i]
        h, t, idx, _ = sc.trace(r[0:3], r[4:7], r[3], r[7], brute=True)
        assert (idx if h else NO_HIT) == sph_n[i] and (not h or np.float32(t) == t_n[i])


@pytest.mark.parametrize("cell_table", [None, 0, 3])
@pytest.mark.parametrize("name", ["A", "B"])
def test_parity_and_stats(gpu, oracle, name, cell_table):
    """t bit-equal, sphere and hit flag equal, counters equal to the oracle's
    sums, for nearest and any; with the auto cell table, none (descents and
    stack pops only) and a depth-3 one (jumps and re-entries)."""
    rays = _rays(name)
    with _renderer(name, cell_table=cell_table) as r:
        for kind in ("nearest", "any"):
            exp = _expected(name, kind)
            t, sphere, st = r.trace_rays(rays, kind, stats=True)
            _assert_equal(t, sphere, exp)
            miss = sphere == NO_HIT
            assert np.array_equal(t[miss].view(np.uint32), rays[miss, 7].view(np.uint32))
            assert st.nodes_visited == int(exp[3].sum()) and st.prims_tested == int(exp[4].sum())
            assert (st.primary_rays, st.shadow_rays) == ((len(rays), 0) if kind == "nearest"
                                                         else (0, len(rays)))
            assert st.ms > 0.0
            # the plain launch (no counters) answers the same
            t2, sphere2 = r.trace_rays(rays, kind)
            assert np.array_equal(sphere2, sphere) and np.array_equal(t2.view(np.uint32), t.view(np.uint32))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 257, 4133])
def test_sizes_write_exactly_n_records(gpu, oracle, n):
    """Partial waves and blocks: every record below n is rewritten, the one at
    n is untouched (the buffer is pre-filled with 0xAB and one record longer)."""
    import torch
    rays = _rays("A")[:n]
    with _renderer("A") as r:
        d_rays = torch.from_numpy(rays.copy()).cuda()
        for kind in ("nearest", "any"):
            d_hits = torch.full((n + 1, 8), 0xAB, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            st = r.trace_rays_device(d_rays.data_ptr(), n, d_hits.data_ptr(), kind, stats=True)
            raw = d_hits.cpu().numpy()
            assert (raw[n] == 0xAB).all()
            hits = raw[:n].copy().view(np.uint32).reshape(n, 2)
            exp = _expected("A", kind)
            _assert_equal(hits[:, 0].copy().view(np.float32), hits[:, 1].copy(), exp, n)
            assert st.nodes_visited == int(exp[3][:n].sum()) and st.prims_tested == int(exp[4][:n].sum())


def test_zero_rays_and_argument_errors(gpu):
    lib = _lib.load()
    with rt.KernelRenderer(64, 64, mode="scene") as r:
        with pytest.raises(_lib.RtError) as e:  # no scene yet
            r.trace_rays(np.zeros((1, 8), np.float32))
        assert e.value.code == _lib.RT_E_NOSCENE
        with pytest.raises(_lib.RtError) as e:
            r.pick(1.0, 1.0)
        assert e.value.code == _lib.RT_E_NOSCENE
        sp, al = _spheres("A")
        r.set_scene(sp, al)
        st = _lib.RtStats()
        assert lib.rt_trace_rays(r._h, None, 0, _lib.RT_QUERY_NEAREST, None, None, None) == _lib.RT_OK
        assert lib.rt_trace_rays(r._h, None, 0, _lib.RT_QUERY_ANY, None, None, ctypes.byref(st)) == _lib.RT_OK
        assert (st.primary_rays, st.shadow_rays, st.nodes_visited) == (0, 0, 0)
        t, sphere = r.trace_rays(np.zeros((0, 8), np.float32))
        assert t.shape == (0,) and sphere.shape == (0,)
        fb = r.framebuffer_ptr()  # any valid device address: the call must refuse before using it
        assert lib.rt_trace_rays(r._h, fb, 1, 2, fb, None, None) == _lib.RT_E_INVALID
        assert lib.rt_trace_rays(r._h, None, 1, 0, fb, None, None) == _lib.RT_E_INVALID
        assert lib.rt_trace_rays(r._h, fb, 1, 0, None, None, None) == _lib.RT_E_INVALID
        with pytest.raises(KeyError):
            r.trace_rays_device(fb, 1, fb, "closest")


def test_edge_rays(gpu, oracle):
    """One small batch of rays a camera never casts (scene A); the oracle's
    answers for them were checked on the CPU when this was written.  The last
    two rays (NaN in z) are not given to the oracle: its walk has no defined
    answer for them (its exit-plane minimum is NaN there and no axis steps),
    so the miss is asserted directly."""
    sp, _ = _spheres("A")
    sc = _oracle_scene("A")
    nan = np.float32(np.nan)
    down = (0.0, 0.0, -1.0)
    _, t459, _, _ = sc.trace((0.64, 0.64, 3.0), down)
    k = 123  # no other sphere is entered or left before this one's surface along +x
    c = tuple(sp[k, :3])
    rays = np.array([
        (0.64, 0.64, 3.0, 0.0, *down, INF),              # 0 axis-parallel: sphere 459
        (0.64, 0.64, -3.0, 0.0, *down, INF),             # 1 the same line from behind the box
        (0.64, 0.64, 3.0, t459, *down, t459),            # 2 tmin == tmax (at the hit's own t)
        (0.64, 0.64, 3.0, 1.0, *down, 1.0),              # 3 tmin == tmax (elsewhere)
        (0.64, 0.64, 3.0, 0.0, *down, t459),             # 4 the hit at tmax exactly: t < tmax fails
        (0.64, 0.64, 3.0, t459, *down, INF),             # 5 the hit at tmin exactly: 459's far root
        (*c, 0.0, 1.0, 0.0, 0.0, INF),                   # 6 origin at a centre: that sphere at t = r
        (0.64, 0.64, 3.0, 0.0, 0.0, 0.0, 0.0, INF),      # 7 zero direction outside the box
        (0.01, 0.01, 0.01, 0.0, 0.0, 0.0, 0.0, INF),     # 8 zero direction inside it, in no sphere
        (0.64, 0.64, 3.0, 0.0, 0.0, 0.0, -INF, INF),     # 9 infinite direction component
        (0.64, INF, 3.0, 0.0, *down, INF),               # 10 infinite origin component
        (0.64, 0.64, 0.64, 0.0, nan, 0.6, 0.8, INF),     # 11 NaN direction component
        (0.64, 0.64, 0.64, 0.0, 0.6, nan, 0.8, INF),     # 12
        (0.64, nan, 0.64, 0.0, 0.6, 0.0, 0.8, INF),      # 13 NaN origin component
        (0.64, 0.64, 3.0, 0.0, *down, 2.0),              # 14 an ordinary miss: tmax before the hit
        (0.64, 0.64, 0.64, 0.0, 0.6, 0.8, nan, INF),     # 15 NaN in z: direction,
        (0.64, 0.64, nan, 0.0, 0.6, 0.0, 0.8, INF),      # 16 origin (GPU only, see above)
    ], np.float32)
    n_orc = 15
    with _renderer("A") as r:
        for kind in ("nearest", "any"):
            t, sphere = r.trace_rays(rays, kind)
            _assert_equal(t[:n_orc], sphere[:n_orc], _oracle_trace(sc, rays[:n_orc], kind == "any"))
            assert sphere[0] == 459 and abs(float(t[0]) - 2.87103) < 1e-5
            assert sphere[6] == k and abs(float(t[6]) / float(sp[k, 3]) - 1.0) < 1e-6
            for i in (1, 2, 3, 4, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16):
                assert sphere[i] == NO_HIT, i
                assert t[i].view(np.uint32) == rays[i, 7].view(np.uint32), i  # a miss: {tmax, RT_NO_HIT}
            assert sphere[5] == 459 and t[5] > t[0]


def test_pick_matches_oracle_and_the_rendered_image(gpu, oracle):
    """pick(u, v) = the oracle's getRay + trace at a grid of pixels; and, with no
    oracle involved, a 1-spp unjittered frame's R byte is the miss value 200
    exactly where pick misses."""
    sc = _oracle_scene("A")
    pose = scene_pose()
    origin = pose[3, :3].astype(np.float32)
    with _renderer("A", spp=1, jitter=False) as r:
        _, K = r.camera()
        r.render()
        img = r.readback()
        hits = 0
        for y in range(1, CAM_H, 5):
            for x in range(2, CAM_W, 5):
                hit, t, sphere, point = r.pick(float(x), float(y))
                d = oracle.get_ray(pose, K, float(x), float(y))
                eh, et, es, _ = sc.trace(origin, d)
                assert hit == eh
                assert (img[y, x, 0] == 200) == (not hit), (x, y)
                if hit:
                    hits += 1
                    assert sphere == es and np.float32(t) == np.float32(et)
                    assert np.array_equal(point, origin + np.float32(t) * d)
                else:
                    assert sphere == NO_HIT and t == np.inf
        assert 20 < hits < 200  # of 247 pixels: both outcomes are exercised
        assert r.pick(-1.0e6, 0.0)[0] is False  # far off the image: the ray misses the box


def test_queries_do_not_disturb_frames(gpu):
    """A progressive sequence of 3 frames with queries in between is byte-equal
    to the same frames without them, and a stats frame after a query counts
    what it counts without one."""
    rays = _rays("A")[:257]

    def queries(r):
        r.trace_rays(rays, "nearest", stats=True)
        r.trace_rays(rays, "any")
        r.pick(40.0, 30.0)

    assert_frames_undisturbed(functools.partial(_renderer, "A"), queries)


def test_device_pointers_on_a_torch_stream(gpu, oracle):
    import torch
    rays = _rays("A")
    n = len(rays)
    with _renderer("A") as r:
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            d_rays = torch.from_numpy(rays.copy()).cuda()
            d_hits = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
            for kind in ("nearest", "any"):
                assert r.trace_rays_device(d_rays.data_ptr(), n, d_hits.data_ptr(), kind,
                                           stream=s.cuda_stream) is None
                hits = d_hits.cpu().numpy()  # a copy on the same stream: ordered after the query
                _assert_equal(hits[:, 0].copy().view(np.float32), hits[:, 1].copy().view(np.uint32),
                              _expected("A", kind))
        s.synchronize()
        r.synchronize()


def test_multi_device_handle_answers_from_device_0(gpu, oracle):
    rays = _rays("A")[:1000]
    with _renderer("A", devices=[0, 0]) as r:
        r.render()
        for kind in ("nearest", "any"):
            t, sphere, st = r.trace_rays(rays, kind, stats=True)
            exp = _expected("A", kind)
            _assert_equal(t, sphere, exp, 1000)
            assert st.nodes_visited == int(exp[3][:1000].sum())
        hit, t, sphere, _ = r.pick(48.0, 32.0)
        with _renderer("A") as one:
            assert one.pick(48.0, 32.0)[:3] == (hit, t, sphere)
