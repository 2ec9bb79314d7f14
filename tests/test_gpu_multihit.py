"""GPU ordered multi-hit queries (rt_trace_rays_multi, rt_pick_multi; DESIGN.md
5.9) against the brute-force CPU reference of tests/multihit_ref.py, which
test_multihit_cpu.py pins to the oracle: every slot's t bits and sphere index,
every filler slot and every count, ray by ray.  The reference runs once per
scene at k = 16; a smaller k's answer is its first k columns.
"""
import ctypes
import functools

import numpy as np
import pytest

import raytracingstudy_amd as rt
from raytracingstudy_amd import _lib
from raytracingstudy_amd.camera import scene_pose

import multihit_ref as mr
import tie_scenes as ts
from query_scaffold import CAM_H, CAM_W, assert_frames_undisturbed
from query_scaffold import scene_renderer as _renderer  # overlap_ref's A, B and D are multihit_ref's

pytestmark = pytest.mark.gpu

NO_HIT = mr.NO_HIT
INF = np.float32(np.inf)
KS = (1, 2, 3, 4, 8, 16)


def _assert_answer(got, exp, rays, k, what=""):
    """got / exp: (t (n, k), sphere (n, k), count (n,)).  The direct assertions
    first, so that a failure says which property broke."""
    t, sphere, count = got
    et, es, ec = exp
    n = len(rays)
    assert t.shape == (n, k) and sphere.shape == (n, k) and count.shape == (n,), what
    held = np.arange(k)[None, :] < count[:, None]
    assert np.array_equal(sphere != NO_HIT, held), f"{what}: hits fill the first `count` slots"
    for i in range(n):
        s = sphere[i, :count[i]]
        assert len(set(s.tolist())) == len(s), f"{what}: ray {i} reports a sphere twice"
    a, b = t[:, :-1], t[:, 1:]
    both = held[:, 1:]
    assert np.all((a <= b)[both]), f"{what}: t ascending"
    tie = both & (a == b)
    assert np.all((sphere[:, :-1] < sphere[:, 1:])[tie]), f"{what}: tied spheres in index order"
    fill = np.broadcast_to(rays[:, 7:8], (n, k))
    assert np.array_equal(t[~held].view(np.uint32), fill[~held].view(np.uint32)), f"{what}: fillers hold tmax"
    assert np.array_equal(count, ec), f"{what}: counts"
    assert np.array_equal(sphere, es), f"{what}: sphere indices"
    assert np.array_equal(t.view(np.uint32), et.view(np.uint32)), f"{what}: t bits"


def test_ray_mixes_are_not_vacuous(gpu):
    """From the reference: D truncates at k = 16 and has rays with no hit; B has
    rays with three or more spheres (truncation at k = 2); A truncates too."""
    total = mr.expected("D")[3]
    assert (total > 16).sum() >= 16 and (total == 0).sum() >= 64
    assert (mr.expected("B")[3] >= 3).sum() >= 8
    assert (mr.expected("A")[3] >= 3).sum() >= 1
    info = None
    with _renderer("D") as r:
        info = r.scene_info()
    # the dense scene: many references per sphere, so spheres are met again
    assert info["n_prim_refs"] > 10 * info["n_spheres"]


@pytest.mark.parametrize("cell_table", [None, 0, 3])
@pytest.mark.parametrize("name", ["A", "B", "D"])
def test_parity(gpu, name, cell_table):
    """Every k on every scene, with the auto cell table, none and a depth-3 one;
    the stats launch and the plain launch answer the same."""
    rays = mr.rays(name)
    ref = mr.expected(name)
    with _renderer(name, cell_table=cell_table) as r:
        for k in KS:
            exp = mr.cut(ref, rays, k)
            t, sphere, count, st = r.trace_rays_multi(rays, k, stats=True)
            _assert_answer((t, sphere, count), exp, rays, k, f"{name} k={k} stats")
            assert (st.primary_rays, st.shadow_rays) == (len(rays), 0) and st.ms > 0.0
            _assert_answer(r.trace_rays_multi(rays, k), exp, rays, k, f"{name} k={k}")


@pytest.mark.parametrize("name", ["A", "B", "D"])
def test_k1_is_the_nearest_query_and_stats_grow_with_k(gpu, name):
    """k = 1: hits and all four stats equal trace_rays(kind="nearest"); over k
    the summed nodes and tests never decrease (a later stop visits no less)."""
    rays = mr.rays(name)
    with _renderer(name) as r:
        tn, sn, stn = r.trace_rays(rays, "nearest", stats=True)
        prev = None
        for k in KS:
            t, sphere, count, st = r.trace_rays_multi(rays, k, stats=True)
            cur = (st.nodes_visited, st.prims_tested)
            if k == 1:
                assert np.array_equal(sphere[:, 0], sn)
                assert np.array_equal(t[:, 0].view(np.uint32), tn.view(np.uint32))
                assert np.array_equal(count, (sn != NO_HIT).astype(np.uint32))
                assert (st.primary_rays, st.shadow_rays, st.nodes_visited, st.prims_tested) == (
                    stn.primary_rays, stn.shadow_rays, stn.nodes_visited, stn.prims_tested)
            else:
                assert cur[0] >= prev[0] and cur[1] >= prev[1], (k, prev, cur)
            prev = cur


def _tie_case(name):
    if name == "T":
        sc = ts.tangent_pairs()
        return sc, sc["rays"], ts.T_TREE
    import oracle
    sc = ts.SCENES[name]()
    P, K = ts.pose(), ts.intrinsic()
    px = sorted({p for pair in ts.tie_pixels(sc) for p in pair})
    rays = np.zeros((len(px), 8), np.float32)
    rays[:, :3] = P[3, :3]
    for i, (x, y) in enumerate(px):
        rays[i, 4:7] = oracle.get_ray(P, K, float(x), float(y))
    rays[:, 7] = INF
    return sc, rays, {}


@pytest.mark.parametrize("name", ["D", "M", "T"])
def test_ties(gpu, oracle, name):
    """tie_scenes' duplicates, mirror pairs and tangent pairs with k = 4: tied
    spheres in index order, exact duplicates both present, and the same with
    the sphere list reversed (the reference is computed for each order)."""
    sc, rays, tree = _tie_case(name)
    m = len(sc["sp"])
    for sp in (sc["sp"], sc["sp"][::-1].copy()):
        ref = mr.reference(sp, rays, 4)
        et, es, ec = ref[0], ref[1], ref[2]
        tied = (ec >= 2) & (et[:, 0] == et[:, 1])
        assert tied.sum() >= 30, "the scene's rays do tie"  # (test_ties_cpu.py shows why they do)
        assert np.all(es[tied, 0] < es[tied, 1])
        if name == "D":   # a duplicate pair is i and i + 60 in either order
            assert np.all(es[tied, 1] - es[tied, 0] == m // 2)
        with rt.KernelRenderer(ts.W, ts.H, mode="scene") as r:
            r.set_scene(sp, None, **tree)
            _assert_answer(r.trace_rays_multi(rays, 4), (et, es, ec), rays, 4, f"ties {name}")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_sizes_write_exactly_n_times_k_records(gpu, n):
    """Partial waves and blocks with k = 3: the n*k hits and n counts are
    rewritten, the record after each is untouched (0xAB-filled buffers one
    record longer); and dev_counts = NULL writes the same hits."""
    import torch
    k = 3
    rays = mr.rays("D")[:n]
    et, es, ec = mr.cut(mr.expected("D"), mr.rays("D"), k)
    with _renderer("D") as r:
        d_rays = torch.from_numpy(rays.copy()).cuda()
        for with_counts in (True, False):
            d_hits = torch.full((n * k + 1, 8), 0xAB, dtype=torch.uint8, device="cuda")
            d_cnt = torch.full((n + 1, 4), 0xAB, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            r.trace_rays_multi_device(d_rays.data_ptr(), n, k, d_hits.data_ptr(),
                                      d_cnt.data_ptr() if with_counts else None)
            r.synchronize()
            raw = d_hits.cpu().numpy()
            assert (raw[n * k] == 0xAB).all()
            hits = raw[:n * k].copy().view(np.uint32).reshape(n, k, 2)
            assert np.array_equal(hits[:, :, 1], es[:n])
            assert np.array_equal(hits[:, :, 0], et[:n].view(np.uint32))
            cnt = d_cnt.cpu().numpy()
            if with_counts:
                assert (cnt[n] == 0xAB).all()
                assert np.array_equal(cnt[:n].copy().view(np.uint32).reshape(n), ec[:n])
            else:
                assert (cnt == 0xAB).all()


def test_edge_rays(gpu):
    """Rays a camera never casts (scene A, test_gpu_query.py's batch): an origin
    inside a sphere reports that sphere's far root as its one entry, tmin /
    tmax windows cut the list at both ends, NaN / infinite rays have count 0
    and all fillers."""
    sp = mr.spheres("A")
    nan = np.float32(np.nan)
    down = (0.0, 0.0, -1.0)
    k = 4
    # a line of the shared mix through three spheres or more: its windows
    rays_a, ref_a = mr.rays("A"), mr.expected("A")
    b = int(np.flatnonzero((ref_a[3] >= 3) & (rays_a[:, 7] == INF))[0])
    o, d = tuple(rays_a[b, 0:3]), tuple(rays_a[b, 4:7])
    bt, bs = ref_a[0][b], ref_a[1][b]
    assert bt[0] < bt[1] < bt[2]
    j = 123  # no other sphere is entered or left before this one's surface along +x
    c = tuple(sp[j, :3])
    rays = np.array([
        (0.64, 0.64, 3.0, 0.0, *down, INF),              # 0 axis-parallel: sphere 459 alone
        (0.64, 0.64, -3.0, 0.0, *down, INF),             # 1 the same line from behind the box
        (*o, bt[0], *d, bt[0]),                          # 2 tmin == tmax (at a hit's own t)
        (*o, 0.0, *d, bt[0]),                            # 3 the first hit at tmax exactly: empty
        (*o, 0.0, *d, bt[1]),                            # 4 the second at tmax exactly: one entry
        (*o, bt[0], *d, INF),                            # 5 the first at tmin exactly: its far root
        (*c, 0.0, 1.0, 0.0, 0.0, INF),                   # 6 origin at a centre: the far root at t = r
        (0.64, 0.64, 3.0, 0.0, 0.0, 0.0, 0.0, INF),      # 7 zero direction outside the box
        (0.64, 0.64, 3.0, 0.0, 0.0, 0.0, -INF, INF),     # 8 infinite direction component
        (0.64, INF, 3.0, 0.0, *down, INF),               # 9 infinite origin component
        (0.64, 0.64, 0.64, 0.0, nan, 0.6, 0.8, INF),     # 10 NaN direction component
        (0.64, nan, 0.64, 0.0, 0.6, 0.0, 0.8, INF),      # 11 NaN origin component
        (0.64, 0.64, 0.64, 0.0, 0.6, 0.8, nan, 2.0),     # 12 NaN in z, a finite tmax
        (0.64, 0.64, nan, 0.0, 0.6, 0.0, 0.8, INF),      # 13
        (0.64, 0.64, 3.0, 0.0, *down, 2.0),              # 14 an ordinary miss: tmax before the hit
        (*o, bt[0], *d, bt[2]),                          # 15 a window open at both ends
    ], np.float32)
    ref = mr.reference(sp, rays, k)
    with _renderer("A") as r:
        t, sphere, count = r.trace_rays_multi(rays, k)
    _assert_answer((t, sphere, count), ref[:3], rays, k, "edge rays")
    assert sphere[0, 0] == 459 and count[0] == 1 and abs(float(t[0, 0]) - 2.87103) < 1e-5
    for i in (1, 2, 3, 7, 8, 9, 10, 11, 12, 13, 14):
        assert count[i] == 0 and np.all(sphere[i] == NO_HIT), i
        assert np.all(t[i].view(np.uint32) == rays[i, 7].view(np.uint32)), i
    assert count[4] == 1 and sphere[4, 0] == bs[0] and t[4, 0] == bt[0]
    # the first sphere's near root is not past tmin: it is listed once, at its far root
    at = list(sphere[5]).count(bs[0])
    assert at <= 1 and (at == 0 or t[5, list(sphere[5]).index(bs[0])] > bt[0])
    assert bs[1] in sphere[5] and bs[1] in sphere[15] and bs[2] not in sphere[15]
    assert sphere[6, 0] == j and abs(float(t[6, 0]) / float(sp[j, 3]) - 1.0) < 1e-6
    assert list(sphere[6]).count(j) == 1  # the near root (t < 0) is no second entry


def test_zero_rays_and_argument_errors(gpu):
    lib = _lib.load()
    with rt.KernelRenderer(64, 64, mode="scene") as r:
        with pytest.raises(_lib.RtError) as e:  # no scene yet
            r.trace_rays_multi(np.zeros((1, 8), np.float32), 2)
        assert e.value.code == _lib.RT_E_NOSCENE
        with pytest.raises(_lib.RtError) as e:
            r.pick_multi(1.0, 1.0, 2)
        assert e.value.code == _lib.RT_E_NOSCENE
        r.set_scene(mr.spheres("A"), None)
        st = _lib.RtStats()
        st.nodes_visited = 5
        assert lib.rt_trace_rays_multi(r._h, None, 0, 3, None, None, None, None) == _lib.RT_OK
        assert lib.rt_trace_rays_multi(r._h, None, 0, 3, None, None, None, ctypes.byref(st)) == _lib.RT_OK
        assert (st.primary_rays, st.nodes_visited) == (0, 0)
        t, sphere, count = r.trace_rays_multi(np.zeros((0, 8), np.float32), 3)
        assert t.shape == (0, 3) and sphere.shape == (0, 3) and count.shape == (0,)
        fb = r.framebuffer_ptr()  # any valid device address: the call must refuse before using it
        for k in (0, 17, 0xFFFFFFFF):
            assert lib.rt_trace_rays_multi(r._h, fb, 1, k, fb, None, None, None) == _lib.RT_E_INVALID
            assert lib.rt_trace_rays_multi(r._h, None, 0, k, None, None, None, None) == _lib.RT_E_INVALID
        assert lib.rt_trace_rays_multi(r._h, None, 1, 2, fb, None, None, None) == _lib.RT_E_INVALID
        assert lib.rt_trace_rays_multi(r._h, fb, 1, 2, None, None, None, None) == _lib.RT_E_INVALID
        hits = (_lib.RtHit * 16)()
        for k in (0, 17):
            assert lib.rt_pick_multi(r._h, 1.0, 1.0, k, hits, None) == _lib.RT_E_INVALID
        assert lib.rt_pick_multi(r._h, 1.0, 1.0, 2, None, None) == _lib.RT_E_INVALID
        assert lib.rt_pick_multi(r._h, 32.0, 32.0, 16, hits, None) == _lib.RT_OK  # count_out may be NULL


def test_pick_multi(gpu, oracle):
    """pick_multi(x, y, 4): its first entry is pick(x, y), and the list is a
    1-ray multi query of the oracle's getRay direction."""
    pose = scene_pose()
    origin = pose[3, :3].astype(np.float32)
    with _renderer("D", spp=1, jitter=False) as r:
        _, K = r.camera()
        seen = set()
        for y in range(1, CAM_H, 9):
            for x in range(2, CAM_W, 9):
                cnt, t, sphere = r.pick_multi(float(x), float(y), 4)
                hit, pt, ps, _ = r.pick(float(x), float(y))
                assert (cnt > 0) == hit and sphere[0] == (ps if hit else NO_HIT) and t[0] == np.float32(pt)
                ray = np.zeros((1, 8), np.float32)
                ray[0, :3] = origin
                ray[0, 4:7] = oracle.get_ray(pose, K, float(x), float(y))
                ray[0, 7] = INF
                qt, qs, qc = r.trace_rays_multi(ray, 4)
                assert cnt == qc[0] and np.array_equal(sphere, qs[0])
                assert np.array_equal(t.view(np.uint32), qt[0].view(np.uint32))
                seen.add(cnt)
        assert 4 in seen and len(seen) >= 2  # full lists and shorter ones
        assert r.pick_multi(-1.0e6, 0.0, 4)[0] == 0  # far off the image: the ray misses the box


def test_multi_queries_do_not_disturb_frames(gpu):
    """A progressive sequence of 3 frames with multi-hit queries in between is
    byte-equal to the same frames without them, and a stats frame after them
    counts what it counts without them (accumulated samples included)."""
    rays = mr.rays("A")[:257]

    def queries(r):
        r.trace_rays_multi(rays, 4, stats=True)
        r.trace_rays_multi(rays, 16)
        r.pick_multi(40.0, 30.0, 3)

    assert_frames_undisturbed(functools.partial(_renderer, "A"), queries)


def test_multi_device_handle_answers_from_device_0(gpu):
    rays = mr.rays("D")[:600]
    exp = tuple(a[:600] for a in mr.cut(mr.expected("D"), mr.rays("D"), 8))
    with _renderer("D", devices=[0, 0]) as r:
        r.render()
        t, sphere, count, st = r.trace_rays_multi(rays, 8, stats=True)
        _assert_answer((t, sphere, count), exp, rays, 8, "devices {0, 0}")
        got = r.pick_multi(48.0, 32.0, 4)
        with _renderer("D") as one:
            st1 = one.trace_rays_multi(rays, 8, stats=True)[3]
            assert (st.nodes_visited, st.prims_tested) == (st1.nodes_visited, st1.prims_tested)
            exp_pick = one.pick_multi(48.0, 32.0, 4)
        assert got[0] == exp_pick[0] and np.array_equal(got[2], exp_pick[2])
        assert np.array_equal(got[1].view(np.uint32), exp_pick[1].view(np.uint32))
