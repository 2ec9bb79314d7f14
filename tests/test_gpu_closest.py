"""GPU closest-sphere queries (rt_query_closest, rt_closest_at)
against the brute-force f32 reference of tests/closest_ref.py: every distance
bit, every sphere index, every filler and every count, probe by probe.  The
reference runs once per scene at k = 16; a smaller k's answer is its first k
columns.
"""
import ctypes
import functools

import numpy as np
import pytest

import raytracingstudy_amd as rt
from raytracingstudy_amd import _lib

import closest_ref as cr
import overlap_ref as ov
from query_scaffold import CAM_H, CAM_W, assert_frames_undisturbed
from query_scaffold import bits as _bits
from query_scaffold import scene_renderer as _renderer

pytestmark = pytest.mark.gpu

NO_HIT = cr.NO_HIT
INF = cr.INF
KS = (1, 2, 3, 4, 8, 16)


def _assert_answer(got, exp, pr, k, what=""):
    """got / exp: (dist (n, k), sphere (n, k), count (n,)); pr: the probes.  The
    direct assertions first, so that a failure says which property broke."""
    dist, sphere, count = got
    ed, es, ec = exp
    n = len(es)
    assert dist.shape == (n, k) and sphere.shape == (n, k) and count.shape == (n,), what
    assert count.max(initial=0) <= k, what
    held = np.arange(k)[None, :] < count[:, None]
    assert np.array_equal(sphere != NO_HIT, held), f"{what}: spheres fill the first `count` slots"
    radius = np.repeat(np.asarray(pr, np.float32)[:, 3:4], k, axis=1)
    assert np.array_equal(_bits(dist)[~held], _bits(radius)[~held]), f"{what}: a free slot holds the probe's radius"
    with np.errstate(invalid="ignore"):
        assert np.all((dist <= radius)[held]), f"{what}: every answer is within the radius"
        both = held[:, 1:]
        d0, d1, s0, s1 = dist[:, :-1], dist[:, 1:], sphere[:, :-1], sphere[:, 1:]
        assert np.all(((d0 < d1) | ((d0 == d1) & (s0 < s1)))[both]), f"{what}: ordered by (dist, sphere), none twice"
    assert np.array_equal(count, ec), f"{what}: counts"
    assert np.array_equal(sphere, es), f"{what}: sphere indices and fillers"
    assert np.array_equal(_bits(dist), _bits(ed)), f"{what}: distance bits"


@pytest.mark.parametrize("cell_table", [None, 0])
@pytest.mark.parametrize("name", ["A", "B", "D"])
def test_parity(gpu, name, cell_table):
    """Every k on every scene, with the auto cell table and none (the answers
    may not depend on it); the stats launch and the plain launch answer the same."""
    pr = cr.probes(name)
    ref = cr.expected(name)
    with _renderer(name, cell_table=cell_table) as r:
        for k in KS:
            exp = cr.cut(ref, k)
            dist, sphere, count, st = r.query_closest(pr, k, stats=True)
            _assert_answer((dist, sphere, count), exp, pr, k, f"{name} k={k} stats")
            assert (st.primary_rays, st.shadow_rays) == (0, 0) and st.ms > 0.0
            _assert_answer(r.query_closest(pr, k), exp, pr, k, f"{name} k={k}")


@pytest.mark.parametrize("name", ["one", "five", "E", "F", "G"])
def test_small_and_boundary_scenes(gpu, name):
    """The root-is-leaf scenes (1 and 5 spheres), scene E (exactly equal keys:
    ties go by index, and the duplicate of sphere 0 is reported beside it with
    the same distance), scene F (A moved 1000 units from the origin) and scene
    G (three pairs there that a box without the M term of its slack loses,
    overlap_ref._g_scene; its probes as they are and unbounded)."""
    sp = ov.spheres(name)
    pr = cr.probes(name)
    if name == "E":
        pr = np.concatenate([cr.with_cutoffs(ov.e_probes()[0]), pr])
    if name == "G":
        pr = np.concatenate([np.array(ov.g_probes()), cr.with_cutoffs(ov.g_probes()), pr])
    ref = cr.reference(sp, pr, 16)
    with _renderer(name) as r:
        info = r.scene_info()
        assert (info["n_nodes"] == 1) == (name in ("one", "five"))
        for k in (1, 3, 16):
            _assert_answer(r.query_closest(pr, k), cr.cut(ref, k), pr, k, f"{name} k={k}")
        dist, sphere, count = r.query_closest(pr, 16)
    assert ref[3].max() == len(sp) and (ref[3] == 0).sum() >= 64
    if name == "G":   # probe a's own sphere a is its nearest, and within its radius its only one
        assert [list(row[:2]) for row in sphere[:3]] == [[0, NO_HIT], [1, NO_HIT], [2, NO_HIT]]
        assert list(sphere[4]) == [1, 0, 2, 3] + [NO_HIT] * 12   # (row 4: g probe 1, unbounded)
    if name == "E":
        tie = (dist[:, 1:] == dist[:, :-1]) & (sphere[:, 1:] != NO_HIT)
        assert tie.any(axis=1).sum() >= 300 and np.all(sphere[:, 1:][tie] > sphere[:, :-1][tie])
        whole = ref[3] <= 16
        has0 = (sphere == 0).any(axis=1)
        assert (has0 & whole).sum() >= 4 and np.array_equal(has0[whole], (sphere == 18).any(axis=1)[whole])
        rows = np.flatnonzero(has0 & whole)
        at0, at18 = np.argmax(sphere[rows] == 0, axis=1), np.argmax(sphere[rows] == 18, axis=1)
        assert np.array_equal(_bits(dist[rows, at0]), _bits(dist[rows, at18]))


def test_odd_probes_among_ordinary_ones(gpu):
    """Between ordinary probes: a point so far away that d2 overflows (every key
    is +inf: unbounded it lists the k smallest indices at distance +inf, bounded
    nothing); a point far outside the root box, unbounded (the true nearest
    spheres); non-finite centres, a NaN and a negative radius (empty, every slot
    the radius as given); R = -0 (R = 0)."""
    sp = ov.spheres("D")
    nan = np.float32(np.nan)
    pr = cr.probes("D")[:320].copy()
    c = sp[0, :3]
    odd = {7: (1e20, 0.5, 0.5, INF), 8: (1e20, 0.5, 0.5, 1e30), 9: (-1e20, 1e20, 1e20, INF),
           64: (40.0, -25.0, 17.0, INF), 65: (-300.0, 0.5, 0.5, INF), 66: (0.5, 0.5, 3000.0, INF),
           100: (nan, 0.5, 0.5, INF), 101: (0.5, INF, 0.5, 0.1), 102: (0.5, 0.5, -INF, INF),
           128: (*c, nan), 129: (*c, -1e-6), 130: (*c, -INF), 131: (*c, -1.0),
           255: (*c, -0.0), 256: (*c, 0.0), 319: (*c, INF)}
    for i, p in odd.items():
        pr[i] = p
    ref = cr.reference(sp, pr, 16)
    ed, es, ec, total = ref
    assert list(es[7]) == list(range(16)) and np.all(np.isinf(ed[7])) and total[8] == 0
    assert list(es[9]) == list(range(16))
    assert all(total[i] == len(sp) and np.all(np.isfinite(ed[i])) for i in (64, 65, 66))
    assert all(total[i] == 0 for i in (100, 101, 102, 128, 129, 130, 131))
    assert total[255] == total[256] >= 1 and es[255, 0] == 0 and total[319] == len(sp)
    with _renderer("D") as r:
        for k in (1, 4, 16):
            got = r.query_closest(pr, k)
            _assert_answer(got, cr.cut(ref, k), pr, k, f"odd k={k}")
            dist, sphere, count = got
            assert np.all(sphere[[100, 101, 102, 128, 129, 130, 131]] == NO_HIT)
            assert np.all(np.signbit(dist[255, count[255]:]))   # a -0 radius comes back as -0


def test_stats(gpu):
    """On A: two stats launches count the same; the visited set nests (the
    children's order depends on the probe alone, so k = 1 with its smaller
    bound tests no more than k = 16, and a cutoff no more than none); an
    unbounded query tests far fewer than every reference."""
    pr = cr.probes("A").copy()
    pr[:, 3] = INF
    cut = pr.copy()
    cut[:, 3] = cr.CUTOFF
    with _renderer("A") as r:
        info = r.scene_info()
        a = r.query_closest(pr, 16, stats=True)[3]
        b = r.query_closest(pr, 16, stats=True)[3]
        one = r.query_closest(pr, 1, stats=True)[3]
        cut16 = r.query_closest(cut, 16, stats=True)[3]
        cut1 = r.query_closest(cut, 1, stats=True)[3]
    every = len(pr) * info["n_prim_refs"]
    print(f"closest stats on A, per probe: k=16 {a.prims_tested / len(pr):.1f} tests {a.nodes_visited / len(pr):.1f} "
          f"nodes; k=1 {one.prims_tested / len(pr):.1f} / {one.nodes_visited / len(pr):.1f}; "
          f"R=0.05 k=16 {cut16.prims_tested / len(pr):.1f}, k=1 {cut1.prims_tested / len(pr):.1f}; "
          f"every reference {info['n_prim_refs']}")
    assert (a.nodes_visited, a.prims_tested) == (b.nodes_visited, b.prims_tested)
    assert a.ms > 0.0 and b.ms > 0.0
    assert 0 < one.prims_tested <= a.prims_tested <= every and one.prims_tested < every
    assert 0 < one.nodes_visited <= a.nodes_visited <= len(pr) * info["n_nodes"]
    assert cut16.prims_tested <= a.prims_tested and cut1.prims_tested <= one.prims_tested
    assert cut16.nodes_visited <= a.nodes_visited and cut1.nodes_visited <= one.nodes_visited
    assert cut1.prims_tested <= cut16.prims_tested
    assert 16 * len(pr) <= a.prims_tested   # every answer was tested
    assert (a.primary_rays, a.shadow_rays, one.primary_rays, one.shadow_rays) == (0, 0, 0, 0)


def test_skip_self_with_the_scenes_own_device_spheres(gpu):
    """Each sphere's nearest neighbours: the device sphere list that made the
    scene is the probe list (its fourth column, the radius, is then the
    cutoff), with RT_CLOSEST_SKIP_SELF, on D at k = 16."""
    import torch
    sp = ov.spheres("D")
    n, k = len(sp), 16
    ed, es, ec, total = cr.reference(sp, sp, k, skip_self=True)
    assert (total >= 3).sum() > n // 2 and (total > k).sum() >= 1 and not np.any(es == np.arange(n)[:, None])
    with rt.KernelRenderer(CAM_W, CAM_H, mode="scene") as r:
        d_sp = torch.from_numpy(sp.copy()).cuda()
        d_near = torch.full((n, k, 2), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        d_cnt = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        r.set_scene_device(d_sp.data_ptr(), n, **ov.TREES["D"])
        r.query_closest_device(d_sp.data_ptr(), n, k, d_near.data_ptr(), d_cnt.data_ptr(), skip_self=True)
        r.synchronize()
        near = d_near.cpu().numpy()
        got = (np.ascontiguousarray(near[:, :, 0]).view(np.float32),
               np.ascontiguousarray(near[:, :, 1]).view(np.uint32), d_cnt.cpu().numpy().view(np.uint32))
        _assert_answer(got, (ed, es, ec), sp, k, "skip_self")
        # the host wrapper's flag, and without it every sphere reports itself first (key = -r)
        _assert_answer(r.query_closest(sp, k, skip_self=True), (ed, es, ec), sp, k, "skip_self (host)")
        plain = cr.reference(sp, sp, k)
        got = r.query_closest(sp, k)
        _assert_answer(got, plain[:3], sp, k, "with self")
        assert (got[1] == np.arange(n)[:, None]).any(axis=1).all()


def test_sizes_write_exactly_n_records(gpu):
    """n = 300 probes (no multiple of 256) write n*k records and n counts, the
    sentinel tail after each stays; dev_counts = NULL writes the same records."""
    import torch
    k = 3
    sp = ov.spheres("D")
    pr = cr.probes("D")[:300].copy()
    ed, es, ec, _ = cr.reference(sp, pr, k)
    n = len(pr)
    with _renderer("D") as r:
        d_pr = torch.from_numpy(pr).cuda()
        for with_counts in (True, False):
            d_near = torch.full((n * k + 5, 2), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
            d_cnt = torch.full((n + 5,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            r.query_closest_device(d_pr.data_ptr(), n, k, d_near.data_ptr(),
                                   d_cnt.data_ptr() if with_counts else None)
            r.synchronize()
            raw = d_near.cpu().numpy().view(np.uint32)
            assert np.all(raw[n * k:] == 0x5A5A5A5A)
            assert np.array_equal(raw[:n * k, 0].reshape(n, k), _bits(ed))
            assert np.array_equal(raw[:n * k, 1].reshape(n, k), es)
            words = d_cnt.cpu().numpy().view(np.uint32)
            if with_counts:
                assert np.all(words[n:] == 0x5A5A5A5A) and np.array_equal(words[:n], ec)
            else:
                assert np.all(words == 0x5A5A5A5A)


def test_closest_at_is_the_batch_calls_row(gpu):
    pr = cr.probes("D")
    rows = [0, 1, 2, 400, 401, 520, 700, 800, 900, 1000, 1001]   # contacts, points, small, large, far
    exp = cr.expected("D")
    with _renderer("D") as r:
        for k in (1, 4, 16):
            dist, sphere, count = r.query_closest(pr[rows], k)
            for m, i in enumerate(rows):
                c, d, s = r.closest_at(pr[i, :3], float(pr[i, 3]), k)
                assert c == int(count[m]), (k, i)
                assert np.array_equal(s, sphere[m]) and np.array_equal(_bits(d), _bits(dist[m])), (k, i)
        assert np.array_equal(sphere, exp[1][rows]) and (count == 16).any() and (count == 0).any()
        # a click that hits: the picked sphere is listed for the picked point, at distance ~ 0 (the
        # point o + t * d and the key are a dozen f32 roundings of values below 16: under 16 * 2^-20)
        hit, _, picked, point = r.pick(48.0, 32.0)
        assert hit
        c, d, s = r.closest_at(point, 0.05, 16)
        assert c >= 1 and picked in s[:c] and abs(float(d[list(s).index(picked)])) < 2e-5
        # count_out may be NULL
        lib = _lib.load()
        out = (_lib.RtNear * 16)()
        ctr = (ctypes.c_float * 3)(*[float(x) for x in pr[1, :3]])
        assert lib.rt_closest_at(r._h, ctr, float("inf"), 16, out, None) == _lib.RT_OK
        assert np.array_equal(np.array([o.sphere for o in out], np.uint32), exp[1][1])


def test_closest_queries_do_not_disturb_frames(gpu):
    """A progressive sequence of 3 frames with closest queries in between is
    byte-equal to the same frames without them, and a stats frame after them
    counts what it counts without them (accumulated samples included)."""
    pr = cr.probes("A")[:300]

    def queries(r):
        r.query_closest(pr, 4, stats=True)
        r.query_closest(pr, 16, skip_self=True)
        r.closest_at((0.6, 0.6, 0.6), float("inf"), 3)

    assert_frames_undisturbed(functools.partial(_renderer, "A"), queries)


def test_zero_probes_and_argument_errors(gpu):
    lib = _lib.load()
    with rt.KernelRenderer(64, 64, mode="scene") as r:
        with pytest.raises(_lib.RtError) as e:  # no scene yet
            r.query_closest(np.zeros((1, 4), np.float32), 2)
        assert e.value.code == _lib.RT_E_NOSCENE
        with pytest.raises(_lib.RtError) as e:
            r.closest_at((0.5, 0.5, 0.5), 0.1, 2)
        assert e.value.code == _lib.RT_E_NOSCENE
        r.set_scene(ov.spheres("A"), None)
        st = _lib.RtStats()
        st.nodes_visited = 5
        assert lib.rt_query_closest(r._h, None, 0, 3, 0, None, None, None, None) == _lib.RT_OK
        assert lib.rt_query_closest(r._h, None, 0, 3, 0, None, None, None, ctypes.byref(st)) == _lib.RT_OK
        assert (st.primary_rays, st.nodes_visited) == (0, 0)
        dist, sphere, count = r.query_closest(np.zeros((0, 4), np.float32), 3)
        assert dist.shape == (0, 3) and sphere.shape == (0, 3) and count.shape == (0,)
        fb = r.framebuffer_ptr()  # any valid device address: the call must refuse before using it
        for k in (0, 17, 0xFFFFFFFF):
            assert lib.rt_query_closest(r._h, fb, 1, k, 0, fb, None, None, None) == _lib.RT_E_INVALID
            assert lib.rt_query_closest(r._h, None, 0, k, 0, None, None, None, None) == _lib.RT_E_INVALID
        for flags in (2, 3, 0x80000000):
            assert lib.rt_query_closest(r._h, fb, 1, 2, flags, fb, None, None, None) == _lib.RT_E_INVALID
        assert lib.rt_query_closest(r._h, None, 1, 2, 0, fb, None, None, None) == _lib.RT_E_INVALID
        assert lib.rt_query_closest(r._h, fb, 1, 2, 0, None, None, None, None) == _lib.RT_E_INVALID
        out = (_lib.RtNear * 16)()
        c = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
        for k in (0, 17):
            assert lib.rt_closest_at(r._h, c, 0.1, k, out, None) == _lib.RT_E_INVALID
        assert lib.rt_closest_at(r._h, c, 0.1, 2, None, None) == _lib.RT_E_INVALID
        assert lib.rt_closest_at(r._h, None, 0.1, 2, out, None) == _lib.RT_E_INVALID


def test_multi_device_handle_answers_from_device_0(gpu):
    pr = cr.probes("D")[:600]
    exp = tuple(a[:600] for a in cr.cut(cr.expected("D"), 8))
    with _renderer("D", devices=[0, 0]) as r:
        r.render()
        dist, sphere, count, st = r.query_closest(pr, 8, stats=True)
        _assert_answer((dist, sphere, count), exp, pr, 8, "devices {0, 0}")
        with _renderer("D") as one:
            st1 = one.query_closest(pr, 8, stats=True)[3]
        assert (st.nodes_visited, st.prims_tested) == (st1.nodes_visited, st1.prims_tested)
