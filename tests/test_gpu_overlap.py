"""GPU sphere-overlap queries (rt_query_overlaps, rt_overlaps_at)
against the brute-force f32 reference of tests/overlap_ref.py: every index
slot, every filler, every count and every MORE bit, probe by probe.  The
reference runs once per scene at k = 16; a smaller k's answer is its first k
columns.
"""
import ctypes
import functools

import numpy as np
import pytest

import raytracingstudy_amd as rt
from raytracingstudy_amd import _lib

import overlap_ref as ov
from query_scaffold import CAM_H, CAM_W, assert_frames_undisturbed
from query_scaffold import scene_renderer as _renderer

pytestmark = pytest.mark.gpu

NO_HIT = ov.NO_HIT
KS = (1, 2, 3, 4, 8, 16)


def _assert_answer(got, exp, k, what=""):
    """got / exp: (indices (n, k), count (n,), more (n,)).  The direct
    assertions first, so that a failure says which property broke."""
    idx, count, more = got
    ei, ec, em = exp
    n = len(ei)
    assert idx.shape == (n, k) and count.shape == (n,) and more.shape == (n,), what
    assert count.max(initial=0) <= k, what
    held = np.arange(k)[None, :] < count[:, None]
    assert np.array_equal(idx != NO_HIT, held), f"{what}: hits fill the first `count` slots"
    both = held[:, 1:]
    # strictly ascending: in order, and no index twice
    assert np.all((idx[:, :-1] < idx[:, 1:])[both]), f"{what}: indices ascending, none twice"
    assert np.all(count[more] == k), f"{what}: MORE only with a full list"
    assert np.array_equal(count, ec), f"{what}: counts"
    assert np.array_equal(more, em), f"{what}: MORE bits"
    assert np.array_equal(idx, ei), f"{what}: sphere indices and fillers"


def test_dense_scene_lists_each_sphere_in_many_leaves(gpu):
    """D: many references per sphere, so the descent meets a sphere again and
    again and must count it once."""
    with _renderer("D") as r:
        info = r.scene_info()
    assert info["n_prim_refs"] > 10 * info["n_spheres"]


@pytest.mark.parametrize("cell_table", [None, 0])
@pytest.mark.parametrize("name", ["A", "B", "D"])
def test_parity(gpu, name, cell_table):
    """Every k on every scene, with the auto cell table and none (the answers
    may not depend on it); the stats launch and the plain launch answer the same."""
    pr = ov.probes(name)
    ref = ov.expected(name)
    with _renderer(name, cell_table=cell_table) as r:
        for k in KS:
            exp = ov.cut(ref, k)
            idx, count, more, st = r.query_overlaps(pr, k, stats=True)
            _assert_answer((idx, count, more), exp, k, f"{name} k={k} stats")
            assert (st.primary_rays, st.shadow_rays) == (0, 0) and st.ms > 0.0
            _assert_answer(r.query_overlaps(pr, k), exp, k, f"{name} k={k}")


@pytest.mark.parametrize("name", ["A", "D"])
def test_stats(gpu, name):
    """Two stats launches count the same; every member of every set was tested
    at least once, and no probe tests a leaf reference twice."""
    pr = ov.probes(name)
    total = ov.expected(name)[3]
    with _renderer(name) as r:
        info = r.scene_info()
        a = r.query_overlaps(pr, 16, stats=True)[3]
        b = r.query_overlaps(pr, 16, stats=True)[3]
        one = r.query_overlaps(pr, 1, stats=True)[3]
    assert (a.nodes_visited, a.prims_tested) == (b.nodes_visited, b.prims_tested)
    assert (one.nodes_visited, one.prims_tested) == (a.nodes_visited, a.prims_tested)  # k stops nothing
    assert a.ms > 0.0 and b.ms > 0.0
    assert int(total.sum()) <= a.prims_tested <= len(pr) * info["n_prim_refs"]
    assert 0 < a.nodes_visited <= len(pr) * info["n_nodes"]
    assert (a.primary_rays, a.shadow_rays, b.primary_rays, b.shadow_rays) == (0, 0, 0, 0)


def test_skip_self_with_the_scenes_own_device_spheres(gpu):
    """All contacts of the scene: the device sphere list that made the scene is
    the probe list, with RT_OVERLAP_SKIP_SELF, on D at k = 16."""
    import torch
    sp = ov.spheres("D")
    n, k = len(sp), 16
    ei, ec, em, total = ov.reference(sp, sp, k, skip_self=True)
    assert (total >= 3).sum() > n // 2 and em.sum() >= 1 and not np.any(ei == np.arange(n)[:, None])
    with rt.KernelRenderer(CAM_W, CAM_H, mode="scene") as r:
        d_sp = torch.from_numpy(sp.copy()).cuda()
        d_idx = torch.full((n, k), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        d_cnt = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        r.set_scene_device(d_sp.data_ptr(), n, **ov.TREES["D"])
        r.query_overlaps_device(d_sp.data_ptr(), n, k, d_idx.data_ptr(), d_cnt.data_ptr(), skip_self=True)
        r.synchronize()
        idx = d_idx.cpu().numpy().view(np.uint32)
        words = d_cnt.cpu().numpy().view(np.uint32)
        _assert_answer((idx, words & np.uint32(0x7FFFFFFF), (words & np.uint32(ov.MORE)) != 0),
                       (ei, ec, em), k, "skip_self")
        # the host wrapper's flag, and without it every sphere reports itself
        _assert_answer(r.query_overlaps(sp, k, skip_self=True), (ei, ec, em), k, "skip_self (host)")
        plain = ov.reference(sp, sp, k)
        _assert_answer(r.query_overlaps(sp, k), plain[:3], k, "with self")


@pytest.mark.parametrize("name", ["one", "five", "E", "F", "G"])
def test_small_and_boundary_scenes(gpu, name):
    """The root-is-leaf scenes (1 and 5 spheres), scene E, scene F (A moved
    1000 units from the origin) and scene G (three pairs there that a box
    without the M term of its slack loses, overlap_ref._g_scene): the probe mix, and for E the exactly tangent pairs, their one-ulp-out twins
    and the duplicate."""
    sp = ov.spheres(name)
    pr = ov.probes(name)
    cases = []
    if name == "E":
        eb, cases = ov.e_probes()
        pr = np.concatenate([eb, pr])
    if name == "G":
        pr = np.concatenate([ov.g_probes(), pr])
    ref = ov.reference(sp, pr, 16)
    with _renderer(name) as r:
        info = r.scene_info()
        assert (info["n_nodes"] == 1) == (name in ("one", "five"))
        for k in (1, 3, 16):
            _assert_answer(r.query_overlaps(pr, k), ov.cut(ref, k), k, f"{name} k={k}")
        idx = r.query_overlaps(pr, 16)[0]
    assert ref[3].max() >= min(len(sp), 2) and (ref[3] == 0).sum() >= 64
    for p, j, yes in cases:
        assert (j in idx[p]) == yes, (p, j, yes)
    if name == "G":
        assert [list(row[:2]) for row in idx[:3]] == [[0, NO_HIT], [1, NO_HIT], [2, NO_HIT]]
    if name == "E":   # a probe that touches sphere 0 reports its duplicate 18 too (where 16 slots hold the set)
        whole = ref[3] <= 16
        has0 = (idx == 0).any(axis=1)[whole]
        assert has0.sum() >= 4 and np.array_equal(has0, (idx == 18).any(axis=1)[whole])


def test_bad_probes_are_empty_and_sizes_write_exactly_n_records(gpu):
    """Non-finite and negative-radius probes between ordinary ones: empty, and
    the neighbours' slots intact; n = 300 probes (no multiple of 256) write
    n*k indices and n counts, the sentinel tail after each stays; dev_counts =
    NULL writes the same indices."""
    import torch
    k = 3
    sp = ov.spheres("D")
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    pr = ov.probes("D")[:300].copy()
    good = sp[0].copy()   # touches 4 spheres, itself included
    bad = {10: (nan, 0.5, 0.5, 0.1), 11: (0.5, inf, 0.5, 0.1), 12: (0.5, 0.5, -inf, 0.1),
           64: (*good[:3], -1e-6), 65: (*good[:3], nan), 127: (*good[:3], inf), 255: (*good[:3], -inf),
           256: (nan, nan, nan, nan), 299: (*good[:3], -1.0)}
    for i, p in bad.items():
        pr[i] = p
    pr[63], pr[66] = good, (*good[:3], -0.0)      # ordinary neighbours (R = -0 is R = 0)
    ei, ec, em, total = ov.reference(sp, pr, k)
    assert all(total[i] == 0 for i in bad) and total[63] >= 3 and total[66] >= 1
    n = len(pr)
    with _renderer("D") as r:
        d_pr = torch.from_numpy(pr).cuda()
        for with_counts in (True, False):
            d_idx = torch.full((n * k + 5,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
            d_cnt = torch.full((n + 5,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            r.query_overlaps_device(d_pr.data_ptr(), n, k, d_idx.data_ptr(),
                                    d_cnt.data_ptr() if with_counts else None)
            r.synchronize()
            raw = d_idx.cpu().numpy().view(np.uint32)
            assert np.all(raw[n * k:] == 0x5A5A5A5A)
            idx = raw[:n * k].reshape(n, k)
            assert np.array_equal(idx, ei)
            for i in bad:
                assert np.all(idx[i] == NO_HIT), i
            words = d_cnt.cpu().numpy().view(np.uint32)
            if with_counts:
                assert np.all(words[n:] == 0x5A5A5A5A)
                assert np.array_equal(words[:n] & np.uint32(0x7FFFFFFF), ec)
                assert np.array_equal((words[:n] & np.uint32(ov.MORE)) != 0, em)
                assert all(words[i] == 0 for i in bad)
            else:
                assert np.all(words == 0x5A5A5A5A)


def test_overlaps_at_is_the_batch_calls_row(gpu):
    pr = ov.probes("D")
    rows = [0, 5, 400, 520, 700, 800, 900, 1000]   # contacts, points, small, large, far
    with _renderer("D") as r:
        for k in (1, 4, 16):
            idx, count, more = r.query_overlaps(pr[rows], k)
            for m, i in enumerate(rows):
                c, one, mo = r.overlaps_at(pr[i, :3], float(pr[i, 3]), k)
                assert (c, mo) == (int(count[m]), bool(more[m])), (k, i)
                assert np.array_equal(one, idx[m]), (k, i)
        exp = ov.cut(ov.expected("D"), 16)
        assert np.array_equal(idx, exp[0][rows]) and more.any() and (count == 0).any()
        # a brush around the point under the mouse: it holds the picked sphere
        hit, _, sphere, point = r.pick(48.0, 32.0)
        assert hit
        c, one, _ = r.overlaps_at(point, 0.05, 16)
        assert sphere in one[:c]
        # count_out may be NULL
        lib = _lib.load()
        out = (ctypes.c_uint32 * 16)()
        ctr = (ctypes.c_float * 3)(*[float(x) for x in pr[0, :3]])
        assert lib.rt_overlaps_at(r._h, ctr, float(pr[0, 3]), 16, out, None) == _lib.RT_OK
        assert np.array_equal(np.array(list(out), np.uint32), exp[0][0])


def test_overlap_queries_do_not_disturb_frames(gpu):
    """A progressive sequence of 3 frames with overlap queries in between is
    byte-equal to the same frames without them, and a stats frame after them
    counts what it counts without them (accumulated samples included)."""
    pr = ov.probes("A")[:300]

    def queries(r):
        r.query_overlaps(pr, 4, stats=True)
        r.query_overlaps(pr, 16, skip_self=True)
        r.overlaps_at((0.6, 0.6, 0.6), 0.1, 3)

    assert_frames_undisturbed(functools.partial(_renderer, "A"), queries)


def test_zero_probes_and_argument_errors(gpu):
    lib = _lib.load()
    with rt.KernelRenderer(64, 64, mode="scene") as r:
        with pytest.raises(_lib.RtError) as e:  # no scene yet
            r.query_overlaps(np.zeros((1, 4), np.float32), 2)
        assert e.value.code == _lib.RT_E_NOSCENE
        with pytest.raises(_lib.RtError) as e:
            r.overlaps_at((0.5, 0.5, 0.5), 0.1, 2)
        assert e.value.code == _lib.RT_E_NOSCENE
        r.set_scene(ov.spheres("A"), None)
        st = _lib.RtStats()
        st.nodes_visited = 5
        assert lib.rt_query_overlaps(r._h, None, 0, 3, 0, None, None, None, None) == _lib.RT_OK
        assert lib.rt_query_overlaps(r._h, None, 0, 3, 0, None, None, None, ctypes.byref(st)) == _lib.RT_OK
        assert (st.primary_rays, st.nodes_visited) == (0, 0)
        idx, count, more = r.query_overlaps(np.zeros((0, 4), np.float32), 3)
        assert idx.shape == (0, 3) and count.shape == (0,) and more.shape == (0,)
        fb = r.framebuffer_ptr()  # any valid device address: the call must refuse before using it
        for k in (0, 17, 0xFFFFFFFF):
            assert lib.rt_query_overlaps(r._h, fb, 1, k, 0, fb, None, None, None) == _lib.RT_E_INVALID
            assert lib.rt_query_overlaps(r._h, None, 0, k, 0, None, None, None, None) == _lib.RT_E_INVALID
        for flags in (2, 3, 0x80000000):
            assert lib.rt_query_overlaps(r._h, fb, 1, 2, flags, fb, None, None, None) == _lib.RT_E_INVALID
        assert lib.rt_query_overlaps(r._h, None, 1, 2, 0, fb, None, None, None) == _lib.RT_E_INVALID
        assert lib.rt_query_overlaps(r._h, fb, 1, 2, 0, None, None, None, None) == _lib.RT_E_INVALID
        out = (ctypes.c_uint32 * 16)()
        c = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
        for k in (0, 17):
            assert lib.rt_overlaps_at(r._h, c, 0.1, k, out, None) == _lib.RT_E_INVALID
        assert lib.rt_overlaps_at(r._h, c, 0.1, 2, None, None) == _lib.RT_E_INVALID
        assert lib.rt_overlaps_at(r._h, None, 0.1, 2, out, None) == _lib.RT_E_INVALID


def test_multi_device_handle_answers_from_device_0(gpu):
    pr = ov.probes("D")[:600]
    exp = tuple(a[:600] for a in ov.cut(ov.expected("D"), 8))
    with _renderer("D", devices=[0, 0]) as r:
        r.render()
        idx, count, more, st = r.query_overlaps(pr, 8, stats=True)
        _assert_answer((idx, count, more), exp, 8, "devices {0, 0}")
        with _renderer("D") as one:
            st1 = one.query_overlaps(pr, 8, stats=True)[3]
        assert (st.nodes_visited, st.prims_tested) == (st1.nodes_visited, st1.prims_tested)
