"""GPU swept-sphere queries (rt_sweep_spheres, rt_sweep_at, rt_pick_thick;
DESIGN.md 5.14) against the brute-force reference of tests/sweep_ref.py: every
t bit and every sphere index, cast by cast, no case left out of a comparison.
"""
import ctypes
import functools

import numpy as np
import pytest

import raytracingstudy_amd as rt
from raytracingstudy_amd import _lib

import overlap_ref as ov
import sweep_ref as sr
from query_scaffold import CAM_H, CAM_W, assert_frames_undisturbed
from query_scaffold import bits as _bits
from query_scaffold import scene_renderer as _renderer
from test_sweep_cpu import odd_casts

pytestmark = pytest.mark.gpu

NO_HIT = sr.NO_HIT
FLAGS = [dict(entry_only=e, skip_self=s) for e in (False, True) for s in (False, True)]


def _flag_bits(entry_only=False, skip_self=False):
    return (sr.ENTRY_ONLY if entry_only else 0) | (sr.SKIP_SELF if skip_self else 0)


def _assert_answer(got, exp, what=""):
    t, sphere = got[0], got[1]
    et, es = exp
    assert t.shape == et.shape and sphere.shape == es.shape, what
    assert np.array_equal(sphere, es), f"{what}: sphere indices"
    assert np.array_equal(_bits(t), _bits(et)), f"{what}: t bits"


def _check_scene(r, name):
    """Both flags with per-cast radii, stats launches and plain ones; a uniform
    radius against the same radii as an array."""
    sp = ov.spheres(name)
    rays, radii = sr.casts(name)
    for kw in FLAGS:
        exp = sr.expected(name, _flag_bits(**kw))
        t, sphere, st = r.sweep_spheres(rays, radii, stats=True, **kw)
        _assert_answer((t, sphere), exp, f"{name} {kw} stats")
        assert (st.primary_rays, st.shadow_rays) == (len(rays), 0) and st.ms > 0.0
        _assert_answer(r.sweep_spheres(rays, radii, **kw), exp, f"{name} {kw}")
    exp = sr.reference(sp, rays, 0.05)
    _assert_answer(r.sweep_spheres(rays, 0.05), exp, f"{name} uniform")
    _assert_answer(r.sweep_spheres(rays, np.full(len(rays), 0.05, np.float32)), exp, f"{name} uniform as an array")


@pytest.mark.parametrize("cell_table", [None, 0])
@pytest.mark.parametrize("name", ["A", "B", "D"])
def test_parity(gpu, name, cell_table):
    """With the auto cell table and none: the answers may not depend on it."""
    with _renderer(name, cell_table=cell_table) as r:
        _check_scene(r, name)


@pytest.mark.parametrize("name", ["one", "five", "E", "F", "G"])
def test_small_and_boundary_scenes(gpu, name):
    """The root-is-leaf scenes, scene E (exact ties in t go to the smaller
    index: sphere 18 is sphere 0 again), F (A moved 1000 units from the origin)
    and G (tops 1e-5 below a cell face there, casts from 1280 units above)."""
    with _renderer(name) as r:
        info = r.scene_info()
        assert (info["n_nodes"] == 1) == (name in ("one", "five"))
        _check_scene(r, name)
    if name == "E":
        sphere = sr.expected("E")[1]
        assert (sphere == 0).sum() >= 1 and not (sphere == 18).any()


@pytest.mark.parametrize("name", ["A", "B"])
def test_radius_zero_is_trace_rays_nearest(gpu, name):
    rays, radii = sr.casts(name)
    assert sr.cast_ok(rays, radii).all()
    with _renderer(name) as r:
        t, sphere = r.sweep_spheres(rays, 0.0)
        tt, ts = r.trace_rays(rays, "nearest")
    assert np.array_equal(sphere, ts) and np.array_equal(_bits(t), _bits(tt))
    assert (sphere != NO_HIT).sum() >= 300


def test_odd_casts_among_ordinary_ones(gpu):
    """In one launch, between ordinary casts: non-finite origins, directions,
    windows and radii, negative radii and -0, zero and non-unit directions,
    tmax <= tmin, a cast from far outside the root box pointing away.  All as
    the reference has them, and the neighbours as in a launch without them."""
    sp = ov.spheres("D")
    rays, radii = (np.array(a[:400]) for a in sr.casts("D"))
    orays, oradii, valid = odd_casts(sp)
    at = 7 + 9 * np.arange(len(orays))
    assert at.max() < 400
    plain = sr.reference(sp, rays, radii)
    rays[at], radii[at] = orays, oradii
    exp = sr.reference(sp, rays, radii)
    rest = np.ones(400, bool)
    rest[at] = False
    assert np.array_equal(exp[1][rest], plain[1][rest]) and np.all(exp[1][at][~valid] == NO_HIT)
    with _renderer("D") as r:
        for kw in (dict(), dict(entry_only=True)):
            exp = sr.reference(sp, rays, radii, _flag_bits(**kw))
            t, sphere, st = r.sweep_spheres(rays, radii, stats=True, **kw)
            _assert_answer((t, sphere), exp, f"odd {kw} stats")
            _assert_answer(r.sweep_spheres(rays, radii, **kw), exp, f"odd {kw}")
            assert np.all(sphere[at][~valid] == NO_HIT)
            assert np.array_equal(_bits(t[at][~valid]), _bits(orays[~valid, 7]))   # a miss: tmax as given
        # alone, the invalid casts read nothing
        st = r.sweep_spheres(orays[~valid], oradii[~valid], stats=True)[2]
        assert (st.nodes_visited, st.prims_tested) == (0, 0)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 257, 1000])
def test_sizes_write_exactly_n_records(gpu, n):
    import torch
    sp = ov.spheres("D")
    rays, radii = (np.array(a[:n]) for a in sr.casts("D"))
    et, es = sr.reference(sp, rays, radii)
    with _renderer("D") as r:
        d_rays = torch.from_numpy(rays).cuda()
        d_radii = torch.from_numpy(radii).cuda()
        for with_radii in (True, False):
            d_hits = torch.full((n + 5, 2), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            r.sweep_spheres_device(d_rays.data_ptr(), n, d_hits.data_ptr(), 0.05,
                                   d_radii.data_ptr() if with_radii else None)
            r.synchronize()
            raw = d_hits.cpu().numpy().view(np.uint32)
            assert np.all(raw[n:] == 0x5A5A5A5A)
            if not with_radii:
                et, es = sr.reference(sp, rays, 0.05)
            assert np.array_equal(raw[:n, 0], _bits(et)) and np.array_equal(raw[:n, 1], es)


def test_single_item_calls_are_the_batch_calls_rows(gpu, oracle):
    rays, radii = sr.casts("D")
    rows = [i for i in (400, 500, 600, 700, 780, 810, 850, 900, 960, 1000, 1023) if rays[i, 3] == 0.0]
    assert len(rows) >= 8
    with _renderer("D") as r:
        for entry in (False, True):
            t, sphere = r.sweep_spheres(rays[rows], radii[rows], entry_only=entry)
            for m, i in enumerate(rows):
                hit, th, s, point = r.sweep_at(rays[i, :3], rays[i, 4:7], float(radii[i]), float(rays[i, 7]),
                                               entry_only=entry)
                assert (hit, s) == (sphere[m] != NO_HIT, sphere[m]), (entry, i)
                assert _bits(np.float32(th)) == _bits(t[m:m + 1])[0], (entry, i)
                if hit:
                    assert np.array_equal(point, rays[i, :3] + np.float32(th) * rays[i, 4:7])
        assert (sphere != NO_HIT).any() and (sphere == NO_HIT).any()
        # a finite tmax that ends the cast before its contact
        i = rows[int(np.flatnonzero(sphere != NO_HIT)[0])]
        assert not r.sweep_at(rays[i, :3], rays[i, 4:7], float(radii[i]), float(t[rows.index(i)]) * 0.5,
                              entry_only=True)[0]
        # pick_thick: rt_pick's ray as a one-cast sweep
        pose, K = r.camera()
        hits = 0
        for u, v in ((48.0, 32.0), (10.5, 20.25), (95.0, 0.0), (0.0, 63.0), (70.0, 50.0)):
            ray = np.zeros((1, 8), np.float32)
            ray[0, :3] = pose.reshape(-1)[12:15]
            ray[0, 4:7] = oracle.get_ray(pose, K, u, v)
            ray[0, 7] = np.inf
            for R in (0.0, 0.01, 0.1):
                t, sphere = r.sweep_spheres(ray, R)
                hit, th, s, point = r.pick_thick(u, v, R)
                assert (hit, s, _bits(np.float32(th))) == (sphere[0] != NO_HIT, sphere[0], _bits(t)[0]), (u, v, R)
                hits += hit
            ph, pt, ps, ppoint = r.pick(u, v)
            hit, th, s, point = r.pick_thick(u, v, 0.0)
            assert (hit, s, _bits(np.float32(th))) == (ph, ps, _bits(np.float32(pt))) and np.array_equal(point, ppoint)
        assert hits >= 3
        # point_out may be NULL
        lib = _lib.load()
        h = _lib.RtHit()
        assert lib.rt_pick_thick(r._h, 48.0, 32.0, 0.01, ctypes.byref(h), None) == _lib.RT_OK
        assert h.sphere == r.pick_thick(48.0, 32.0, 0.01)[2]


def test_skip_self_with_the_scenes_own_centres_and_radii(gpu):
    """Each sphere's first impact of a step: the scene's centres as origins, its
    radii as R, random unit velocities, a step of 0.3, RT_SWEEP_SKIP_SELF."""
    sp = ov.spheres("D")
    n = len(sp)
    g = np.random.default_rng(31)
    rays = np.zeros((n, 8), np.float32)
    rays[:, :3] = sp[:, :3]
    rays[:, 4:7] = sr.normalise_f32(g.normal(size=(n, 3)).astype(np.float32))
    rays[:, 7] = 0.3
    radii = np.array(sp[:, 3])
    with _renderer("D") as r:
        for entry in (False, True):
            flags = sr.SKIP_SELF | (sr.ENTRY_ONLY if entry else 0)
            exp = sr.reference(sp, rays, radii, flags)
            assert not np.any(exp[1] == np.arange(n)) and (exp[1] != NO_HIT).sum() > n // 2
            _assert_answer(r.sweep_spheres(rays, radii, entry_only=entry, skip_self=True), exp, f"skip_self {entry}")
        # without the flag a sphere can touch itself first (the far root of its own doubled sphere,
        # where D's dense cloud leaves that long a step free)
        t, sphere = r.sweep_spheres(rays, radii)
        _assert_answer((t, sphere), sr.reference(sp, rays, radii), "with self")
        assert (sphere == np.arange(n)).sum() >= 8


def test_sweeps_do_not_disturb_frames(gpu):
    rays, radii = (a[:300] for a in sr.casts("A"))

    def queries(r):
        r.sweep_spheres(rays, radii, stats=True)
        r.sweep_spheres(rays, 0.02, entry_only=True, skip_self=True)
        r.sweep_at((0.6, 0.6, -1.0), (0.0, 0.0, 1.0), 0.05)
        r.pick_thick(40.0, 30.0, 0.02)

    assert_frames_undisturbed(functools.partial(_renderer, "A"), queries)


def test_a_callers_stream(gpu):
    import torch
    rays, radii = (np.array(a[:600]) for a in sr.casts("D"))
    exp = tuple(a[:600] for a in sr.expected("D"))
    with _renderer("D") as r:
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            d_rays = torch.from_numpy(rays).cuda()
            d_radii = torch.from_numpy(radii).cuda()
            d_hits = torch.full((600, 2), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
            assert r.sweep_spheres_device(d_rays.data_ptr(), 600, d_hits.data_ptr(), 0.0, d_radii.data_ptr(),
                                          stream=s.cuda_stream) is None
            raw = d_hits.cpu().numpy().view(np.uint32)   # on s: ordered after the launch
        s.synchronize()
        r.synchronize()
    assert np.array_equal(raw[:, 1], exp[1]) and np.array_equal(raw[:, 0], _bits(exp[0]))


def test_zero_casts_and_argument_errors(gpu):
    lib = _lib.load()
    with rt.KernelRenderer(64, 64, mode="scene") as r:
        with pytest.raises(_lib.RtError) as e:  # no scene yet
            r.sweep_spheres(np.zeros((1, 8), np.float32), 0.1)
        assert e.value.code == _lib.RT_E_NOSCENE
        with pytest.raises(_lib.RtError) as e:
            r.sweep_at((0.5, 0.5, 0.5), (1.0, 0.0, 0.0), 0.1)
        assert e.value.code == _lib.RT_E_NOSCENE
        with pytest.raises(_lib.RtError) as e:
            r.pick_thick(1.0, 1.0, 0.1)
        assert e.value.code == _lib.RT_E_NOSCENE
        r.set_scene(ov.spheres("A"), None)
        st = _lib.RtStats()
        st.nodes_visited = 5
        assert lib.rt_sweep_spheres(r._h, None, None, 0.1, 0, 0, None, None, None) == _lib.RT_OK
        assert lib.rt_sweep_spheres(r._h, None, None, 0.1, 0, 3, None, None, ctypes.byref(st)) == _lib.RT_OK
        assert (st.primary_rays, st.nodes_visited) == (0, 0)
        t, sphere = r.sweep_spheres(np.zeros((0, 8), np.float32), 0.1)
        assert t.shape == (0,) and sphere.shape == (0,)
        t, sphere = r.sweep_spheres(np.zeros((0, 8), np.float32), np.zeros(0, np.float32))
        assert t.shape == (0,) and sphere.shape == (0,)
        with pytest.raises(ValueError):
            r.sweep_spheres(np.zeros((2, 8), np.float32), np.zeros(3, np.float32))
        fb = r.framebuffer_ptr()  # any valid device address: the call must refuse before using it
        for flags in (4, 7, 0x80000000):
            assert lib.rt_sweep_spheres(r._h, fb, None, 0.1, 1, flags, fb, None, None) == _lib.RT_E_INVALID
            assert lib.rt_sweep_spheres(r._h, None, None, 0.1, 0, flags, None, None, None) == _lib.RT_E_INVALID
        assert lib.rt_sweep_spheres(r._h, None, None, 0.1, 1, 0, fb, None, None) == _lib.RT_E_INVALID
        assert lib.rt_sweep_spheres(r._h, fb, None, 0.1, 1, 0, None, None, None) == _lib.RT_E_INVALID
        h = _lib.RtHit()
        o = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
        d = (ctypes.c_float * 3)(1.0, 0.0, 0.0)
        assert lib.rt_sweep_at(r._h, o, d, 0.1, 1.0, 4, ctypes.byref(h), None) == _lib.RT_E_INVALID
        assert lib.rt_sweep_at(r._h, None, d, 0.1, 1.0, 0, ctypes.byref(h), None) == _lib.RT_E_INVALID
        assert lib.rt_sweep_at(r._h, o, None, 0.1, 1.0, 0, ctypes.byref(h), None) == _lib.RT_E_INVALID
        assert lib.rt_sweep_at(r._h, o, d, 0.1, 1.0, 0, None, None) == _lib.RT_E_INVALID
        assert lib.rt_pick_thick(r._h, 1.0, 1.0, 0.1, None, None) == _lib.RT_E_INVALID


def test_multi_device_handle_answers_from_device_0(gpu):
    rays, radii = (a[:600] for a in sr.casts("D"))
    exp = tuple(a[:600] for a in sr.expected("D"))
    with _renderer("D", devices=[0, 0]) as r:
        r.render()
        t, sphere, st = r.sweep_spheres(rays, radii, stats=True)
        _assert_answer((t, sphere), exp, "devices {0, 0}")
        with _renderer("D") as one:
            st1 = one.sweep_spheres(rays, radii, stats=True)[2]
        assert (st.nodes_visited, st.prims_tested) == (st1.nodes_visited, st1.prims_tested)


def test_stats(gpu):
    """On A: two stats launches count the same; a shorter tmax reads no more
    node records and tests no more spheres than a longer one on the same casts
    (the children's order depends on the direction alone and the bound only
    prunes); far fewer tests than every reference."""
    rays, radii = (np.array(a) for a in sr.casts("A"))
    rays[:, 3] = 0.0
    rays[:, 7] = np.inf
    short = rays.copy()
    short[:, 7] = 0.25
    with _renderer("A") as r:
        info = r.scene_info()
        a = r.sweep_spheres(rays, radii, stats=True)[2]
        b = r.sweep_spheres(rays, radii, stats=True)[2]
        c = r.sweep_spheres(short, radii, stats=True)[2]
    n = len(rays)
    print(f"sweep stats on A, per cast: {a.prims_tested / n:.1f} tests {a.nodes_visited / n:.1f} nodes; "
          f"tmax 0.25: {c.prims_tested / n:.1f} / {c.nodes_visited / n:.1f}; every reference {info['n_prim_refs']}")
    assert (a.nodes_visited, a.prims_tested) == (b.nodes_visited, b.prims_tested) and a.ms > 0.0 and b.ms > 0.0
    assert 0 < c.nodes_visited <= a.nodes_visited <= n * info["n_nodes"]
    assert 0 < c.prims_tested <= a.prims_tested < n * info["n_prim_refs"] // 4
    assert (a.primary_rays, a.shadow_rays) == (n, 0)


def test_the_slab_guide_follows_the_line(gpu):
    """Scene L (sweep_ref.l_scene): one oblique cast with R = 0 across a sheet
    of 256 depth-4 leaves, which it misses.  A line crosses at most 2^d +
    2^(d-1) + 1 cells of depth d: 50 records for depths 0 to 4; a descent
    guided by the segment's bounding box reads at least 128 depth-4 records."""
    sp, ray, R = sr.l_scene()
    assert sr.reference(sp, ray, R)[1][0] == NO_HIT
    with rt.KernelRenderer(CAM_W, CAM_H, mode="scene") as r:
        info = r.set_scene(sp, None, **sr.L_TREE)
        assert info["n_leaves"] == 256
        t, sphere, st = r.sweep_spheres(ray, R, stats=True)
    print("scene L: nodes_visited", st.nodes_visited, "prims_tested", st.prims_tested)
    assert sphere[0] == NO_HIT and np.isinf(t[0])
    assert 0 < st.nodes_visited <= 64
