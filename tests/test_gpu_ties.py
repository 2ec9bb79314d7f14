"""Exact ties on the GPU ("ties go to the smaller sphere index,
so the result does not depend on traversal order").  The rule is implemented
twice, in the walk (csrc/rt_walk.h, the th == best_t branch) and in the bins'
lists (csrc/rt_bins.h, the bin list and the wide list); the queries and the
G-buffer inherit the walk's.  tie_scenes.py's scenes (test_ties_cpu.py shows
that they tie, and that the reversed rule would change 100+ pixels) against
the oracle byte for byte and id for id, on every path that resolves a tie.
"""
import functools

import numpy as np
import pytest

import raytracingstudy_amd as rt

import tie_scenes as ts

pytestmark = pytest.mark.gpu

NO_HIT = 0xFFFFFFFF


@functools.lru_cache(maxsize=None)
def _scene(name):
    return ts.tangent_pairs() if name == "T" else ts.SCENES[name]()


@functools.lru_cache(maxsize=None)
def _oracle_scene(name):
    import oracle
    sc = _scene(name)
    return oracle.Scene(sc["sp"], sc["al"], **(ts.T_TREE if name == "T" else {}))


@functools.lru_cache(maxsize=None)
def _first_hits(name):
    """The oracle's first hit of every pixel-centre ray: t (H, W) f32 (a miss:
    +inf) and sphere (H, W) u32."""
    import oracle
    s, P, K = _oracle_scene(name), ts.pose(), ts.intrinsic()
    t = np.full((ts.H, ts.W), np.inf, np.float32)
    sphere = np.full((ts.H, ts.W), NO_HIT, np.uint32)
    for y in range(ts.H):
        for x in range(ts.W):
            hit, th, j, _ = s.trace(P[3, :3], oracle.get_ray(P, K, float(x), float(y)))
            if hit:
                t[y, x], sphere[y, x] = th, j
    t.setflags(write=False)
    sphere.setflags(write=False)
    return t, sphere


@functools.lru_cache(maxsize=None)
def _oracle_frame(name, spp):
    return _oracle_scene(name).render(ts.W, ts.H, ts.pose(), ts.intrinsic(), spp=spp, jitter=False)


def _renderer(name, spp=1, **kw):
    sc = _scene(name)
    r = rt.KernelRenderer(ts.W, ts.H, mode="scene", spp=spp, radiance=True, jitter=False, **kw)
    r.resize(ts.W, ts.H)
    r.setIntrinsic(ts.intrinsic())
    r.setPosition(ts.pose())
    r.set_scene(sc["sp"], sc["al"], **(ts.T_TREE if name == "T" else {}))
    return r


@pytest.fixture
def hooks(monkeypatch):
    """Bins at this frame size and list length (test_gpu_bins' hooks)."""
    monkeypatch.setenv("RT_TEST_BIN_MIN_SAMPLES", "0")
    monkeypatch.setenv("RT_TEST_BIN_MEAN", "1000000")


@pytest.mark.parametrize("spp", ts.SPPS)
@pytest.mark.parametrize("name", ["D", "M"])
def test_frames(gpu, oracle, hooks, name, spp):
    """The plain frame from bins and occluder lists, the plain frame without
    bins (the walk's counter-free instance) and the stats frame: each the
    oracle's bytes, at one round, whole waves and sorted rounds."""
    ref8, ref32, cnt = _oracle_frame(name, spp)
    with _renderer(name, spp) as r:
        r.render()
        bi = r.bin_info()
        assert bi["reason"] == "on" and bi["entries"] > 0, bi
        assert r.scene_info()["occluder_lists_on"] == 1
        assert np.array_equal(r.readback(), ref8), "bins: RGBA8"
        assert np.array_equal(r.readback_radiance(), ref32), "bins: radiance"
        st = r.render(stats=True)
        assert np.array_equal(r.readback(), ref8), "stats frame: RGBA8"
        assert np.array_equal(r.readback_radiance(), ref32), "stats frame: radiance"
        assert (st.primary_rays, st.shadow_rays, st.nodes_visited, st.prims_tested) == tuple(
            int(c) for c in cnt)
    with _renderer(name, spp, bins=False) as r:
        r.render()
        assert r.bin_info()["reason"] == "flag"
        assert np.array_equal(r.readback(), ref8), "bins=False: RGBA8"
        assert np.array_equal(r.readback_radiance(), ref32), "bins=False: radiance"


@pytest.mark.parametrize("name", ["D", "M"])
def test_gbuffer_and_pick(gpu, oracle, name):
    """rt_render_gbuffer's t, ids and albedo, and rt_pick at the tie pixels."""
    sc = _scene(name)
    t, sphere = _first_hits(name)
    hit = sphere != NO_HIT
    with _renderer(name) as r:
        gb = r.render_gbuffer()
        assert np.array_equal(gb["sphere"], sphere)
        assert np.array_equal(gb["t"].view(np.uint32), t.view(np.uint32))
        assert np.array_equal(gb["albedo"][hit], sc["al"][sphere[hit]])
        picked = 0
        px = {p for pair in ts.tie_pixels(sc) for p in pair}
        for x, y in sorted(px):
            if not hit[y, x]:
                continue
            h, tp, j, _ = r.pick(float(x), float(y))
            assert h and j == sphere[y, x] and np.float32(tp) == t[y, x], (x, y)
            picked += 1
    assert picked >= 100


def test_trace_rays_tangent_pairs(gpu, oracle):
    """rt_trace_rays over T: nearest names the lower index at the tie's t;
    any-hit reports the hit and the same t (both spheres give it; which one
    an any-hit walk names is its traversal's business)."""
    sc = _scene("T")
    s, rays = _oracle_scene("T"), sc["rays"]
    exp = [s.trace(q[0:3], q[4:7], q[3], q[7]) for q in rays]
    assert all(e[0] for e in exp)
    et = np.array([e[1] for e in exp], np.float32)
    ej = np.array([e[2] for e in exp], np.uint32)
    assert np.array_equal(ej, sc["pairs"].min(1)) and np.array_equal(et, sc["t"])
    with _renderer("T") as r:
        t, sphere = r.trace_rays(rays, "nearest")
        assert np.array_equal(sphere, ej)
        assert np.array_equal(t.view(np.uint32), et.view(np.uint32))
        t, sphere = r.trace_rays(rays, "any")
        assert np.all(sphere != NO_HIT)
        assert np.array_equal(t.view(np.uint32), et.view(np.uint32))
        assert np.all((sphere == sc["pairs"][:, 0]) | (sphere == sc["pairs"][:, 1]))
