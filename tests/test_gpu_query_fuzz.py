"""Every query entry point on every query_fuzz.py case against the references:
rt_trace_rays (nearest / any), rt_trace_rays_multi, rt_query_overlaps,
rt_render_gbuffer and the host one-shots rt_pick, rt_pick_multi and
rt_overlaps_at.  The other query tests run the
generator's cloud and hand-made lattices; these 64 scenes have a grown,
non-cubic root box, radii over three decades, leaf capacities 1..16, depths
1..8 and the plain fuzz's cameras and intrinsics.

Per seed, one renderer with the case's tree and a cell table picked by the
seed (auto, none, a fixed depth), and query_fuzz.model's expectations: the
oracle's walk for nearest / any (t bits, sphere, summed counters), the brute
force of multihit_ref and overlap_ref for the lists, the oracle per pixel for
the G-buffer.  No tolerance anywhere: every comparison is of bits or integers.
"""
import json
import os

import numpy as np
import pytest

import raytracingstudy_amd as rt

import multihit_ref as mr
import overlap_ref as ov
from query_fuzz import BAD_PROBES, N_ORACLE, NO_HIT, SEEDS, model
from test_gpu_gbuffer import _assert_equal as _assert_gbuffer, _assert_stats as _assert_gbuffer_stats, _bits, _run
from test_gpu_multihit import _assert_answer as _assert_multi
from test_gpu_overlap import _assert_answer as _assert_overlap
from test_gpu_query import _assert_equal as _assert_hits

pytestmark = pytest.mark.gpu

INF = np.float32(np.inf)
# seed -> what the device reported; the module's last test reads it
RECORD = {}


def _cell_table(seed, depth):
    return (None, 0, 1 + seed % depth)[seed % 3]


def _counters(st):
    return (st.primary_rays, st.shadow_rays, st.nodes_visited, st.prims_tested)


def _trace(r, m, rec):
    """trace_rays, nearest and any: a stats launch and a plain launch over the
    512 rays the oracle was given, then the 8 bad rays in a launch of their own."""
    rays = m["case"]["rays"]
    good, bad = rays[:N_ORACLE], rays[N_ORACLE:]
    for kind in ("nearest", "any"):
        exp = m[kind]
        t, sphere, st = r.trace_rays(good, kind, stats=True)
        _assert_hits(t, sphere, exp, N_ORACLE)
        miss = sphere == NO_HIT
        assert np.array_equal(t[miss].view(np.uint32), good[miss, 7].view(np.uint32))
        assert _counters(st) == ((N_ORACLE, 0) if kind == "nearest" else (0, N_ORACLE)) + (
            int(exp[3].sum()), int(exp[4].sum())), kind
        t2, sphere2 = r.trace_rays(good, kind)
        assert np.array_equal(sphere2, sphere) and np.array_equal(t2.view(np.uint32), t.view(np.uint32))
        tb, sb = r.trace_rays(bad, kind)
        assert np.all(sb == NO_HIT), f"{kind}: a bad ray hit"
        assert np.array_equal(tb.view(np.uint32), bad[:, 7].view(np.uint32)), f"{kind}: a bad ray's miss holds tmax"
        rec[kind] = dict(hits=int((~miss).sum()), nodes=st.nodes_visited, prims=st.prims_tested)
        if kind == "nearest":
            nearest = (t, sphere, _counters(st))
    return nearest


def _multi(r, m, nearest, rec):
    """trace_rays_multi over all 520 rays, k in {1, 3, 4, 16}; k = 1 on the
    oracle's 512 is the nearest query, all four stats included."""
    rays = m["case"]["rays"]
    for k in (1, 3, 4, 16):
        exp = mr.cut(m["multi"], rays, k)
        t, sphere, count, st = r.trace_rays_multi(rays, k, stats=True)
        _assert_multi((t, sphere, count), exp, rays, k, f"k={k} stats")
        assert (st.primary_rays, st.shadow_rays) == (len(rays), 0)
        _assert_multi(r.trace_rays_multi(rays, k), exp, rays, k, f"k={k}")
    rec["multi"] = dict(full=int((count == 16).sum()), nodes=st.nodes_visited, prims=st.prims_tested)
    tn, sn, stn = nearest
    t, sphere, count, st = r.trace_rays_multi(rays[:N_ORACLE], 1, stats=True)
    assert np.array_equal(sphere[:, 0], sn) and np.array_equal(t[:, 0].view(np.uint32), tn.view(np.uint32))
    assert np.array_equal(count, (sn != NO_HIT).astype(np.uint32))
    assert _counters(st) == stn


def _overlaps(r, m, info, rec):
    """query_overlaps, k in {1, 4, 16}, with and without skip_self, as stats
    launches and plain ones; the bad probes empty; the stats inside
    test_gpu_overlap.test_stats' bounds, and the same at k = 1 and k = 16.
    (Six launches: in the clustered scenes a large probe holds most of a
    million leaf references, and one launch takes most of a second.)"""
    pr = m["case"]["probes"]
    seen = {}
    for skip, key, with_stats in ((False, "overlap", (1, 16)), (True, "overlap_skip", (1,))):
        ref = m[key]
        for k in (1, 4, 16):
            idx, count, more, *st = r.query_overlaps(pr, k, skip_self=skip, stats=k in with_stats)
            _assert_overlap((idx, count, more), ov.cut(ref, k), k, f"{key} k={k}")
            assert np.all(idx[BAD_PROBES] == NO_HIT) and not count[BAD_PROBES].any() and not more[BAD_PROBES].any()
            for a in st:
                assert int(ref[3].sum()) <= a.prims_tested <= len(pr) * info["n_prim_refs"]
                assert 0 < a.nodes_visited <= len(pr) * info["n_nodes"]
                assert (a.primary_rays, a.shadow_rays) == (0, 0) and a.ms > 0.0
                seen[key, k] = (a.nodes_visited, a.prims_tested)
        rec[key] = dict(touching=int((count > 0).sum()), more=int(more.sum()), nodes=seen[key, 1][0],
                        prims=seen[key, 1][1])
    assert seen["overlap", 1] == seen["overlap", 16]  # k stops nothing


def _gbuffer(r, m, rec):
    """render_gbuffer into 0xAB-filled buffers one record longer than the frame
    (_run asserts the guard records): a stats launch and a plain one."""
    c, exp = m["case"], m["gbuffer"]
    got = _run(r, c["w"], c["h"], stats=True)
    _assert_gbuffer(got, exp)
    _assert_gbuffer_stats(got["stats"], exp, c["w"], c["h"])
    _assert_gbuffer(_run(r, c["w"], c["h"]), exp)
    rec["gbuffer"] = dict(hits=int((got["sphere"] != NO_HIT).sum()), nodes=got["stats"].nodes_visited,
                          prims=got["stats"].prims_tested)
    return got


def _one_shots(r, orc, m, got, rec):
    """pick, pick_multi(.., 4) and overlaps_at at the picked point, at up to two
    pixels that hit and two that miss: each is the batch call's answer."""
    c, exp = m["case"], m["gbuffer"]
    origin = c["pose"][3, :3].astype(np.float32)
    rec["picks"] = []
    for x, y in m["pixels"]:
        hit, t, sphere, point = r.pick(float(x), float(y))
        assert sphere == got["sphere"][y, x] == exp["sphere"][y, x] and hit == (sphere != NO_HIT)
        assert np.float32(t).view(np.uint32) == got["t"][y, x].view(np.uint32)
        d = orc.get_ray(c["pose"], c["K"], float(x), float(y))
        assert np.array_equal(_bits(d), _bits(exp["dirs"][y, x]))
        ray = np.zeros((1, 8), np.float32)
        ray[0, :3], ray[0, 4:7], ray[0, 7] = origin, d, INF
        cnt, mt, ms = r.pick_multi(float(x), float(y), 4)
        ref = mr.reference(c["sp"], ray, 4)
        _assert_multi(r.trace_rays_multi(ray, 4), ref[:3], ray, 4, f"pixel ({x}, {y}) batch")
        assert cnt == ref[2][0] and np.array_equal(ms, ref[1][0])
        assert np.array_equal(mt.view(np.uint32), ref[0][0].view(np.uint32))
        assert ms[0] == sphere and mt[0] == np.float32(t)
        if hit:
            # a brush of the picked sphere's own radius around the picked point: it holds that sphere
            assert np.array_equal(point, origin + np.float32(t) * d)
            R = float(c["sp"][sphere, 3])
        else:
            # a miss picks no point: the case's first far probe
            point, R = c["probes"][BAD_PROBES.start - 1, :3], float(c["probes"][BAD_PROBES.start - 1, 3])
        probe = np.array([(*point, R)], np.float32)
        ref = ov.reference(c["sp"], probe, 16)
        idx, count, more = r.query_overlaps(probe, 16)
        _assert_overlap((idx, count, more), ref[:3], 16, f"pixel ({x}, {y}) brush")
        oc, oi, om = r.overlaps_at(point, R, 16)
        assert (oc, om) == (int(count[0]), bool(more[0])) and np.array_equal(oi, idx[0])
        rec["picks"].append(dict(x=int(x), y=int(y), sphere=int(sphere), listed=int(cnt), brush=int(ref[3][0])))


@pytest.mark.parametrize("seed", range(SEEDS))
def test_queries_are_the_references(gpu, oracle, seed):
    m = model(seed, oracle, gbuffer=True)
    c = m["case"]
    cell_table = _cell_table(seed, c["depth"])
    rec = dict(seed=seed, n=c["n"], depth=c["depth"], leaf=c["leaf"], mode=c["mode"], w=c["w"], h=c["h"],
               cell_table=cell_table)
    with rt.KernelRenderer(c["w"], c["h"], mode="scene", cell_table=cell_table) as r:
        r.resize(c["w"], c["h"])
        r.setIntrinsic(c["K"])
        r.setPosition(c["pose"])
        info = r.set_scene(c["sp"], c["al"], max_depth=c["depth"], leaf_capacity=c["leaf"])
        pose, K = r.camera()
        assert np.array_equal(K, c["K"]) and np.array_equal(pose, c["pose"])
        # the tree is the oracle's, its grown root box included
        assert {k: info[k] for k in m["info"]} == m["info"]
        assert np.array_equal(np.array(info["root_min"], np.float32), m["root"][0])
        assert np.array_equal(np.array(info["root_max"], np.float32), m["root"][1])
        rec.update(n_nodes=info["n_nodes"], n_prim_refs=info["n_prim_refs"], depth_reached=info["depth_reached"],
                   cell_table_depth=info["cell_table_depth"])
        nearest = _trace(r, m, rec)
        _multi(r, m, nearest, rec)
        _overlaps(r, m, info, rec)
        got = _gbuffer(r, m, rec)
        _one_shots(r, oracle, m, got, rec)
    RECORD[seed] = rec


def test_the_cases_ran_on_every_kind_of_tree(gpu):
    """What the device reported over the 64 cases: all three cell table
    settings ran (21 or 22 seeds each), a fixed depth was honoured, trees whose
    root is a leaf ran, and trees that list a sphere in ten leaves or more on
    average ran (the clustered scenes: a 0.2 radius beside 0.0005 ones).  The
    oracle's trees of the 64 cases have 4 of the former (n = 1, or n = 7 under
    a leaf capacity of 7 or more) and 6 of the latter, and the per-seed test
    holds the device's tree to the oracle's; the floors are 3 and 4, and a
    change of plain_case that loses them is what this notices.  Judged only when every
    seed ran in this process (the record above is filled by the per-seed
    test); a run of a subset checks nothing here.  With RT_QUERY_FUZZ_RECORD
    set, the per-seed record is written to that file."""
    path = os.environ.get("RT_QUERY_FUZZ_RECORD")
    if path:
        with open(path, "w") as f:
            for seed in sorted(RECORD):
                f.write(json.dumps(RECORD[seed]) + "\n")
    if len(RECORD) < SEEDS:
        return
    rows = list(RECORD.values())
    auto = [v for v in rows if v["cell_table"] is None]
    off = [v for v in rows if v["cell_table"] == 0]
    fixed = [v for v in rows if v["cell_table"]]
    leaf_root = [v for v in rows if v["n_nodes"] == 1]
    dense = [v for v in rows if v["n_prim_refs"] >= 10 * v["n"]]
    print(f"query fuzz: cell table auto {len(auto)}, off {len(off)}, fixed {len(fixed)}; "
          f"{len(leaf_root)} root-is-leaf trees, {len(dense)} dense trees; "
          f"{sum(v['nearest']['hits'] for v in rows)} nearest hits, "
          f"{sum(v['multi']['full'] for v in rows)} full 16-lists, "
          f"{sum(v['overlap']['more'] for v in rows)} MORE bits, "
          f"{sum(v['gbuffer']['hits'] for v in rows)} pixels hit")
    assert min(len(auto), len(off), len(fixed)) >= 21
    assert all(v["cell_table_depth"] == 0 for v in off)
    assert all(v["cell_table_depth"] in (0, min(v["cell_table"], v["depth"], v["depth_reached"], 7))
               for v in fixed if v["n_nodes"] > 1)
    assert any(v["cell_table_depth"] > 0 for v in fixed) and any(v["cell_table_depth"] > 0 for v in auto)
    assert len(leaf_root) >= 3, len(leaf_root)
    assert len(dense) >= 4, len(dense)
