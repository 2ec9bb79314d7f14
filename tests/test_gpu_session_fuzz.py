"""One long-lived renderer per session_fuzz.py session: the steps run in order
on ONE handle, and every reading step is held to session_fuzz.expected, bit
for bit.  The other GPU tests read from fresh handles; what a handle shows
after scenes grew, shrank and emptied, the tree was rebuilt, the frame resized,
the camera moved and calls were refused, with queries and frames alternating
on three streams, is decided by its host state (csrc/rt_host.h), and only such
a sequence sees that state go stale.

The expectations come from session_fuzz.Model (include/rt.h's rules) and the
references, never from the handle.  Reading steps on a caller's stream are read
after that stream alone is synchronised, so the handle's own ordering
(order_after_last) is what keeps them behind the step before.  Every caller
buffer is filled with 0xAB and carries a guard record; the handle's own
buffers are poisoned by RT_FLAG_TEST_POISON (conftest.py).

A mismatch names the seed, the step and the kinds so far, then replays the
model's state on a fresh handle: "fresh agrees" points at stale host state,
"fresh disagrees" at a kernel or a builder.

Measured on the MI355X box, oracle time included: a session takes 0.1 to 0.3 s
at the median and 2.2 to 2.8 s at most (a pool with a clustered scene of 3,000
spheres), all 32 together 7 to 16 s.
"""
import json
import os
import time
import types

import numpy as np
import pytest

import raytracingstudy_amd as rt
from raytracingstudy_amd._lib import RT_OVERLAP_MORE, RtError

import session_fuzz as sf
from bins_native import build_dump
from session_fuzz import N_GOOD, READ_KINDS, SESSIONS, STATE_KINDS, TS, Model, expected, session
from test_gpu_closest import _assert_answer as _assert_closest
from test_gpu_gbuffer import _assert_equal as _assert_gbuffer, _assert_stats as _assert_gbuffer_stats, _run
from test_gpu_multihit import _assert_answer as _assert_multi
from test_gpu_overlap import _assert_answer as _assert_overlap
from test_gpu_query import _assert_equal as _assert_hits

pytestmark = pytest.mark.gpu

GUARD = 16
# seed -> what the session reported; the module's last test reads it
RECORD = {}


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    return build_dump(tmp_path_factory.mktemp("bin"))


@pytest.fixture
def hooks(monkeypatch):
    monkeypatch.setenv("RT_TEST_BIN_MIN_SAMPLES", "0")
    monkeypatch.setenv("RT_TEST_BIN_MEAN", "1000000")


# ---- buffers and streams -----------------------------------------------------------

def _dev(a):
    """A host array's bytes in device memory (None for an empty one)."""
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda() if a.size else None


def _out(nbytes):
    """nbytes of 0xAB in device memory, and a guard record after them."""
    import torch
    return torch.full((nbytes + GUARD,), 0xAB, dtype=torch.uint8, device="cuda")


def _ptr(t):
    return t.data_ptr() if t is not None else 0


def _host(t, nbytes, dtype):
    raw = t.cpu().numpy()
    assert (raw[nbytes:] == 0xAB).all(), "a write past the end of a caller's buffer"
    return raw[:nbytes].view(dtype)


def _context(r, m, orc, dump, rec, tmp):
    import torch
    c = types.SimpleNamespace(r=r, m=m, orc=orc, dump=dump, rec=rec, tmp=tmp,
                              streams=[None, torch.cuda.Stream(), torch.cuda.Stream()])
    c.ptr = lambda step: c.streams[step["stream"]].cuda_stream if step["stream"] else None
    # the step's stream alone (the handle's own: the handle's call)
    c.sync = lambda step: c.streams[step["stream"]].synchronize() if step["stream"] else r.synchronize()
    return c


def _ready():
    """The buffers were made and filled on torch's stream: they are done before a launch on another."""
    import torch
    torch.cuda.synchronize()


def _fits(c):
    assert c.r.width * c.r.height <= c.m.w * c.m.h, "the handle's frame is larger than the model's buffers"


def _counters(st):
    return (st.primary_rays, st.shadow_rays, st.nodes_visited, st.prims_tested)


def _tree_counts(c):
    info = c.r.scene_info()
    return info["n_nodes"], info["n_prim_refs"]


# ---- reading steps -------------------------------------------------------------------

def _trace(c, step, exp):
    kind = step["kind"][6:]
    rays = sf.inputs(c.m, step)
    n = len(rays)
    d_rays, d_hits = _dev(rays), _out(n * 8)
    _ready()
    c.r.trace_rays_device(d_rays.data_ptr(), n, d_hits.data_ptr(), kind, stream=c.ptr(step))
    c.sync(step)
    hits = _host(d_hits, n * 8, np.uint32).reshape(n, 2)
    t, sphere = np.ascontiguousarray(hits[:, 0]).view(np.float32), np.ascontiguousarray(hits[:, 1])
    _assert_hits(t, sphere, exp["hits"])
    # the stats launch: the rays the oracle was given (test_gpu_query.test_edge_rays says why)
    st = c.r.trace_rays_device(d_rays.data_ptr(), N_GOOD, d_hits.data_ptr(), kind, stream=c.ptr(step), stats=True)
    hits = _host(d_hits, n * 8, np.uint32).reshape(n, 2)
    _assert_hits(np.ascontiguousarray(hits[:, 0]).view(np.float32), np.ascontiguousarray(hits[:, 1]), exp["hits"])
    work = (int(exp["hits"][3].sum()), int(exp["hits"][4].sum()))
    assert _counters(st) == ((N_GOOD, 0) if kind == "nearest" else (0, N_GOOD)) + work, kind


def _in_flight(c, step):
    """Leaves a nearest query unsynchronised on the step's stream; the returned
    call waits for that stream and checks the answer."""
    q = dict(kind="trace_nearest", stream=step["stream"])
    rays = sf.inputs(c.m, q)
    n = len(rays)
    d_rays, d_hits = _dev(rays), _out(n * 8)
    _ready()
    c.r.trace_rays_device(d_rays.data_ptr(), n, d_hits.data_ptr(), "nearest", stream=c.ptr(step))

    def done():
        c.sync(step)
        hits = _host(d_hits, n * 8, np.uint32).reshape(n, 2)
        _assert_hits(np.ascontiguousarray(hits[:, 0]).view(np.float32), np.ascontiguousarray(hits[:, 1]),
                     expected(c.m, q, c.orc)["hits"])
    return done


def _lists(c, step, launch, width):
    """A list query's two launches, plain on the step's stream and stats:
    (records (n, k, width) uint32, counts (n,) uint32, stats) of each."""
    inp = sf.inputs(c.m, step)
    n, k = len(inp), step["k"]
    d_in = _dev(inp)
    out = []
    for stats in (False, True):
        d_rec, d_cnt = _out(n * k * 4 * width), _out(n * 4)
        _ready()
        st = launch(_ptr(d_in), n, k, d_rec.data_ptr() if n else 0, d_cnt.data_ptr() if n else 0,
                    stream=c.ptr(step), stats=stats)
        c.sync(step)
        rec = _host(d_rec, n * k * 4 * width, np.uint32).reshape(n, k, width)
        out.append((rec, _host(d_cnt, n * 4, np.uint32).copy(), st))
    return inp, out


def _multi(c, step, exp):
    rays, got = _lists(c, step, c.r.trace_rays_multi_device, 2)
    for rec, count, st in got:
        t, sphere = np.ascontiguousarray(rec[:, :, 0]).view(np.float32), np.ascontiguousarray(rec[:, :, 1])
        _assert_multi((t, sphere, count), exp["answer"], rays, step["k"], "stats" if st else "plain")
    assert (st.primary_rays, st.shadow_rays) == (len(rays), 0)


def _work_within(c, st, n, least):
    n_nodes, n_refs = _tree_counts(c)
    assert least <= st.prims_tested <= n * n_refs and st.nodes_visited <= n * n_nodes
    assert (st.primary_rays, st.shadow_rays) == (0, 0)


def _overlaps(c, step, exp):
    skip = step["kind"] == "overlaps_self"
    probes, got = _lists(c, step, lambda *a, **kw: c.r.query_overlaps_device(*a, skip_self=skip, **kw), 1)
    for rec, words, st in got:
        count, more = words & np.uint32(~RT_OVERLAP_MORE & 0xFFFFFFFF), (words & np.uint32(RT_OVERLAP_MORE)) != 0
        _assert_overlap((np.ascontiguousarray(rec[:, :, 0]), count, more), exp["answer"], step["k"],
                        "stats" if st else "plain")
    _work_within(c, st, len(probes), exp["total"])


def _closest(c, step, exp):
    skip = step["kind"] == "closest_self"
    probes, got = _lists(c, step, lambda *a, **kw: c.r.query_closest_device(*a, skip_self=skip, **kw), 2)
    for rec, count, st in got:
        dist, sphere = np.ascontiguousarray(rec[:, :, 0]).view(np.float32), np.ascontiguousarray(rec[:, :, 1])
        _assert_closest((dist, sphere, count), exp["answer"], probes, step["k"], "stats" if st else "plain")
    _work_within(c, st, len(probes), int(exp["answer"][2].sum()))


def _gbuffer(c, step, exp):
    import torch
    _fits(c)
    s = c.streams[step["stream"]]
    for stats in (False, True):
        if s is None:
            got = _run(c.r, c.m.w, c.m.h, stats=stats)
        else:
            with torch.cuda.stream(s):      # (the buffers are made, filled and read on the step's stream)
                got = _run(c.r, c.m.w, c.m.h, stream=s.cuda_stream, stats=stats)
        _assert_gbuffer(got, exp["gbuffer"])
    _assert_gbuffer_stats(got["stats"], exp["gbuffer"], c.m.w, c.m.h)


def _pick(c, step, exp):
    done = _in_flight(c, step)
    x, y = exp["xy"]
    hit, t, sphere, point = c.r.pick(float(x), float(y))
    assert (hit, sphere) == (exp["hit"], exp["sphere"]), (x, y)
    assert np.float32(t).view(np.uint32) == exp["t"].view(np.uint32)
    if hit:
        assert np.array_equal(point.view(np.uint32), exp["point"].view(np.uint32))
    done()


def _pick_multi(c, step, exp):
    done = _in_flight(c, step)
    x, y = exp["xy"]
    count, t, sphere = c.r.pick_multi(float(x), float(y), step["k"])
    assert count == exp["count"] and np.array_equal(sphere, exp["sphere"]), (x, y)
    assert np.array_equal(t.view(np.uint32), exp["t"].view(np.uint32))
    done()


def _overlaps_at(c, step, exp):
    done = _in_flight(c, step)
    p = exp["probe"]
    count, idx, more = c.r.overlaps_at(p[:3], float(p[3]), step["k"])
    assert (count, more) == (exp["count"], exp["more"]) and np.array_equal(idx, exp["indices"])
    done()


def _closest_at(c, step, exp):
    done = _in_flight(c, step)
    p = exp["probe"]
    count, dist, sphere = c.r.closest_at(p[:3], float(p[3]), step["k"])
    assert count == exp["count"] and np.array_equal(sphere, exp["sphere"])
    assert np.array_equal(dist.view(np.uint32), exp["dist"].view(np.uint32))
    done()


def _same_frame(c, exp, rgba8):
    assert rgba8.shape == exp["rgba8"].shape and np.array_equal(rgba8, exp["rgba8"]), "RGBA8 differs from the oracle"
    assert np.array_equal(c.r.readback_radiance().view(np.uint32), exp["radiance"].view(np.uint32)), \
        "radiance differs from the oracle"


def _frame(c, step, exp):
    """A plain frame into the internal framebuffer, and the path its bins report."""
    c.r.render(stream=c.ptr(step))
    c.sync(step)
    _same_frame(c, exp, c.r.readback())
    bi = c.r.bin_info()
    reason, wide, entries = sf.bins_rule(c.dump, c.orc, c.m)
    c.rec["bins"].append((reason, bi["reason"]))
    if reason == "capacity" and bi["reason"] != "capacity":
        # the entry buffer only grows: an earlier scene's held these entries
        reason = "wide" if wide > sf.WIDE_CAP else "on"
    assert bi["reason"] == reason, (bi, reason)
    if reason == "on":
        assert (bi["wide"], bi["entries"]) == (wide, entries), (bi, wide, entries)
    c.rec["lists"].append(c.r.scene_info()["occluder_lists_on"])


def _frame_stats(c, step, exp):
    st = c.r.render(stream=c.ptr(step), stats=True)
    _same_frame(c, exp, c.r.readback())
    assert _counters(st) == exp["counters"]
    if c.m.cfg["progressive"]:
        assert st.samples_per_pixel == c.m.cfg["spp"] * len(c.m.history)
    assert c.r.bin_info()["reason"] == "kernel"


def _frame_caller(c, step, exp):
    _fits(c)
    n = c.m.w * c.m.h * 4
    buf = _out(n)
    _ready()
    c.r.render(dev_ptr=buf.data_ptr(), stream=c.ptr(step))
    c.sync(step)
    _same_frame(c, exp, _host(buf, n, np.uint8).reshape(c.m.h, c.m.w, 4))


def _tiles(c, step, exp):
    _fits(c)
    ids = exp["ids"]
    n, px = len(ids) * TS * TS * 4, c.m.w * c.m.h * 4
    packed, img = _out(n), _out(px)
    _ready()
    c.r.render_tiles(ids, TS, packed.data_ptr(), stream=c.ptr(step))
    c.r.unpack_tiles(packed.data_ptr(), ids, TS, img.data_ptr(), stream=c.ptr(step))
    c.sync(step)
    assert np.array_equal(_host(packed, n, np.uint8).reshape(len(ids), TS, TS, 4), exp["packed"]), \
        "a packed tile differs from the oracle's frame"
    assert np.array_equal(_host(img, px, np.uint8).reshape(c.m.h, c.m.w, 4), exp["image"]), \
        "the unpacked tiles differ from the oracle's frame"


CHECKS = dict(frame=_frame, frame_stats=_frame_stats, frame_caller=_frame_caller, tiles=_tiles, gbuffer=_gbuffer,
              pick=_pick, pick_multi=_pick_multi, trace_nearest=_trace, trace_any=_trace, multi=_multi,
              overlaps=_overlaps, overlaps_self=_overlaps, closest=_closest, closest_self=_closest,
              overlaps_at=_overlaps_at, closest_at=_closest_at)


# ---- state-changing steps ------------------------------------------------------------

def _scene_device(c, i, sp, al, step):
    import torch
    s = c.streams[1 + i % 2]
    with torch.cuda.stream(s):      # the list is produced on a caller's stream, which the call waits for
        d_sp = torch.from_numpy(sp.copy()).cuda(non_blocking=True) if len(sp) else None
        d_al = torch.from_numpy(al.copy().view(np.int32)).cuda(non_blocking=True) if len(sp) else None
    c.r.set_scene_device(_ptr(d_sp), len(sp), _ptr(d_al), stream=s.cuda_stream, max_depth=step["depth"],
                         leaf_capacity=step["leaf"])


def _refused(c, i, step):
    """A call rt.h refuses: RT_E_INVALID, and the handle's scene, tree and camera stay."""
    r, what = c.r, step["what"]
    before = r.scene_info()
    with pytest.raises(RtError) as e:
        if what in ("nan_scene", "zero_radius_scene"):
            r.set_scene(*sf.refused_spheres(c.m.cfg, step), max_depth=step["depth"], leaf_capacity=step["leaf"])
        elif what == "zero_radius_device":
            _scene_device(c, i, *sf.refused_spheres(c.m.cfg, step), step)
        elif what == "empty_box":
            r.setOctree((0.5, 0.0, 0.0), (0.5, 1.0, 1.0), 0.05)
        elif what == "tile_id":
            packed = _out(TS * TS * 4)
            _ready()
            tx, ty = rt.tiles.tile_grid(r.width, r.height, TS)
            r.render_tiles(np.array([tx * ty], np.uint32), TS, packed.data_ptr())
        else:
            k = 0 if what == "k0" else 17
            inp = sf.inputs(c.m, dict(kind=step["query"]))
            d_in, d_rec, d_cnt = _dev(inp), _out(len(inp) * 17 * 8), _out(len(inp) * 4)
            _ready()
            launch = dict(multi=r.trace_rays_multi_device, overlaps=r.query_overlaps_device,
                          closest=r.query_closest_device)[step["query"]]
            launch(d_in.data_ptr(), len(inp), k, d_rec.data_ptr(), d_cnt.data_ptr())
    assert e.value.code == sf.RT_E_INVALID, (what, e.value)
    after = r.scene_info()
    for key in ("n_spheres", "n_nodes", "n_prim_refs", "max_depth", "root_min", "root_max"):
        assert after[key] == before[key], (what, key)


def _apply(c, i, step):
    """The step's call on the handle; the model has not applied it yet."""
    r, kind, cfg = c.r, step["kind"], c.m.cfg
    if kind in sf.SCENE_KINDS:
        sp, al = sf.spheres(cfg, step["scene"])
        if kind == "set_scene":
            r.set_scene(sp, al, max_depth=step["depth"], leaf_capacity=step["leaf"])
        elif kind == "set_scene_device":
            _scene_device(c, i, sp, al, step)
        else:
            path = str(c.tmp / f"scene_{cfg['seed']}_{i}.bin")
            rt.save_spheres(path, sp, al)
            r.set_scene_file(path, max_depth=step["depth"], leaf_capacity=step["leaf"])
    elif kind == "set_octree":
        r.setOctree(step["root_min"], step["root_max"], step["resolution"])
    elif kind in ("resize_up", "resize_down"):
        r.resize(step["w"], step["h"])
    elif kind == "set_pose":
        r.setPosition(sf.camera(cfg, step["cam"])["pose"])
    elif kind == "set_intrinsic":
        r.setIntrinsic(sf.camera(cfg, step["cam"])["K"])
    elif kind == "reset_accumulation":
        r.reset_accumulation()
    else:
        _refused(c, i, step)


def _built(c, step):
    """After a scene or tree change: the handle's tree is the oracle's of the model's state."""
    m = c.m
    info = c.r.scene_info()
    s = sf.oracle_scene(c.orc, m.cfg, m.seen, m.tree)
    assert info["n_spheres"] == len(sf.spheres(m.cfg, m.seen)[0]) and info["max_depth"] == m.tree[2], info
    assert {k: info[k] for k in s.info()} == s.info(), (info, s.info())
    assert np.array_equal(np.array(info["root_min"], np.float32), s.root()[0])
    assert np.array_equal(np.array(info["root_max"], np.float32), s.root()[1])
    c.rec["builders"].append(info["builder"])


def _renderer(cfg, w, h):
    return rt.KernelRenderer(w, h, mode="scene", spp=cfg["spp"], radiance=True, shadows=cfg["shadows"],
                             jitter=cfg["jitter"], light_dir=cfg["light"], ambient=cfg["ambient"],
                             progressive=cfg["progressive"], cell_table=cfg["cell_table"])


def _fresh_agrees(sess, m, step, orc, dump, tmp):
    """The model's current state on a fresh handle, and the same reading step
    (a progressive frame: as the first of its sums)."""
    fm = Model(sess)
    fm.scene, fm.seen, fm.tree, fm.w, fm.h, fm.pose, fm.K, fm.view_pose = (m.scene, m.seen, m.tree, m.w, m.h,
                                                                           m.pose, m.K, m.pose)
    sp, al = sf.spheres(m.cfg, m.seen)
    with _renderer(m.cfg, m.w, m.h) as fr:
        fr.resize(m.w, m.h)
        fr.setIntrinsic(m.K)
        fr.setPosition(m.pose)
        fr.set_scene(sp, al, root_min=m.tree[0], root_max=m.tree[1], max_depth=m.tree[2], leaf_capacity=m.tree[3])
        c = _context(fr, fm, orc, dump, dict(bins=[], lists=[], builders=[]), tmp)
        try:
            CHECKS[step["kind"]](c, step, expected(fm, step, orc))
        except AssertionError:
            return False
    return True


def run_session(seed, orc, dump, tmp, withhold=None, rec=None):
    """The session's steps on one handle.  `withhold`: the index of a
    state-changing step the handle is not given, while the model applies it
    (the negative control)."""
    sess = session(seed)
    cfg, steps = sess["cfg"], sess["steps"]
    m = Model(sess)
    rec = rec if rec is not None else {}
    rec.update(seed=seed, steps=len(steps), kinds=[s["kind"] for s in steps], spp=cfg["spp"],
               progressive=cfg["progressive"], pool=list(cfg["pool"]), bins=[], lists=[], builders=[])
    with _renderer(cfg, cfg["w"], cfg["h"]) as r:
        c = _context(r, m, orc, dump, rec, tmp)
        for i, step in enumerate(steps):
            if step["kind"] in STATE_KINDS:
                if i != withhold:
                    _apply(c, i, step)
                m.apply(step, orc)
                if i != withhold and step["kind"] in sf.SCENE_KINDS + ("set_octree",) and withhold is None:
                    _built(c, step)
                continue
            exp = expected(m, step, orc)
            try:
                CHECKS[step["kind"]](c, step, exp)
            except AssertionError as e:
                # (only after a mismatch: a HIP error is no AssertionError and ends the session as it is)
                where = f"session {seed}, step {i} ({step}) after {[s['kind'] for s in steps[:i]]}"
                if withhold is not None:
                    raise AssertionError(f"{where}: {e}") from e
                fresh = _fresh_agrees(sess, m, step, orc, dump, tmp)
                verdict = ("a fresh handle in this state agrees with the reference: stale host state" if fresh else
                           "a fresh handle in this state disagrees too: a kernel or builder fault")
                raise AssertionError(f"{where}: {e}\n{verdict}") from e
        pose, K = r.camera()
        assert np.array_equal(pose, m.pose) and np.array_equal(K, m.K)
    return rec


@pytest.mark.parametrize("seed", range(SESSIONS))
def test_session(gpu, oracle, hooks, dump, tmp_path, seed):
    t0 = time.perf_counter()
    rec = {}
    run_session(seed, oracle, dump, tmp_path, rec=rec)
    rec["seconds"] = round(time.perf_counter() - t0, 3)
    print(f"session {seed}: {rec['steps']} steps in {rec['seconds']} s")
    RECORD[seed] = rec


def _first_seen(orc, kind, readers):
    """(seed, index) of the first step of this kind, past the session's
    opening calls, whose next step is one of `readers` with another expected
    answer when the step is left out: the references say that a handle which
    never got the call is seen there."""
    for seed in range(SESSIONS):
        sess = session(seed)
        steps = sess["steps"]
        for i in range(3, len(steps) - 1):
            if steps[i]["kind"] != kind or steps[i + 1]["kind"] not in readers:
                continue
            with_it, without = Model(sess), Model(sess)
            for j, step in enumerate(steps[:i + 2]):
                if step["kind"] in STATE_KINDS:
                    with_it.apply(step, orc)
                    if j != i:
                        without.apply(step, orc)
                else:
                    a, b = expected(with_it, step, orc), expected(without, step, orc)
            if not sf.same(a, b):
                return seed, i
    raise AssertionError(f"no session has such a {kind} step")


# the readings that cannot miss another size or camera: whole frames and the G-buffer
WHOLE = ("frame", "frame_stats", "frame_caller", "gbuffer")


@pytest.mark.parametrize("kind", ["set_scene", "resize_up", "set_pose"])
def test_withheld_call_is_seen(gpu, oracle, hooks, dump, tmp_path, kind):
    """The negative control, on the device: the handle is not given one
    state-changing call (a second set_scene, a resize, a setPosition) that the
    model applies, and the session's checks must notice at a later step."""
    seed, at = _first_seen(oracle, kind, READ_KINDS if kind == "set_scene" else WHOLE)
    with pytest.raises(AssertionError, match=rf"session {seed}, step (\d+)") as e:
        run_session(seed, oracle, dump, tmp_path, withhold=at)
    seen_at = int(str(e.value).split("step ")[1].split(" ")[0])
    print(f"withheld {kind} (session {seed}, step {at}) seen at step {seen_at}")
    assert seen_at > at


def test_tile_list_cache_evicts_and_refills(gpu, oracle, hooks):
    """Beside the fuzz, what its sessions are too short to reach: the handle
    keeps the device copies of the 16 tile lists used last (rt_frame.cpp,
    tile_list) and gives the least recently used slot to a new one.  One handle
    renders 30 distinct lists (every sequence of 1 to 4 of a two-tile frame's
    tiles, repeats included) in turn on three streams, each also unpacked, then
    the first eight again, which were evicted by then: every packed buffer and
    every unpacked image is the oracle's frame."""
    import itertools
    sess = session(1)
    m = Model(sess)
    for step in sess["steps"][:3]:
        m.apply(step, oracle)
    m.apply(dict(kind="resize_up", w=70, h=50), oracle)
    ref8 = sf._render(m.cfg, oracle, m.frame_key(), 0, None)[0]
    assert len(np.unique(ref8.reshape(-1, 4), axis=0)) > 1      # (the camera sees the scene)
    lists = [np.array(t, np.uint32) for n in range(1, 5) for t in itertools.product((0, 1), repeat=n)]
    assert len(lists) == 30
    sp, al = sf.spheres(m.cfg, m.seen)
    with _renderer(m.cfg, m.cfg["w"], m.cfg["h"]) as r:
        c = _context(r, m, oracle, None, {}, None)
        r.resize(m.w, m.h)
        r.setPosition(m.pose)
        r.set_scene(sp, al, max_depth=m.tree[2], leaf_capacity=m.tree[3])
        for i, ids in enumerate(lists + lists[:8]):
            exp = dict(ids=ids, packed=rt.tiles.pack_reference(ref8, ids, TS))
            exp["image"] = rt.tiles.unpack_host(exp["packed"], ids, m.w, m.h, TS,
                                                out=np.full((m.h, m.w, 4), 0xAB, np.uint8))
            try:
                _tiles(c, dict(kind="tiles", stream=i % 3), exp)
            except AssertionError as e:
                raise AssertionError(f"list {i} {ids.tolist()}: {e}") from e


def test_the_sessions_ran_on_bins(gpu):
    """What the sessions reported.  With RT_SESSION_FUZZ_RECORD set, the
    per-seed record (steps, kinds, the bins' reasons as (static rule, device),
    builders, occluder-list state, seconds) is written to that file.  Judged
    only when every seed ran in this process: of the plain frames whose static
    rule says `on`, at least half reported `on` (a handle's history may only
    turn a `capacity` into `on`, never an `on` into anything else, so this
    notices a generator that stopped reaching the bins)."""
    path = os.environ.get("RT_SESSION_FUZZ_RECORD")
    if path:
        with open(path, "w") as f:
            for seed in sorted(RECORD):
                f.write(json.dumps(RECORD[seed]) + "\n")
    if len(RECORD) < SESSIONS:
        return
    bins = [b for v in RECORD.values() for b in v["bins"]]
    static_on = [b for b in bins if b[0] == "on"]
    print(f"session fuzz: {sum(v['steps'] for v in RECORD.values())} steps, {len(bins)} plain frames, "
          f"{len(static_on)} with the static rule `on`, {sum(b[1] == 'on' for b in static_on)} of them on bins; "
          f"slowest session {max(v['seconds'] for v in RECORD.values())} s, "
          f"all {round(sum(v['seconds'] for v in RECORD.values()), 1)} s")
    assert static_on and 2 * sum(b[1] == "on" for b in static_on) >= len(static_on), bins
