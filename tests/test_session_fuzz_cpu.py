"""The session fuzz (session_fuzz.py) on the CPU, before a GPU sees it: what the
32 generated call sequences cover, that every reading step has a reference
answer and a check, that the two references of the ray queries agree on every
tree a session builds, and that the sequences can see stale state: eleven
wrong models, each breaking one of include/rt.h's rules, give a different
expected answer than the true model.  Nothing here touches the product.
"""
import collections

import numpy as np
import pytest

import session_fuzz as sf
from session_fuzz import (EMPTY, FRAME_KINDS, MUTANTS, N_GOOD, PAIRS, READ_KINDS, SCENE_KINDS, SESSIONS,
                          STATE_KINDS, Model, expected, session)


def _walk(seed, orc, mutant=None):
    """(index, step, model) per step, the model as it is when the step begins."""
    s = session(seed)
    m = Model(s, mutant)
    for i, step in enumerate(s["steps"]):
        yield i, step, m
        if step["kind"] in STATE_KINDS:
            m.apply(step, orc)


def test_the_sessions_cover_what_they_are_for(oracle):
    """Conditions on the generator, not on the product: where one fails, change
    the generator, never the floor.  Floor and what the generator gives:

      every pair of PAIRS adjacent, over the 32 sessions            >= 2      2 to 13
      every reading kind on each of the three streams               >= 1      6 and more
      sessions with a growth and a shrink of n_prim_refs            == 32     32
      sessions with the empty scene between two non-empty ones      >= 8      11
      progressive sessions                                          >= 10     11
        each with a tile frame between two full frames              all       all
      steps per session (1,018 in all)                              24 to 40  30 to 37
      every refusal (REFUSALS)                                      >= 2      3 to 7
    """
    adjacent, streams, refusals = collections.Counter(), collections.Counter(), collections.Counter()
    empties = progressive = 0
    lengths = []
    for seed in range(SESSIONS):
        s = session(seed)
        steps = s["steps"]
        lengths.append(len(steps))
        kinds = [st["kind"] for st in steps]
        assert set(kinds) <= set(STATE_KINDS + READ_KINDS)
        assert kinds.index("set_scene") < min(i for i, k in enumerate(kinds) if k in READ_KINDS)
        for a, b in zip(kinds, kinds[1:]):
            adjacent[a, b] += 1
        refs, scenes = [], []
        for i, st, m in _walk(seed, oracle):
            if st["kind"] in READ_KINDS:
                streams[st["kind"], st["stream"]] += 1
                key = (m.seen, m.tree)
                if not refs or refs[-1][0] != key:
                    refs.append((key, sf.oracle_scene(oracle, m.cfg, m.seen, m.tree).info()["n_prim_refs"]))
            elif st["kind"] in SCENE_KINDS:
                scenes.append(st["scene"])
            elif st["kind"] == "refused":
                refusals[st["what"]] += 1
            if st["kind"] in ("resize_up", "resize_down"):
                assert (st["w"] * st["h"] > m.w * m.h) == (st["kind"] == "resize_up")
                assert 9 <= st["w"] <= 72 and 9 <= st["h"] <= 56 and st["w"] % 8 and st["h"] % 8
            if st["kind"] == "reset_accumulation":
                assert s["cfg"]["progressive"]
        sizes = [n for _, n in refs]
        assert any(b > a for a, b in zip(sizes, sizes[1:])), (seed, sizes)
        assert any(b < a for a, b in zip(sizes, sizes[1:])), (seed, sizes)
        assert len({sf.case_of(s["cfg"], k)["n"] for k in range(3)}) == 3
        empties += any(b == EMPTY and a != EMPTY and c != EMPTY for a, b, c in zip(scenes, scenes[1:], scenes[2:]))
        if s["cfg"]["progressive"]:
            progressive += 1
            assert any(a in FRAME_KINDS[:3] and b == "tiles" and c in FRAME_KINDS[:3]
                       for a, b, c in zip(kinds, kinds[1:], kinds[2:])), seed
    print("session fuzz: steps", min(lengths), "to", max(lengths), "sum", sum(lengths), "; pairs",
          min(adjacent[p] for p in PAIRS), "to", max(adjacent[p] for p in PAIRS), "; fewest of a kind on a stream",
          min(streams[k, s] for k in READ_KINDS for s in range(3)), "; empty", empties, "; progressive",
          progressive, "; refusals", dict(refusals))
    assert all(adjacent[p] >= 2 for p in PAIRS), [p for p in PAIRS if adjacent[p] < 2]
    assert all(streams[k, s] >= 1 for k in READ_KINDS for s in range(3))
    assert empties >= 8 and progressive >= 10
    assert 24 <= min(lengths) and max(lengths) <= 40
    assert all(refusals[w] >= 2 for w in sf.REFUSALS), refusals


@pytest.mark.parametrize("seed", range(SESSIONS))
def test_every_reading_step_is_checked_and_the_references_agree(oracle, seed):
    """Every reading step has an expectation, and the GPU test a check for its
    kind: the share left unchecked is zero.  And on every (scene, tree) the
    session queries, rebuilt trees included, the oracle's walk of the session's
    rays equals the brute force's first slot (test_query_fuzz_cpu.py's check)."""
    import test_gpu_session_fuzz as gpu_side
    assert set(gpu_side.CHECKS) == set(READ_KINDS)
    trees = set()
    for i, st, m in _walk(seed, oracle):
        if st["kind"] not in READ_KINDS:
            continue
        exp = expected(m, st, oracle)
        assert exp and all(v is not None or k == "point" for k, v in exp.items()), (i, st)
        if (m.seen, m.tree) in trees:
            continue
        trees.add((m.seen, m.tree))
        step = dict(kind="trace_nearest", stream=0)
        hit, t, sphere, _, _ = expected(m, step, oracle)["hits"]
        bt, bs, bc = expected(m, dict(kind="multi", stream=0, k=1), oracle)["answer"]
        assert np.array_equal(bc[:N_GOOD] == 1, hit[:N_GOOD]) and not bc[N_GOOD:].any()
        assert np.array_equal(bs[:, 0], sphere)
        assert np.array_equal(bt[:, 0].view(np.uint32), t.view(np.uint32))
        assert np.array_equal(expected(m, dict(kind="trace_any", stream=0), oracle)["hits"][0], hit)
        if m.seen == EMPTY:
            assert not hit.any()


@pytest.mark.parametrize("mutant", MUTANTS)
def test_a_wrong_model_gives_another_answer(oracle, mutant):
    """The mutation check: a model that breaks one rule of rt.h runs beside the
    true one.  In at least three sessions, the first reading step that reads
    state in which the two models differ (Model.state of its kind) has
    different expected answers: the sessions can see that class of stale
    state, from the references alone."""
    seen = []
    for seed in range(SESSIONS):
        wrong = _walk(seed, oracle, mutant)
        for (i, st, m), (_, _, w) in zip(_walk(seed, oracle), wrong):
            if st["kind"] not in READ_KINDS:
                continue
            a, b = expected(m, st, oracle), expected(w, st, oracle)
            differ = m.state(st["kind"]) != w.state(st["kind"])      # (after it: a frame may have restarted the sums)
            if differ:
                if not sf.same(a, b):
                    seen.append((seed, i, st["kind"]))
                break
            assert sf.same(a, b)
    print(mutant, "seen at (seed, step, kind):", seen)
    assert len(seen) >= 3, seen


def test_the_model_keeps_rt_h_rules(oracle):
    """The model on a hand-made sequence: equal bytes keep the sums, every other
    change restarts them, a query leaves them alone, a refused call changes
    nothing, and a resize sets the FOV-80 intrinsic."""
    s = next(session(seed) for seed in range(SESSIONS) if session(seed)["cfg"]["progressive"])
    m = Model(s)
    for st in s["steps"][:3]:
        m.apply(st, oracle)
    pose, K = m.pose, m.K
    frame, tiles_ = dict(kind="frame", stream=0), dict(kind="tiles", stream=0, mask=1)
    expected(m, frame, oracle)
    expected(m, dict(kind="frame_stats", stream=0), oracle)
    expected(m, dict(kind="multi", stream=0, k=4), oracle)
    expected(m, dict(kind="gbuffer", stream=0), oracle)
    assert len(m.history) == 2          # (a stats frame counts; queries and the G-buffer do not)
    m.apply(dict(kind="set_pose", cam=[c for c in range(3) if sf.camera(m.cfg, c)["pose"] is pose][0]), oracle)
    m.apply(dict(kind="refused", what="empty_box"), oracle)
    m.apply(dict(kind="refused", what="nan_scene", scene=0, depth=3, leaf=2, row=0), oracle)
    assert len(m.history) == 2 and m.pose is pose and m.K is K
    expected(m, tiles_, oracle)
    assert len(m.history) == 1 and m.pixset == ("tiles", (0,))
    expected(m, frame, oracle)
    assert len(m.history) == 1 and m.pixset == ("full",)
    for change in (dict(kind="set_pose", cam=0), dict(kind="set_pose", cam=1), dict(kind="set_intrinsic", cam=2),
                   dict(kind="resize_up", w=71, h=55), dict(kind="reset_accumulation"),
                   dict(kind="set_octree", root_min=(-0.1,) * 3, root_max=(1.3,) * 3, resolution=0.05),
                   dict(kind="set_scene_device", scene=EMPTY, depth=2, leaf=3)):
        before = m.state("frame_stats")
        m.apply(change, oracle)
        if m.state("frame_stats")[0] != before[0] or change["kind"] == "reset_accumulation":
            assert m.history == [], change
        expected(m, frame, oracle)
    assert (m.w, m.h) == (71, 55) and m.seen == EMPTY
    assert m.tree == ((0.0,) * 3, (1.28,) * 3, 2, 3)
    m.apply(dict(kind="resize_down", w=33, h=27), oracle)
    assert np.array_equal(m.K, oracle.resize_intrinsic(33, 27))
