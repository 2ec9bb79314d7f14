"""The frame of every pair_fuzz.py case is the oracle's, with pixel pairs and
without (DESIGN.md 5.1 rounds 26 and 27: a binned plain frame of 33 .. 64 spp
shades two pixels a wave pass; the placed scenes of test_gpu_pixel_pairs.py
are one camera and two frame sizes).

Per seed, under the case's own hooks (bin cap, occluder cap, ticket size,
dense flag): the frame with pairs and the frame with RT_FLAG_NO_PAIRS against
the oracle and against each other, RGBA8 byte for byte and radiance bit for
bit; the path the frame reports against the CPU model (pair_fuzz.model); and
whether the pair instance ran against a predicate written from the model and
the scene's reported state.  Then, over all seeds, what the pair instance met
(the record), a negative control under RT_TEST_BIN_SHRINK, and one renderer
led through pair and one-pixel frames.
"""
import ctypes
import json
import os

import numpy as np
import pytest

import raytracingstudy_amd as rt
from raytracingstudy_amd.camera import translation_pose

from bins_native import build_dump
from bins_oracle import look_at_pose
from pair_fuzz import BUILT, SEEDS, case_env, model
from test_gpu_frame_chain import _E1, _column_scene
from test_gpu_occluders import CAM_GATE, LIGHT, _cam_ratio
from test_gpu_pixel_pairs import BINS, OCC, PAIR, POSE, WALK, WAVEQ, _bits, _pair_scene

pytestmark = pytest.mark.gpu

# seed -> what the frame reported and met; the coverage test reads it
RECORD = {}


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    return build_dump(tmp_path_factory.mktemp("bin"))


def _set_env(monkeypatch, c, **more):
    for k, v in {**case_env(c), **more}.items():
        monkeypatch.setenv(k, v)


def _open(c, pairs=True):
    """The case's renderer (the hooks are read here), its camera and scene set."""
    r = rt.KernelRenderer(c["w"], c["h"], mode="scene", spp=c["spp"], radiance=True, shadows=c["shadows"],
                          jitter=c["jitter"], light_dir=c["light"], ambient=c["ambient"], pairs=pairs,
                          opt_off=c["ticket"] << 4)
    try:
        r.resize(c["w"], c["h"])
        r.setIntrinsic(c["K"])
        r.setPosition(c["pose"])
        r.set_scene(c["sp"], c["al"], max_depth=c["depth"], leaf_capacity=c["leaf"])
    except BaseException:
        r.close()
        raise
    return r


def _frame(r):
    return r.readback(), r.readback_radiance()


def _same(got, want, what):
    assert np.array_equal(got[0], want[0]), f"{what}: RGBA8 differs"
    assert np.array_equal(_bits(got[1]), _bits(want[1])), f"{what}: radiance differs"


def _centre_hits(r):
    """The sphere the pixel-centre ray of every pixel meets first, (h, w)
    uint32 (WALK: none): rt_render_gbuffer's hit records, into a device buffer
    of the HIP runtime's own."""
    hip = ctypes.CDLL("/opt/rocm/lib/libamdhip64.so")
    hits = np.zeros((r.height, r.width, 2), np.int32)      # rt_hit: {t, sphere}
    buf = ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(buf), ctypes.c_size_t(hits.nbytes)) == 0
    try:
        r.render_gbuffer_device(hits_ptr=buf.value)
        r.synchronize()
        assert hip.hipMemcpy(hits.ctypes.data_as(ctypes.c_void_p), buf, ctypes.c_size_t(hits.nbytes), 2) == 0
    finally:
        hip.hipFree(buf)
    return hits[..., 1].copy().view(np.uint32)


def _met(r, c, bi, info):
    """What the frame's pairs met, from the exported bins and occluder lists
    and the pixel centres' first hits."""
    out = dict(listed_bins=0, walk_bins=0, list_0=False, list_1=False, list_cap=False, walk_header=False,
               a_list_b_walk=0, a_walk_b_list=0)
    if bi["reason"] == "on":
        cnt = r.export_bins()[0][:, 1]
        out["listed_bins"] = int(((cnt != WALK) & (cnt > 0)).sum())
        out["walk_bins"] = int((cnt == WALK).sum())
    if info["occluder_lists_on"]:
        _, cnt, _, _ = r.export_occluders()
        g = _centre_hits(r)
        hit = g != WALK
        seen = cnt[g[hit]]
        walks = np.where(hit, cnt[np.where(hit, g, 0)] == WALK, False)
        lists = hit & ~walks
        even, odd = slice(0, c["w"] - 1, 2), slice(1, c["w"], 2)
        out.update(list_0=bool((seen == 0).any()), list_1=bool((seen == 1).any()),
                   list_cap=bool((seen == c["occ_cap"]).any()), walk_header=bool((seen == WALK).any()),
                   a_list_b_walk=int((lists[:, even] & walks[:, odd]).sum()),
                   a_walk_b_list=int((walks[:, even] & lists[:, odd]).sum()))
    return out


@pytest.mark.parametrize("seed", range(SEEDS))
def test_pair_frame_is_the_oracles(gpu, oracle, dump, monkeypatch, seed):
    m = model(seed, dump, oracle, hits=False)
    c, want = m["case"], m["frame"]
    _set_env(monkeypatch, c)
    out = []
    for pairs in (True, False):
        with _open(c, pairs) as r:
            pose, K = r.camera()
            assert np.array_equal(K, c["K"]) and np.array_equal(pose, c["pose"])
            r.render()
            out.append(_frame(r))
            bi, inst, info = r.bin_info(), r.last_instance(), r.scene_info()
            # the path: the CPU model's, with its counts (a frame that built no bins reports none)
            assert bi["reason"] == m["reason"], (pairs, bi, m["reason"])
            if m["reason"] in BUILT:
                assert bi["wide"] == m["wide"] and bi["entries"] == m["entries"], (bi, m["wide"], m["entries"])
                assert bi["overflowed_bins"] == int(m["over"].sum())
                assert bi["non_empty_bins"] == int((m["counts"] > 0).sum())
            # the instance: pairs iff the frame built bins (whatever its device flag then says:
            # "dense", "wide" and "capacity" frames run the instance and walk), casts shadow rays,
            # the scene has occluder lists and the camera is inside their gate
            in_gate = bool(_cam_ratio(c["pose"], info) <= CAM_GATE)
            expect = m["reason"] in BUILT and c["shadows"] and bool(info["occluder_lists_on"]) and in_gate
            assert bool(inst & PAIR) == (pairs and expect), (pairs, hex(inst), bi["reason"], info, in_gate)
            if pairs:
                RECORD[seed] = dict(seed=seed, n=c["n"], mode=c["mode"], spp=c["spp"], w=c["w"], h=c["h"],
                                    bin_cap=c["bin_cap"], occ_cap=c["occ_cap"], ticket=c["ticket"],
                                    shadows=c["shadows"], reason=bi["reason"], wide=bi["wide"],
                                    entries=bi["entries"], overflowed_bins=bi["overflowed_bins"],
                                    instance=inst, pair=bool(inst & PAIR),
                                    # the frame shaded pixel pairs: the instance has the path, the device
                                    # flag is clear, and a ticket holds two wave tiles or more (a ticket
                                    # of one never pairs, and at these sizes the auto ticket is one tile)
                                    paired=bool(inst & PAIR) and bi["reason"] == "on" and c["ticket"] >= 2,
                                    lists_on=info["occluder_lists_on"],
                                    in_gate=in_gate, **_met(r, c, bi, info))
        _same(out[-1], want, f"pairs {pairs} / oracle")
    _same(out[0], out[1], "pairs on / off")


def test_the_cases_ran_pairs_beside_their_fallbacks(gpu):
    """Of the cases that shaded pixel pairs (the pair instance under a ticket of
    two wave tiles or more, the frame's device flag clear; reached on the
    MI355X | floor):

      shaded pairs                                               50 | >= 30
      a visible sphere whose shadow rays walk beside a listed
      one inside a pair (x even, x + 1)                          16 | >=  8
      ... A listed, B walks                                      11 | >=  3
      ... A walks, B listed                                      13 | >=  3
      a visible sphere with a list of exactly the case's cap     18 | >=  8

    The pair instance also ran, and shaded no pair, in 39 controls: 17 under a
    ticket of one tile (forced, or the auto ticket at these frame sizes) and 22
    frames whose device flag says dense or wide.

    Conditions on the distribution: where one fails, move pair_case (the
    occluder caps, the cluster share), not the floor.  Judged only when every
    seed ran in this process (the per-seed test fills the record); a run of a
    subset checks nothing here.  With RT_PAIR_FUZZ_RECORD set, the per-seed
    record is written to that file."""
    path = os.environ.get("RT_PAIR_FUZZ_RECORD")
    if path:
        with open(path, "w") as f:
            for seed in sorted(RECORD):
                f.write(json.dumps(RECORD[seed]) + "\n")
    if len(RECORD) < SEEDS:
        return
    inst = sum(v["pair"] for v in RECORD.values())
    ran = [v for v in RECORD.values() if v["paired"]]
    lw = sum(v["a_list_b_walk"] > 0 for v in ran)
    wl = sum(v["a_walk_b_list"] > 0 for v in ran)
    mix = sum(v["a_list_b_walk"] > 0 or v["a_walk_b_list"] > 0 for v in ran)
    cap = sum(v["list_cap"] for v in ran)
    print(f"pair fuzz: {inst} cases ran the pair instance, {len(ran)} shaded pairs; of those: "
          f"walk beside list in a pair {mix} "
          f"(A list / B walk {lw}, A walk / B list {wl}); a visible list of exactly the cap {cap}; "
          f"listed beside walk bins {sum(v['listed_bins'] > 0 and v['walk_bins'] > 0 for v in ran)}")
    assert len(ran) >= 30, len(ran)
    assert mix >= 8 and lw >= 3 and wl >= 3, (mix, lw, wl)
    assert cap >= 8, cap


def test_the_cases_see_unsound_bins_through_pairs(gpu, oracle, dump, monkeypatch):
    """Negative control: with the bins built from radii x 0.9 (the test hook
    RT_TEST_BIN_SHRINK) some case's frame, shaded by the pair instance under a
    ticket of two wave tiles or more, is no longer the oracle's: an unsound tile
    word reaches the comparison through the pair path.  Stops at the first
    such case."""
    for seed in range(SEEDS):
        m = model(seed, dump, oracle, hits=False)
        c = m["case"]
        if not m["pairable"] or m["entries"] == 0 or c["ticket"] < 2:
            continue
        _set_env(monkeypatch, c, RT_TEST_BIN_SHRINK="1")
        with _open(c) as r:
            r.render()
            if r.last_instance() & PAIR and not np.array_equal(_bits(r.readback_radiance()), _bits(m["frame"][1])):
                return
    pytest.fail("no case's pair frame changed under shrunken bins: the cases cannot see an unsound tile word")


def _walk_camera(sp, k=20):
    """Beside the column, facing sphere k from 0.5 away: with _walk_zoom the
    71x45 image holds a few spheres around k, whose lists (the spheres before
    them in the column) are all over a cap of 1."""
    c = sp[k, :3].astype(np.float64)
    return look_at_pose(c + 0.5 * _E1, c)


_WALK_ZOOM = 4.0


def test_one_renderer_through_pair_and_one_pixel_frames(gpu, oracle, monkeypatch):
    """One renderer at 48 spp (tickets of 4 wave tiles, an occluder cap of 1),
    each frame against the oracle bit for bit and its instance checked: sizes
    with an odd and an even width, one pixel wide and one high (windows of the
    first frame, and at FOV 80, which the bins' camera gate refuses), a camera
    outside the occluder lists' gate, a scene whose visible spheres all walk,
    and a stats frame.  Stale tile words, a stale "B is on the image" or a
    plan kept across a resize would show."""
    monkeypatch.setenv("RT_TEST_BIN_MIN_SAMPLES", "0")
    monkeypatch.setenv("RT_TEST_BIN_MEAN", "1000000")
    monkeypatch.setenv("RT_TEST_BIN_CAP", "5")
    monkeypatch.setenv("RT_TEST_OCC_CAP", "1")
    spp = 48
    pairs_scene, column = _pair_scene(71, 45), _column_scene()
    orc = {"pairs": oracle.Scene(*pairs_scene), "column": oracle.Scene(*column)}
    FULL = WAVEQ | OCC | BINS | PAIR
    far = translation_pose(0.64, 0.64, 30.0)

    with rt.KernelRenderer(71, 45, mode="scene", spp=spp, radiance=True, light_dir=LIGHT, opt_off=3 << 4) as r:
        state = {"scene": "pairs", "n": 0}

        def size(w, h):
            r.resize(w, h)

        def crop(x0, y0):
            """The 71x45 frame's camera moved to that frame's pixel (x0, y0): this
            frame is a window of it (the placed spheres of row 20 in view)."""
            K = np.array(rt.resize_intrinsic(71, 45), np.float32).copy()
            K[0, 2] -= x0
            K[1, 2] -= y0
            r.setIntrinsic(K)

        def scene(name):
            r.set_scene(*(pairs_scene if name == "pairs" else column))
            state["scene"] = name

        def frame(pair, stats=False):
            """Render; the frame is the oracle's of the renderer's own camera."""
            state["n"] += 1
            what = f"frame {state['n']} ({r.width}x{r.height}, {state['scene']})"
            r.render(stats=stats)
            got, inst = _frame(r), r.last_instance()
            pose, K = r.camera()
            want = orc[state["scene"]].render(r.width, r.height, pose, K, spp=spp)
            _same(got, want, what)
            if pair:
                assert inst == FULL and r.bin_info()["reason"] == "on", (what, hex(inst))
            else:
                assert inst & PAIR == 0, (what, hex(inst))

        size(71, 45)
        r.setPosition(POSE)
        scene("pairs")
        frame(True)
        size(70, 44)
        frame(True)                              # an even width
        size(1, 9)
        frame(False)                             # (at FOV 80 a frame this narrow is outside the bins' camera gate)
        assert r.bin_info()["reason"] == "camera"
        crop(12, 16)
        frame(True)                              # every pair's B off the image; a bin of exactly the cap
        size(9, 1)
        crop(8, 20)
        frame(True)
        size(71, 45)
        frame(True)
        r.setPosition(far)
        frame(False)                             # outside the lists' gate: the shadow rays walk
        assert r.last_instance() & OCC == 0
        r.setPosition(POSE)
        frame(True)
        # a scene whose visible spheres all have walk headers: every pair falls back
        scene("column")
        r.setPosition(_walk_camera(column[0]))
        K = np.array(rt.resize_intrinsic(71, 45), np.float32).copy()
        K[0, 0] *= _WALK_ZOOM
        K[1, 1] *= _WALK_ZOOM
        r.setIntrinsic(K)
        frame(True)
        _, cnt, _, _ = r.export_occluders()
        g = _centre_hits(r)
        assert (g != WALK).sum() > 50 and np.all(cnt[g[g != WALK]] == WALK)
        frame(True)
        scene("pairs")
        r.setPosition(POSE)
        r.setIntrinsic(rt.resize_intrinsic(71, 45))
        frame(True)
        frame(False, stats=True)                 # a stats frame walks, between two plain frames
        frame(True)
    for s in orc.values():
        s.close()
