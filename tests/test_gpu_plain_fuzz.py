"""The plain frame of every plain_fuzz.py case is the oracle's: plain frames
answer shadow rays from occluder lists and primary rays from screen-space
bins (DESIGN.md 5.1 rounds 7 and 10), stats frames walk, and the suite's other
fuzz tests render stats frames only.

Per seed, with test_gpu_bins' hooks (bins at every frame size and mean list
length) and the occluder lists at the product's rule: the plain frame(s) and a
stats frame against the oracle byte for byte, the stats frame's counters, and
the path the frame reports against the CPU model (plain_fuzz.model: csrc/
rt_bins_math.h run on the CPU).  The device runs the same f64 operations in
the same order, so `wide` and `entries` must be equal, not close.
"""
import json
import os

import numpy as np
import pytest

import raytracingstudy_amd as rt

from bins_native import build_dump
from plain_fuzz import SEEDS, model
from test_gpu_occluders import _cam_ratio, CAM_GATE

pytestmark = pytest.mark.gpu

# seed -> what the frame reported; the module's last test reads it
RECORD = {}


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    return build_dump(tmp_path_factory.mktemp("bin"))


@pytest.fixture
def hooks(monkeypatch):
    monkeypatch.setenv("RT_TEST_BIN_MIN_SAMPLES", "0")
    monkeypatch.setenv("RT_TEST_BIN_MEAN", "1000000")


def _same(r, frame, what):
    ref8, ref32, _ = frame
    assert np.array_equal(r.readback(), ref8), f"{what}: RGBA8 differs from the oracle"
    assert np.array_equal(r.readback_radiance(), ref32), f"{what}: radiance differs from the oracle"


@pytest.mark.parametrize("seed", range(SEEDS))
def test_plain_frame_is_the_oracles(gpu, oracle, hooks, dump, seed):
    m = model(seed, dump, oracle, hits=False)
    c, frames = m["case"], m["frames"]
    with rt.KernelRenderer(c["w"], c["h"], mode="scene", spp=c["spp"], radiance=True,
                           shadows=c["shadows"], jitter=c["jitter"], light_dir=c["light"],
                           ambient=c["ambient"], progressive=c["progressive"]) as r:
        r.resize(c["w"], c["h"])
        r.setIntrinsic(c["K"])
        r.setPosition(c["pose"])
        r.set_scene(c["sp"], c["al"], max_depth=c["depth"], leaf_capacity=c["leaf"])
        pose, K = r.camera()
        assert np.array_equal(K, c["K"]) and np.array_equal(pose, c["pose"])
        # plain frames: lists and bins (a progressive case: two, the sums carried over)
        for k, frame in enumerate(frames):
            r.render()
            bi = r.bin_info()
            _same(r, frame, f"plain frame {k}")
        info = r.scene_info()
        # the stats frame walks: the same bytes, and the oracle's counters
        if c["progressive"]:
            r.reset_accumulation()
        st = r.render(stats=True)
        _same(r, frames[0], "stats frame")
        assert (st.primary_rays, st.shadow_rays, st.nodes_visited, st.prims_tested) == tuple(
            int(x) for x in frames[0][2])
        assert r.bin_info()["reason"] == "kernel"
    RECORD[seed] = dict(seed=seed, n=c["n"], mode=c["mode"], spp=c["spp"], w=c["w"], h=c["h"],
                        reason=bi["reason"], wide=bi["wide"], entries=bi["entries"],
                        overflowed_bins=bi["overflowed_bins"], predicted=m["reason"],
                        predicted_wide=m["wide"], predicted_entries=m["entries"],
                        shadow_rays=int(frames[0][2][1]), lists_on=info["occluder_lists_on"],
                        in_gate=bool(_cam_ratio(c["pose"], info) <= CAM_GATE))
    # the path: the CPU model's, with its counts (a frame that built no bins reports none)
    assert bi["reason"] == m["reason"], (bi, m["reason"])
    if m["reason"] in ("on", "wide", "capacity"):
        assert bi["wide"] == m["wide"] and bi["entries"] == m["entries"], (bi, m["wide"], m["entries"])
        assert bi["overflowed_bins"] == int((m["counts"] > 64).sum())
        assert bi["non_empty_bins"] == int((m["counts"] > 0).sum())


def test_the_cases_see_unsound_bins(gpu, oracle, hooks, dump, monkeypatch):
    """Negative control: with the bins built from radii x 0.9 (the test hook
    RT_TEST_BIN_SHRINK) some case's plain frame is no longer the oracle's.
    Stops at the first such case."""
    monkeypatch.setenv("RT_TEST_BIN_SHRINK", "1")
    for seed in range(SEEDS):
        m = model(seed, dump, oracle, hits=False)
        c = m["case"]
        if m["reason"] != "on" or m["entries"] == 0:
            continue
        with rt.KernelRenderer(c["w"], c["h"], mode="scene", spp=c["spp"], radiance=True,
                               shadows=c["shadows"], jitter=c["jitter"], light_dir=c["light"],
                               ambient=c["ambient"], progressive=c["progressive"]) as r:
            r.resize(c["w"], c["h"])
            r.setIntrinsic(c["K"])
            r.setPosition(c["pose"])
            r.set_scene(c["sp"], c["al"], max_depth=c["depth"], leaf_capacity=c["leaf"])
            r.render()
            if not np.array_equal(r.readback_radiance(), m["frames"][0][1]):
                return
    pytest.fail("no case's frame changed under shrunken bins: the cases cannot see an unsound list")


def test_the_cases_ran_on_lists_and_without(gpu):
    """Of the cases that cast shadow rays, at least a third rendered their
    plain frame from occluder lists (the scene has them and the camera is
    inside the lists' gate), and at least two scenes were refused lists by the
    builder's scene rule.  Judged only when every seed ran in this process
    (the record above is filled by the per-seed test); a run of a subset
    checks nothing here.  With RT_PLAIN_FUZZ_RECORD set, the per-seed record
    is written to that file."""
    path = os.environ.get("RT_PLAIN_FUZZ_RECORD")
    if path:
        with open(path, "w") as f:
            for seed in sorted(RECORD):
                f.write(json.dumps(RECORD[seed]) + "\n")
    if len(RECORD) < SEEDS:
        return
    shadow = [v for v in RECORD.values() if v["shadow_rays"] > 0]
    used = [v for v in shadow if v["lists_on"] and v["in_gate"]]
    refused = [v for v in shadow if not v["lists_on"]]
    print(f"plain fuzz: {len(shadow)} shadow-casting cases, {len(used)} on lists, "
          f"{len(refused)} refused lists, {sum(v['lists_on'] and not v['in_gate'] for v in shadow)} outside the gate")
    assert 3 * len(used) >= len(shadow) > 0, (len(used), len(shadow))
    assert len(refused) >= 2, len(refused)
