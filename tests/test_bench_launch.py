"""bench.py's `--gpus N` contract (CPU): N GPUs are
measured whichever way the bench is launched, a launch that cannot measure N
GPUs exits non-zero, and an N>1 line carries PMC roofs projected from the
N=1 counters."""
import json
import os
import subprocess
import sys

import pytest

import bench
import raytracingstudy_amd as rt
from raytracingstudy_amd._lib import kernel_source_id

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PMC = os.path.join(ROOT, "profiles", "pmc_latest.json")


def test_launch_mode_table():
    lm = bench.launch_mode
    assert lm(1, False, {}) == ("single", None)
    assert lm(8, False, {}) == ("native", None)          # no launcher, N > 1: one process
    assert lm(1, True, {}) == ("native", None)           # forced native at N = 1
    assert lm(8, False, {"WORLD_SIZE": "8"}) == ("torchrun", None)
    assert lm(1, False, {"WORLD_SIZE": "1"}) == ("single", None)
    mode, why = lm(8, False, {"WORLD_SIZE": "4"})
    assert mode is None and "WORLD_SIZE=4" in why
    mode, why = lm(2, True, {"WORLD_SIZE": "2"})
    assert mode is None and "without torchrun" in why
    assert lm(0, False, {})[0] is None


def _run_bench(args, env_extra):
    env = dict(os.environ)
    env.update(env_extra)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env,
                          capture_output=True, text=True, timeout=240)


def test_world_size_mismatch_exits_nonzero():
    """--gpus 4 under a world of 2: exit 2 before anything touches a GPU."""
    p = _run_bench(["--gpus", "4"], {"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert p.returncode == 2, p.stderr
    assert "WORLD_SIZE=2" in p.stderr and not p.stdout.strip()


def test_more_gpus_than_visible_exits_nonzero():
    """--gpus N without a launcher takes the native path, which refuses N >
    visible devices (this container sees none)."""
    n = rt.device_count() + 3
    env_clean = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n),
                        "--config", "c2", "--steps", "1", "--warmup", "0"],
                       env=env_clean, capture_output=True, text=True, timeout=240)
    assert p.returncode == 2, (p.returncode, p.stderr[-2000:])
    assert "visible" in p.stderr and not p.stdout.strip()


def test_full_is_off_by_default():
    assert bench.parse([]).full is False and bench.parse([]).dump_outputs == ""
    a = bench.parse(["--full", "--dump-outputs", "d"])
    assert a.full is True and a.dump_outputs == "d"


def test_dump_outputs_writes_float32_frame_within_budget(tmp_path):
    """--dump-outputs: a frame is written whole as float32 (height, width, 4);
    one over the 64 MB budget as the same seeded pixel sample every time."""
    import numpy as np
    w, h = 7, 5
    fr = (np.arange(w * h * 4) * 37 % 256).astype(np.uint8)
    bench.dump_outputs(str(tmp_path / "a"), fr, w, h)
    a = np.load(tmp_path / "a" / "frame.npy")
    assert a.dtype == np.float32 and a.shape == (h, w, 4)
    assert np.array_equal(a.reshape(-1), fr.astype(np.float32))
    w, h = 3840, 2160  # C4: 133 MB as float32
    big = (np.arange(w * h * 4, dtype=np.uint32) * 2654435761 >> 24).astype(np.uint8)
    bench.dump_outputs(str(tmp_path / "b"), big, w, h)
    bench.dump_outputs(str(tmp_path / "c"), big, w, h)
    b = np.load(tmp_path / "b" / "frame.npy")
    assert b.dtype == np.float32 and b.shape[1] == 4 and b.nbytes <= 64 << 20
    assert np.array_equal(b, np.load(tmp_path / "c" / "frame.npy"))
    idx = np.sort(np.random.default_rng(bench.DUMP_SAMPLE_SEED).choice(w * h, b.shape[0], replace=False))
    assert np.array_equal(b, big.reshape(-1, 4)[idx].astype(np.float32))


@pytest.mark.gpu
def test_plain_run_prints_headline_and_dumps_last_frame(gpu, tmp_path):
    """A plain `--gpus 1` run prints the headline line alone (what moved behind
    --full is absent) and --dump-outputs holds the frame the timed path
    rendered: the same bytes one renderer gives for the config."""
    import numpy as np
    from raytracingstudy_amd.camera import scene_pose
    p = _run_bench(["--gpus", "1", "--config", "c2", "--steps", "3", "--warmup", "1",
                    "--dump-outputs", str(tmp_path)], {})
    assert p.returncode == 0, p.stderr[-3000:]
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert line["unit"] == "Mrays/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    c = rt.CONFIGS["c2"]
    rays = line["config"]["rays_per_frame"]
    assert line["value"] == pytest.approx(rays / line["ms_per_step"] / 1e3, rel=1e-3)
    assert line["cpu_baseline"] is None
    assert "roofline" not in line and "secondary" not in line
    assert "scene_rebuild_ms" not in line["config"]
    sp, al = rt.configs.scene_spheres(c, rt.SEED)
    with rt.KernelRenderer(c.width, c.height, mode="scene", spp=c.spp, device=0,
                           light_dir=rt.configs.LIGHT_DIR, ambient=rt.configs.AMBIENT) as r:
        r.resize(c.width, c.height)
        r.setPosition(scene_pose())
        r.set_scene(sp, al, max_depth=c.max_depth, leaf_capacity=c.leaf_capacity)
        r.render()
        ref = r.readback()
    got = np.load(tmp_path / "frame.npy")
    assert got.dtype == np.float32 and got.shape == (c.height, c.width, 4)
    assert np.array_equal(got, ref.reshape(c.height, c.width, 4).astype(np.float32))


def _c3_pmc():
    with open(PMC) as f:
        return json.load(f)["c3"]


def test_projected_pmc_scales_counts_and_keeps_fractions():
    ent = _c3_pmc()
    p = bench.project_pmc(ent, 0.125, "note")
    assert p["projected"] == "note"
    for k in bench.PMC_PER_LAUNCH:
        if ent.get(k) is not None:
            assert p[k] == pytest.approx(ent[k] * 0.125)
    assert p["sq"]["SQ_INSTS_VALU"] == pytest.approx(ent["sq"]["SQ_INSTS_VALU"] * 0.125)
    assert p["sq"].get("GRBM_GUI_ACTIVE") == ent["sq"].get("GRBM_GUI_ACTIVE")
    for k in ("td_busy_frac", "ta_busy_frac", "valu_lane_util", "effective_clock_ghz"):
        assert p.get(k) == ent.get(k)
    assert ent.get("projected") is None  # the source entry is untouched


def test_n_gt_1_line_carries_projected_binding_unit_and_waste():
    """a rank's launch of 1/2 of the C3 frame (the gloo
    world-2 rehearsal's shape) prices its own bytes over its own time and
    names the binding unit and the waste from the projected counters."""
    cfg = rt.CONFIGS["c3"]
    pmc, note = bench.pmc_for_launch(PMC, cfg, 2, kernel_source_id(), 0.5)
    assert pmc is not None and note == "projected", note
    ent = _c3_pmc()
    kern_ms = ent["scene_kernel_avg_ns"] / 1e6 / 2  # half the frame in half the time
    touched = 191.32e9 / 2
    r = bench.roofline(kern_ms, touched, pmc, 1024)
    assert "projected from the N=1 counters of c3" in r["pmc_projected"]
    assert r["binding_unit"]["unit"] in ("vmem_return", "valu_issue", "scalar_issue")
    full = bench.roofline(kern_ms * 2, touched * 2, ent, 1024)
    # half the work in half the time: the same waste, unit and fraction as N = 1
    assert r["waste"] == pytest.approx(full["waste"], rel=1e-6)
    assert r["binding_unit"]["unit"] == full["binding_unit"]["unit"]
    assert r["frac"] == pytest.approx(full["frac"], rel=1e-6)
    # at N = 1 with the whole frame the measured entry itself is used
    same, why = bench.pmc_for_launch(PMC, cfg, 1, kernel_source_id(), 1.0)
    assert why == "ok" and "projected" not in same
