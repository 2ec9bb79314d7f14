"""CPU tests of rt_guide_math.h, the arithmetic that the overlap, closest and
sweep queries share: the grown box of a point and
a reach, the root box's farthest corner and the finiteness test, bit for bit
against a numpy restatement of the formulas, and the three queries' wrappers
against what they are defined as.  The root boxes are those of scenes A, D, F
and G of test_overlap_cpu.py and test_closest_cpu.py.
"""
import os
import subprocess

import numpy as np
import pytest

import overlap_ref as ov
from bins_native import f32_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
# rt_overlap_math.h, rt_closest_math.h, rt_sweep_math.h: k*SlackM, and k*SlackR of the two boxes
SLACK_M = {"overlap": 64.0, "closest": 64.0, "sweep": 256.0}
REL = np.float32(1.0 + 32.0 * U)


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    """tests/native/guide_math_dump.cpp, a stand-alone program built with the
    address and undefined-behaviour sanitizers; a sanitizer report fails the test."""
    d = tmp_path_factory.mktemp("guide_math")
    exe = str(d / "guide_math_dump")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "guide_math_dump.cpp")])

    def run(*args):
        r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, r.stderr
        return r.stdout
    run.dir = d
    return run


@pytest.fixture(scope="module")
def roots(oracle):
    """{scene: (max_depth, rmin, rmax)}: the effective root boxes, f32, from the oracle"""
    out = {}
    for name in ("A", "D", "F", "G"):
        sc = oracle.Scene(ov.spheres(name), None, **ov.TREES[name])
        rmin, rmax = sc.root()
        sc.close()
        out[name] = (ov.TREES[name]["max_depth"], np.asarray(rmin, np.float32), np.asarray(rmax, np.float32))
    return out


def corner_far(rmin, rmax):
    """root_corner_far in numpy: f64, the three squares summed in axis order"""
    c = np.maximum(np.abs(rmin.astype(np.float64)), np.abs(rmax.astype(np.float64)))
    m2 = np.float64(0.0)
    for i in range(3):
        m2 = m2 + c[i] * c[i]
    return np.sqrt(m2)


def grown_box(p, reach, rel, rmin, rmax, depth, slack_m):
    """grown_box in numpy: (n, 6) f32 {lo[3], hi[3]}, every operation one f32
    operation in the header's order"""
    scale = np.float32(1 << depth) / (rmax - rmin)
    grow = (reach * rel + slack_m)[:, None]
    assert scale.dtype == grow.dtype == np.float32
    return np.concatenate([((p - grow) - rmin) * scale, ((p + grow) - rmin) * scale], axis=1)


@pytest.mark.parametrize("name", ["A", "D", "F", "G"])
def test_corner_and_the_three_slacks(dump, roots, name):
    """M bit for bit, and each query's slack_m = its constant * u * M rounded to
    f32 once."""
    _, rmin, rmax = roots[name]
    out = dump("corner", *f32_args(rmin), *f32_args(rmax)).split()
    m = corner_far(rmin, rmax)
    assert m > 0.0 and int(out[0], 16) == int(np.float64(m).view(np.uint64))
    for got, q in zip(out[1:], ("overlap", "closest", "sweep")):
        want = np.float32(SLACK_M[q] * U * m)
        assert int(got, 16) == int(want.view(np.uint32)), q


@pytest.mark.parametrize("name", ["A", "D", "F", "G"])
def test_grown_box_and_its_two_wrappers(dump, roots, name):
    """grown_box bit for bit on the scene's probe mix, each probe with its own
    radius and with R = 0, -0, +inf and a negative one; overlap_box is
    grown_box with R as the reach, closest_box with max(bound, 0)."""
    depth, rmin, rmax = roots[name]
    pr = ov.probes(name)[:128]
    odd = np.array([0.0, -0.0, np.inf, -1.5], np.float32)
    p = np.concatenate([pr[:, :3]] + [pr[:16, :3]] * len(odd))
    reach = np.concatenate([pr[:, 3]] + [np.full(16, r, np.float32) for r in odd])
    slack_m = np.float32(SLACK_M["overlap"] * U * corner_far(rmin, rmax))
    path = str(dump.dir / (name + ".f32"))
    np.ascontiguousarray(np.concatenate([p, reach[:, None]], axis=1), np.float32).tofile(path)
    rows = dump("box", depth, *f32_args(rmin), *f32_args(rmax), *f32_args(REL), *f32_args(slack_m), path)
    rows = [line.split() for line in rows.splitlines()]
    assert len(rows) == len(p)
    finite = np.array([[ch == "1" for ch in r[0]] for r in rows])
    assert np.array_equal(finite, np.isfinite(np.concatenate([p, reach[:, None]], axis=1)))
    got = np.array([[int(t, 16) for t in r[1:]] for r in rows], np.uint32).reshape(len(p), 3, 6)
    with np.errstate(invalid="ignore"):
        want = grown_box(p, reach, REL, rmin, rmax, depth, slack_m)
        want_closest = grown_box(p, np.where(reach > 0, reach, np.float32(0.0)), REL, rmin, rmax, depth, slack_m)
    assert np.array_equal(got[:, 0], want.view(np.uint32))
    assert np.array_equal(got[:, 1], want.view(np.uint32))
    assert np.array_equal(got[:, 2], want_closest.view(np.uint32))
    inf = reach == np.inf                        # the whole space
    assert inf.sum() == 16 and np.all(want[inf, :3] == -np.inf) and np.all(want[inf, 3:] == np.inf)
