"""The plain-frame fuzz cases (plain_fuzz.py) on the CPU, before a GPU sees
them: csrc/rt_bins_math.h's rectangles hold every oracle primary hit under the
cases' own intrinsics (anisotropic, negated, off-centre), radii (three
decades) and spheres outside the root box; and the 64 cases together reach
the paths they are for (the coverage table below), judged from the CPU model
alone: the rectangles' classes and per-bin counts, and the oracle's hits and
ray counters.
"""
import numpy as np
import pytest

from bins_native import BINNED, DROPPED, WIDE, build_dump
from plain_fuzz import BIN, BIN_CAP, MODES, SEEDS, SPPS, model


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    return build_dump(tmp_path_factory.mktemp("bin"))


@pytest.mark.parametrize("seed", range(SEEDS))
def test_oracle_primary_hits_lie_in_the_rectangles(dump, oracle, seed):
    """Every oracle primary hit (pixel, sphere, t) of the pixel-centre rays
    names a sphere that is not dropped, lies inside that sphere's rectangle
    when it is binned, and has t >= its near bound."""
    m = model(seed, dump, oracle)
    x, y, j, t = m["hits"]
    if x.shape[0] == 0:
        return
    cls, r = m["cls"][j], m["rect"][j]
    assert np.all(m["in_tree"][j])
    assert np.all(cls != DROPPED), f"{int((cls == DROPPED).sum())} hits on dropped spheres"
    inside = (r[:, 0] <= x) & (x <= r[:, 2]) & (r[:, 1] <= y) & (y <= r[:, 3])
    b = cls == BINNED
    assert np.all(inside[b]), f"{int((~inside[b]).sum())} hits outside their sphere's rectangle"
    assert np.all(t >= m["near"][j]), "a hit nearer than its sphere's near bound"


def test_the_cases_reach_the_paths(dump, oracle):
    """Conditions on the distribution, not on the product: where one fails,
    change plain_case or add seeds, never the floors.

      bins on and a binned sphere is hit                        >= 40
      bins on, some non-empty bins over the cap of 64, some not >=  8
      the frame-level wide fallback (more than 32 wide spheres) >=  4
      bins on and a wide-list sphere is hit                     >=  6
      frames that cast shadow rays                              >= 32
      every spp value and every camera mode                     >=  3 each
      progressive cases                                         >=  6
    """
    got = dict(binned_hit=0, mixed_cap=0, wide_frame=0, wide_hit=0, shadow=0, progressive=0, hits=0)
    spps = dict.fromkeys(SPPS, 0)
    modes = dict.fromkeys(MODES, 0)
    for seed in range(SEEDS):
        m = model(seed, dump, oracle)
        c = m["case"]
        _, _, j, _ = m["hits"]
        on = m["reason"] == "on"
        ne = m["counts"][m["counts"] > 0]
        got["hits"] += j.shape[0]
        got["binned_hit"] += on and bool(np.any(m["cls"][j] == BINNED))
        got["mixed_cap"] += on and bool(np.any(ne > BIN_CAP)) and bool(np.any(ne <= BIN_CAP))
        got["wide_frame"] += m["reason"] == "wide"
        got["wide_hit"] += on and bool(np.any(m["cls"][j] == WIDE))
        got["shadow"] += int(m["frames"][0][2][1]) > 0
        got["progressive"] += c["progressive"]
        spps[c["spp"]] += 1
        modes[c["mode"]] += 1
        assert m["counts"].shape == ((c["h"] + BIN - 1) // BIN, (c["w"] + BIN - 1) // BIN)
    print("plain fuzz coverage:", got, spps, modes)
    assert got["binned_hit"] >= 40, got
    assert got["mixed_cap"] >= 8, got
    assert got["wide_frame"] >= 4, got
    assert got["wide_hit"] >= 6, got
    assert got["shadow"] >= 32, got
    assert got["progressive"] >= 6, got
    assert min(spps.values()) >= 3, spps
    assert min(modes.values()) >= 3, modes
