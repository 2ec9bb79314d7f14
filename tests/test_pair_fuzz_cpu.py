"""The pixel-pair fuzz cases (pair_fuzz.py) on the CPU, before a GPU sees
them, judged on the reference alone: the 96 cases together reach the pair
path and its fallbacks (the coverage table below), and the oracle's frames of
the cases can show the faults that path can have: a wrong valid-lane count, a
wrong A / B store, a wrong occluder loop.
"""
import numpy as np
import pytest

from bins_native import WIDE, build_dump
from pair_fuzz import SEEDS, SPPS, TICKETS, model, oracle_frame
from plain_fuzz import BIN, oracle_scene


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    return build_dump(tmp_path_factory.mktemp("bin"))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_the_cases_reach_the_paths(dump, oracle):
    """Conditions on the distribution, not on the product: where one fails,
    change pair_case or add seeds, never the floors.  Reached by the 96 seeds
    (`pairable`: the model's reason is "on", shadow rays, no far camera, and a
    forced ticket of two wave tiles or more: the cases that shade pairs):

      pairable                                                   50   >= 34
      pairable, a listed non-empty bin and a bin over the cap    17   >= 14
      pairable, every non-empty bin over the cap                 11   >=  2
      pairable, a wide-list sphere among the oracle's hits       16   >=  5
      pairable, odd width                                        30   >= 14
      ... with an oracle hit in column w - 1 (B off the image)   18   >= 10
      pairable, w <= 8                                            6   >=  4
      every spp value                                             9   >=  5 each
      every ticket setting                                       12   >=  8 each
    """
    got = dict(pairable=0, mixed_cap=0, all_over=0, wide_hit=0, odd=0, odd_last_hit=0, narrow=0, on=0)
    spps = dict.fromkeys(SPPS, 0)
    tickets = dict.fromkeys(TICKETS, 0)
    for seed in range(SEEDS):
        m = model(seed, dump, oracle)
        c = m["case"]
        x, _, j, _ = m["hits"]
        ne = m["counts"] > 0
        spps[c["spp"]] += 1
        tickets[c["ticket"]] += 1
        assert m["counts"].shape == ((c["h"] + BIN - 1) // BIN, (c["w"] + BIN - 1) // BIN)
        got["on"] += m["reason"] == "on"
        if not m["pairable"]:
            continue
        got["pairable"] += 1
        got["mixed_cap"] += bool(np.any(ne & m["over"])) and bool(np.any(ne & ~m["over"]))
        got["all_over"] += bool(ne.any()) and bool(np.all(m["over"][ne]))
        got["wide_hit"] += bool(np.any(m["cls"][j] == WIDE))
        got["odd"] += c["w"] % 2
        got["odd_last_hit"] += bool(c["w"] % 2 and np.any(x == c["w"] - 1))
        got["narrow"] += c["w"] <= 8
    print("pair fuzz coverage:", got, spps, tickets)
    assert got["pairable"] >= 34, got
    assert got["mixed_cap"] >= 14, got
    assert got["all_over"] >= 2, got
    assert got["wide_hit"] >= 5, got
    assert got["odd"] >= 14, got
    assert got["odd_last_hit"] >= 10, got
    assert got["narrow"] >= 4, got
    assert min(spps.values()) >= 5, spps
    assert min(tickets.values()) >= 8, tickets


def test_the_oracles_frames_show_the_faults(dump, oracle):
    """For every pairable case, from oracle frames only: the radiance at
    spp - 1 is not that at spp (a wrong count of valid lanes shows), and for
    w >= 2 the frame with columns 2k and 2k + 1 swapped is not the frame (a
    wrong A / B store shows).  In at least 20 pairable cases the radiance
    without shadow rays differs from the case's own (a wrong occluder loop
    shows), in at least 10 in an even and in an odd column (reached: 26 and
    25)."""
    shadowed, both = 0, 0
    for seed in range(SEEDS):
        m = model(seed, dump, oracle, hits=False)
        if not m["pairable"]:
            continue
        c, ref = m["case"], _bits(m["frame"][1])
        s = oracle_scene(oracle, c)
        fewer = _bits(oracle_frame(s, c, spp=c["spp"] - 1)[1])
        unlit = _bits(oracle_frame(s, c, shadows=False)[1])
        s.close()
        assert not np.array_equal(fewer, ref), f"seed {seed}: {c['spp'] - 1} spp renders as {c['spp']} spp"
        if c["w"] >= 2:
            swap = np.arange(c["w"])
            k = c["w"] // 2 * 2
            swap[:k] = swap[:k].reshape(-1, 2)[:, ::-1].reshape(-1)
            assert not np.array_equal(ref[:, swap], ref), f"seed {seed}: swapped columns render the same"
        cols = np.any(unlit != ref, axis=(0, 2))
        shadowed += bool(cols.any())
        both += bool(cols[0::2].any() and cols[1::2].any())
    print(f"pair fuzz: shadow rays change {shadowed} pairable cases, {both} in an even and an odd column")
    assert shadowed >= 20, shadowed
    assert both >= 10, both
