"""The pixel pairs' rule (csrc/rt_sched.h: pair_starts, and the plan's choice
of the pair instance) on the CPU: a stand-alone
sanitized program (tests/native/pair_rule_dump.cpp) walks a slot's tickets as
the frame kernel's loop does."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIR, BIN_, OCC, WAVEQ, PROG, STATS = 128, 64, 32, 8, 4, 2
NO_PAIRS = 1 << 8


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pair_rule") / "pair_rule_dump")
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "pair_rule_dump.cpp")])

    def run(*args):
        r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, r.stderr
        return r.stdout
    return run


# odd and even widths, edge blocks (no multiple of 8), a full block, one column
GRIDS = [(8, 8), (7, 5), (6, 8), (1, 3), (2, 1), (13, 9), (14, 12), (64, 64), (63, 45), (62, 44), (57, 64)]
# the pair fuzz's narrow frames (tests/pair_fuzz.py SMALL_W: each side of one bin), heights from 1
GRIDS += [(1, 1), (1, 9), (2, 7), (3, 1), (3, 8), (7, 9), (8, 1), (9, 1), (9, 8), (9, 17), (15, 3), (17, 9)]


# (a block slot, ks = 6, holds 8x8 wave tiles; a superblock slot 64x64)
SLOTS = [(gw, gh, ks) for gw, gh in GRIDS for ks in (6, 12) if ks == 12 or (gw <= 8 and gh <= 8)]


@pytest.mark.parametrize("chunk", [1, 2, 4, 8])       # (8: the option field's largest, a block's row)
@pytest.mark.parametrize("gw,gh,ks", SLOTS)
def test_pairs_cover_a_slot_once(dump, gw, gh, chunk, ks):
    seen, pairs, singles = {}, 0, 0
    for line in dump(gw, gh, chunk, ks).splitlines():
        kind, wx, wy = line.split()
        wx, wy = int(wx), int(wy)
        assert wx < gw and wy < gh                      # a unit never starts on padding
        tiles = [(wx, wy)]
        if kind == "P":
            pairs += 1
            assert wx % 2 == 0                          # A is the even pixel ..
            assert (wx + 1) // 8 == wx // 8             # .. and B lies in A's bin, on A's row
            if wx + 1 < gw:
                tiles.append((wx + 1, wy))
        else:
            assert kind == "S"
            singles += 1
        for t in tiles:
            seen[t] = seen.get(t, 0) + 1
    assert sorted(seen) == [(x, y) for x in range(gw) for y in range(gh)]
    assert set(seen.values()) == {1}
    if chunk == 1:
        assert pairs == 0 and singles == gw * gh        # a ticket of one tile never pairs
    else:
        assert singles == 0 and pairs == ((gw + 1) // 2) * gh


def test_the_plan_chooses_the_pair_instance(dump):
    def flags(spp, opt=0, occ=1, bins=1, prog=0, stats=0):
        return int(dump("plan", spp, opt, occ, bins, prog, stats))
    for spp in (33, 48, 64):
        assert flags(spp) == WAVEQ | OCC | BIN_ | PAIR
        assert flags(spp, opt=NO_PAIRS) == WAVEQ | OCC | BIN_
        for k in (1, 2, 3, 4):                                          # (a ticket size changes nothing)
            assert flags(spp, opt=k << 4) == WAVEQ | OCC | BIN_ | PAIR
        assert flags(spp, occ=0) == WAVEQ | BIN_
        assert flags(spp, bins=0) == WAVEQ | OCC
        assert flags(spp, stats=1) & (PAIR | BIN_ | OCC) == 0
    assert flags(64, prog=1) == WAVEQ | OCC | BIN_ | PROG
    for spp in (1, 4, 16, 32, 65, 128, 256):                            # more pixels a wave, or more rounds
        assert flags(spp) & PAIR == 0
