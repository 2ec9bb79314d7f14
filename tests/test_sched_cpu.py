"""How a scene frame is scheduled (csrc/rt_sched.h), on the CPU: which kernel
instance runs it, its wave-tile grid and its workgroup's LDS layout.
tests/native/sched_dump.cpp, built with the address and undefined-behaviour
sanitizers, prints the header's answers; the expected ones are written out
here independently: the dispatch table of the round-13 issue, closed forms of
the grid, and the LDS sizes as the launchers computed them before round 13.
"""
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LANE_UNIFIED, LANE_UNIFIED_2, WAVEQ, WAVEQ_LOW = 7, 10, 13, 4       # kVariant*
STATS, PROG, WQ, SORTED, OCC, BIN = 2, 4, 8, 16, 32, 64            # FrameFlag (kFTiles = 1: the launcher's)
TREES = [(0, 1), (0, 12), (4, 8), (7, 12)]                         # (tab_k, stack_depth)
SORT_WAVE_BYTES = 256 * 8 + 3 * 256 + 64 * 4                       # kSortWaveBytes
LEAF_BUF_BYTES = 4 * 32 * 16                                       # kLeafBufBytes


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bin") / "sched_dump")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "sched_dump.cpp")])

    def run(cmd, rows):
        text = "".join(" ".join(str(int(x)) for x in row) + "\n" for row in rows)
        r = subprocess.run([exe, cmd], input=text, capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, r.stderr   # a sanitizer report fails the test
        out = [tuple(int(t) for t in line.split()) for line in r.stdout.splitlines()]
        assert len(out) == len(rows)
        return out
    return run


def _levels(tab_k, depth, no_stack=False):
    if no_stack and tab_k:
        return 0
    sb = tab_k - 1 if tab_k else 0
    return depth - 1 - sb if depth > 1 + sb else 1


def _scene_lds_bytes(tab_k, depth):      # the launcher's scene_lds_bytes before round 13
    return 256 * 16 + _levels(tab_k, depth) * 256 * 8 + LEAF_BUF_BYTES


def _sort_lds_bytes(tab_k, depth):       # ... and its sort_lds_bytes
    return _levels(tab_k, depth, True) * 256 * 8 + 4 * SORT_WAVE_BYTES + LEAF_BUF_BYTES


# ---- the instance a frame runs -------------------------------------------------

def _expected(variant, spp, prog, count, sort_on, occ, bins, tab_k, depth):
    """The issue's table, first match wins -> (waveq, stats, sorted, occ, bin, min_waves)."""
    v = variant or (WAVEQ if spp >= 8 else WAVEQ_LOW)
    rounds = -(-spp // 64)
    wave_queue = lambda srt: (1, 1, srt, 0, 0, 7) if count else (1, 0, srt, occ, bins, 8)
    block_tile = lambda stats: (0, 1, 0, 0, 0, 1) if stats else (0, 0, 0, occ, 0, 1)
    if (sort_on and spp >= 8 and min(spp, 64) == 64 and 2 <= rounds <= 4 and
            8 * _sort_lds_bytes(tab_k, depth) <= 160 * 1024 and (prog or v == WAVEQ)):
        return wave_queue(1)
    if prog:
        return wave_queue(0) if spp >= 8 else block_tile(count)
    if v == LANE_UNIFIED:
        return block_tile(True)          # counts in every frame
    if v == LANE_UNIFIED_2:
        return block_tile(count)
    assert v in (WAVEQ, WAVEQ_LOW)
    return wave_queue(0)


def test_pick_scene_instance_is_the_dispatch_table(dump):
    rows = [(v, spp, *b, *tree)
            for v in (0, LANE_UNIFIED, LANE_UNIFIED_2, WAVEQ, WAVEQ_LOW)
            for spp in (1, 4, 7, 8, 63, 64, 65, 128, 256, 257, 320)
            for b in itertools.product((0, 1), repeat=5)      # progressive, count_work, sort_on, occ, bins
            for tree in TREES]
    reached = set()
    for row, got in zip(rows, dump("pick", rows)):
        valid, waveq, stats, prog, srt, occ, bins, min_waves, w8, flags = got
        assert valid == 1, row
        assert (waveq, stats, srt, occ, bins, min_waves) == _expected(*row), row
        assert prog == row[2], row
        assert w8 == (min_waves == 8), row                     # reads bins <=> the _w8 instance
        assert not (stats and (occ or bins)), row              # stats frames walk
        assert flags == stats * STATS | prog * PROG | waveq * WQ | srt * SORTED | occ * OCC | bins * BIN, row
        reached.add(flags)
    # the instances launch_scene_o named before round 13, per tiles flag: 6
    # counting scene_kernel ones, 4 plain block-tile ones ({progressive} x
    # {occ}) and 16 scene_kernel_w8 ones ({progressive, sorted, occ, bin}):
    # 26, twice that with the tiles flag, 52 of the 60 kernels of rt_kernels.hip
    stats_set = {STATS, STATS | PROG, STATS | WQ, STATS | WQ | PROG, STATS | WQ | SORTED,
                 STATS | WQ | SORTED | PROG}
    plain_bt = {p | o for p in (0, PROG) for o in (0, OCC)}
    w8_set = {WQ | p | s | o | b for p in (0, PROG) for s in (0, SORTED) for o in (0, OCC) for b in (0, BIN)}
    assert reached == stats_set | plain_bt | w8_set and len(reached) == 26


def test_unknown_variants_are_refused_and_progressive_frames_ignore_the_variant(dump):
    rows = [(v, 8, prog, 0, 1, 0, 0, 0, 1) for v in (1, 2, 3, 5, 6, 8, 9, 11, 12, 14, 15) for prog in (0, 1)]
    for row, got in zip(rows, dump("pick", rows)):
        assert got[0] == row[2], row      # valid only as a progressive frame (the unified walk)


# ---- the wave-tile grid ----------------------------------------------------------

def _ceil(a, b):
    return -(-a // b)


@pytest.mark.parametrize("n_tiles,ts", [(0, 0), (3, 64), (255, 64), (3, 128), (200, 128)])
def test_wave_grid_closed_forms(dump, n_tiles, ts):
    rows = [(w, h, spp, n_tiles, ts)
            for w, h in [(1, 1), (7, 9), (64, 64), (65, 64), (130, 70), (512, 513), (1920, 1080), (3840, 2160)]
            for spp in (1, 2, 4, 8, 16, 64, 130)]
    for (w, h, spp, _, _), got in zip(rows, dump("grid", rows)):
        lanes = 1 << (min(spp, 64) - 1).bit_length()            # lanes per pixel
        lg = (64 // lanes).bit_length() - 1                     # log2 of the pixels per wave
        tw, th = 1 << (lg + 1) // 2, 1 << lg // 2
        gw, gh = (ts // tw, ts // th) if n_tiles else (_ceil(w, tw), _ceil(h, th))
        grids = n_tiles or 1
        blocks = grids * _ceil(gw, 8) * _ceil(gh, 8)
        sbs = grids * _ceil(gw, 64) * _ceil(gh, 64)
        shift = 12 if sbs >= 192 and 4 * blocks >= 3 * 64 * sbs else 6
        assert got == (tw, th, gw, gh, _ceil(gw, 8), _ceil(gh, 8), _ceil(gw, 64), _ceil(gh, 64), blocks, sbs,
                       grids * gw * gh, shift), (w, h, spp)


def test_wave_grid_of_the_flagship_frame(dump):
    got = dump("grid", [(1920, 1080, 64, 0, 0)])[0]
    assert got[:2] == (1, 1) and got[9] == 510 and got[11] == 12


# ---- the workgroup's LDS -----------------------------------------------------------

@pytest.mark.parametrize("tab_k,depth", TREES + [(0, 2), (3, 3), (7, 8)])
def test_frame_lds_layouts(dump, tab_k, depth):
    plain, srt = dump("lds", [(0, tab_k, depth), (1, tab_k, depth)])
    for sums, stacks, waves, leaf, total in (plain, srt):
        assert all(o % 16 == 0 for o in (sums, stacks, waves, leaf, total))
        assert 0 == sums <= stacks <= waves <= leaf < total     # in this order, none overlapping
        assert total - leaf == LEAF_BUF_BYTES
    # plain: 256 float4 sums, [level][thread] uint2 stacks, no sorted regions
    assert plain[1] - plain[0] == 256 * 16 and plain[2] - plain[1] == _levels(tab_k, depth) * 256 * 8
    assert plain[3] == plain[2] and plain[4] == _scene_lds_bytes(tab_k, depth)
    # sorted: no sums, the stackless walk's stacks, 4 per-wave regions
    assert srt[1] == srt[0] and srt[2] - srt[1] == _levels(tab_k, depth, True) * 256 * 8
    assert srt[3] - srt[2] == 4 * SORT_WAVE_BYTES and srt[4] == _sort_lds_bytes(tab_k, depth)
