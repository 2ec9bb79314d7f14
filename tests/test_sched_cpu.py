"""How a scene frame is scheduled (csrc/rt_sched.h), on the CPU: which kernel
instance runs it, its wave-tile grid and its workgroup's LDS layout, the plan
the host makes of all three per frame, and the size of the launch.
tests/native/sched_dump.cpp, built with the address and undefined-behaviour
sanitizers, prints the header's answers; the expected ones are written out
here independently: the dispatch table of the round-13 issue, closed forms of
the grid, the LDS sizes as the launchers computed them before round 13, and
the launch policy as the launchers held it before round 17.
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


# ---- the plan of a frame, and the size of its launch ----------------------------------
# Expected values restate the launchers as they were before round 17, when
# frame_counters, launch_scene, launch_waveq and launch_persistent each derived
# their part: rt_kernels.hip and rt_frame.cpp of commit b82f6d6.

CHUNK_SHIFT, BTS_SHIFT, NO_WG_CAP = 4, 1, 1 << 7                   # kOptChunkShift, kOptBtsShift, kOptNoWgCap
ONE_SPP_LDS = (160 * 1024 // 3) & ~15                              # kOneSppLds


def _plan_tail(spp, opt, grid, sorted_lds_bytes):
    """What frame_counters and launch_scene derived: spw g ppw rounds slot_shift
    slot_stride lds_bytes ticket ticket_forced (grid: the `grid` mode's row)."""
    spw = min(spp, 64)
    g = 1 << (spw - 1).bit_length()
    rounds = _ceil(spp, spw)
    blocks, sbs, shift = grid[8], grid[9], grid[11]
    ck = (opt >> CHUNK_SHIFT) & 7
    ticket = 1 << (ck - 1) if ck else max(1, 4 // max(1, min(rounds, 4)))
    return (spw, g, 64 // g, rounds, shift, (sbs if shift == 12 else blocks) + 2, sorted_lds_bytes, ticket,
            int(ck != 0))


def _wave_queue(units, resident, cus, per_simd, ticket, forced):     # launch_waveq
    want = _ceil(units, 4)
    cap = cus * per_simd if per_simd else resident
    grid = max(1, min(resident, cap, want))
    if not forced:
        per_wave = units // (grid * 4)
        ticket = min(ticket, 4 if per_wave >= 64 else 2 if per_wave >= 16 else 1)
    return grid, ticket


def _block_tiles(w, h, n_tiles, ts, tw, th, resident, force):        # launch_persistent, count_block_tiles
    count = lambda b: n_tiles * (ts // b) ** 2 if n_tiles else _ceil(w, b) * _ceil(h, b)
    min_side, side = 2 * max(tw, th), 16
    if force and (16 >> (force - 1)) >= min_side:
        side = 16 >> (force - 1)
    else:
        while side // 2 >= min_side and count(side) < 8 * resident:
            side //= 2
    return side, min(count(side), resident)


GEOMETRIES = [(1, 1, 0, 0), (7, 9, 0, 0), (64, 64, 0, 0), (130, 70, 0, 0), (1920, 1080, 0, 0),
              (1920, 1080, 3, 64), (1920, 1080, 64, 64), (1920, 1080, 200, 128)]   # W H n_tiles tile_size
OPTS = [0, 1 << CHUNK_SHIFT, 3 << CHUNK_SHIFT, 4 << CHUNK_SHIFT, 2 << BTS_SHIFT, NO_WG_CAP | 2 << CHUNK_SHIFT]
# (variant, progressive, count_work, sort_on): cycled over the sweep, every one with every spp
KINDS = [(0, 0, 0, 1), (0, 0, 1, 1), (0, 1, 0, 1), (LANE_UNIFIED_2, 0, 0, 1), (WAVEQ, 0, 0, 0),
         (LANE_UNIFIED, 0, 0, 1), (0, 1, 1, 1)]


def test_plan_is_what_the_five_places_derived(dump):
    rows = []
    for spp in range(1, 257):
        for gi, geo in enumerate(GEOMETRIES):
            for oi, opt in enumerate(OPTS):
                i = spp + gi + oi
                v, prog, count, sort_on = KINDS[i % len(KINDS)]
                tab_k, depth = TREES[i % len(TREES)]
                rows.append((v, spp, prog, count, sort_on, tab_k, depth, *geo, opt))
    plans = dump("plan", rows)
    picks = dump("pick", [(v, spp, prog, count, sort_on, 0, 0, tab_k, depth)
                          for v, spp, prog, count, sort_on, tab_k, depth, *_ in rows])
    grids = dump("grid", [(w, h, spp, n, ts) for _, spp, _, _, _, _, _, w, h, n, ts, _ in rows])
    ldss = dump("lds", [(pick[4], row[5], row[6]) for row, pick in zip(rows, picks)])   # pick[4]: sorted
    seen_sorted = seen_forced = seen_block_slots = 0
    for row, plan, pick, grid, lds in zip(rows, plans, picks, grids, ldss):
        assert plan[:10] == pick and plan[10:22] == grid, row
        assert plan[22:] == _plan_tail(row[1], row[11], grid, lds[4]), row
        seen_sorted += pick[4]
        seen_forced += plan[30]
        seen_block_slots += plan[26] == 6
    assert seen_sorted and seen_forced and seen_block_slots


def test_plan_known_answers(dump):
    full, share = dump("plan", [(0, 64, 0, 0, 1, 0, 12, 1920, 1080, 0, 0, 0),
                                (0, 64, 0, 0, 1, 0, 12, 1920, 1080, 64, 64, 0)])
    # the full frame: 1x1 wave tile, 510 superblocks, superblock slots, 1 round, 4 wave tiles a ticket
    assert full[10:12] == (1, 1) and full[19] == 510
    assert full[25:28] == (1, 12, 512) and full[29:] == (4, 0)
    # a 1/8 share of it as 64 packed 64x64 tiles: 64 superblocks, block slots
    assert share[19] == 64 and share[26] == 6


def test_wave_queue_launch_size(dump):
    rows = [(units, res, cus, per_simd, ticket, forced)
            for units in (1, 3, 4, 5, 63, 64, 255, 256, 4095, 4096, 32400, 262144, 524288, 2073600, 1 << 33)
            for res, cus in ((1, 1), (8, 2), (1280, 256), (2048, 256), (2432, 304), (4, 256))
            for per_simd in (0, 7, 8)
            for ticket in (1, 2, 4)
            for forced in (0, 1)]
    for row, got in zip(rows, dump("waveq", rows)):
        assert got == _wave_queue(*row), row
    occ = (2048, 256, 8, 4, 0)      # resident, CUs, waves per SIMD, the plan's ticket, not forced
    got = dump("waveq", [(2073600, *occ), (524288, *occ), (262144, *occ), (1, *occ), (262144, 2048, 256, 8, 4, 1)])
    assert got[0] == (2048, 4)      # C3's frame
    assert got[1][1] == 4           # a 1/4 share: 64 units a wave
    assert got[2][1] == 2           # a 1/8 share: 32
    assert got[3] == (1, 1)
    assert got[4][1] == 4           # a forced ticket is not capped


def test_block_tile_launch_size(dump):
    rows = [(w, h, n, ts, tw, th, res, force)
            for w, h, n, ts in GEOMETRIES + [(512, 513, 0, 0), (1920, 1080, 128, 64)]
            for tw, th in ((1, 1), (2, 1), (2, 2), (4, 2), (4, 4), (8, 4), (8, 8))
            for res in (1, 4, 256, 768, 1280, 2048)
            for force in range(8)]
    for row, got in zip(rows, dump("btiles", rows)):
        assert got == _block_tiles(*row), row
    got = dump("btiles", [(1920, 1080, 0, 0, 1, 1, 1280, 0), (1920, 1080, 64, 64, 1, 1, 1280, 0),
                          (1920, 1080, 128, 64, 1, 1, 1280, 0), (1920, 1080, 0, 0, 8, 8, 1280, 0),
                          (1920, 1080, 0, 0, 8, 8, 1280, 2)])
    assert got[0] == (8, 1280)                  # 1080p at 64 spp
    assert got[1][0] == 4 and got[2][0] == 4    # 1/8 and 1/4 shares
    assert got[3][0] == 16 and got[4][0] == 16  # 1 spp: two 8x8 wave tiles a side, forced or not


def test_block_tile_lds_caps_one_spp_at_three_workgroups(dump):
    rows = [(lds, spw, opt) for lds in (0, 6144, 28672, ONE_SPP_LDS - 16, ONE_SPP_LDS, ONE_SPP_LDS + 16, 65536)
            for spw in (1, 2, 4, 64) for opt in (0, NO_WG_CAP, 2 << BTS_SHIFT, NO_WG_CAP | 1 << CHUNK_SHIFT)]
    for (lds, spw, opt), got in zip(rows, dump("btlds", rows)):
        assert got == (max(lds, ONE_SPP_LDS) if spw == 1 and not opt & NO_WG_CAP else lds,), (lds, spw, opt)
    assert 3 * ONE_SPP_LDS <= 160 * 1024 < 4 * ONE_SPP_LDS and ONE_SPP_LDS % 16 == 0
