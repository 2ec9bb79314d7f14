"""The tile words of the screen-space bins restated in
numpy, and tests/native/bin_tiles_dump.cpp compiled and run: a stand-alone
program built with the address and undefined-behaviour sanitizers that prints
csrc/rt_bins_math.h's tile-word functions."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = 8
WALK = 0xFFFFFFFF
SHAPES = [(1, 1), (2, 1), (2, 2), (4, 2), (4, 4), (8, 4), (8, 8)]   # wave tiles, 64 spp .. 1 spp


def build_dump(d):
    """Compile the program into directory `d`; returns run(*args) -> stdout.
    A sanitizer report fails the caller's test."""
    exe = str(d / "bin_tiles_dump")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "bin_tiles_dump.cpp")])

    def run(*args):
        r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, r.stderr
        return r.stdout
    run.dir = d
    return run


def pack_rect(x0, x1, y0, y1):
    return int(x0) | int(x1) << 4 | int(y0) << 8 | int(y1) << 12


def tile_of(x, y, tw, th):
    """Brute force: the tiles of a bin numbered row by row over its pixels."""
    return ((y % BIN) // th) * (BIN // tw) + (x % BIN) // tw


def tile_words(rects, tw, th):
    """rects: (cnt, 4) bin-local inclusive {x0, x1, y0, y1} in list order.  Per
    tile of the bin a Python int: bit k set iff rectangle k holds a pixel of
    the tile, found pixel by pixel."""
    tpb = (BIN // tw) * (BIN // th)
    words = [0] * tpb
    ys, xs = np.mgrid[0:BIN, 0:BIN]
    tile = tile_of(xs, ys, tw, th)      # every pixel's tile
    for k, (x0, x1, y0, y1) in enumerate(np.asarray(rects, np.int64).reshape(-1, 4)):
        for t in np.unique(tile[y0:y1 + 1, x0:x1 + 1]):
            words[int(t)] |= 1 << k
    return words


def frame_tile_words(hdr, idx, rect_px, w, tw, th):
    """The (bins, tiles per bin) words of a frame from its exported lists (hdr,
    idx: rt_export_bins) and the spheres' pixel rectangles (rect_px[i] = {x0,
    y0, x1, y1}, bins_native.rects): empty bins and bins over the cap hold 0."""
    nbx = (w + BIN - 1) // BIN
    tpb = (BIN // tw) * (BIN // th)
    out = np.zeros((hdr.shape[0], tpb), np.uint64)
    for b, (off, cnt) in enumerate(hdr):
        if cnt == WALK or cnt == 0:
            continue
        px, py = (b % nbx) * BIN, (b // nbx) * BIN
        r = rect_px[idx[off:off + cnt].astype(np.int64)]
        loc = np.stack([np.clip(r[:, 0] - px, 0, BIN - 1), np.clip(r[:, 2] - px, 0, BIN - 1),
                        np.clip(r[:, 1] - py, 0, BIN - 1), np.clip(r[:, 3] - py, 0, BIN - 1)], axis=1)
        out[b] = np.array(tile_words(loc, tw, th), np.uint64)
    return out
