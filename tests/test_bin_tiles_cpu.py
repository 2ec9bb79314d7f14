"""The tile words' arithmetic (csrc/rt_bins_math.h: bin_tile_index,
bin_rect_overlaps_tile, bin_tile_word) on the CPU: a
stand-alone sanitized program (tests/native/bin_tiles_dump.cpp) against a numpy
brute force over the bin's pixels, for the seven wave-tile shapes."""
import numpy as np
import pytest

from bin_tiles_model import BIN, SHAPES, build_dump, pack_rect, tile_of, tile_words


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    return build_dump(tmp_path_factory.mktemp("bin_tiles"))


@pytest.mark.parametrize("tw,th", SHAPES)
def test_tile_index(dump, tw, th):
    """Every pixel of a 2x2-bin block: the division form and the kernel's shift
    form are the tile of the pixel inside its bin, row by row; every tile of a
    bin holds tw * th pixels."""
    lines = dump("index", tw, th).split("\n")
    tpb = int(lines[0])
    assert tpb == (BIN // tw) * (BIN // th) == 64 // (tw * th)
    rows = np.array([l.split() for l in lines[1:] if l], np.int64)
    assert rows.shape == (256, 4)
    x, y = rows[:, 0], rows[:, 1]
    want = tile_of(x, y, tw, th)
    assert np.array_equal(rows[:, 2], want) and np.array_equal(rows[:, 3], want)
    inside = (x < BIN) & (y < BIN)
    assert np.array_equal(np.bincount(want[inside], minlength=tpb), np.full(tpb, tw * th))


def _lists(rng):
    """Lists of 1, 2, 63 and 64 entries (and a few lengths between), of
    rectangles that are full-bin, single-pixel, on the bin's edges, or random."""
    def rect(kind):
        if kind == 0:
            return (0, BIN - 1, 0, BIN - 1)
        if kind == 1:
            x, y = rng.integers(0, BIN, 2)
            return (x, x, y, y)
        if kind == 2:    # a row or a column on an edge of the bin
            e = int(rng.choice([0, BIN - 1]))
            a, b = np.sort(rng.integers(0, BIN, 2))
            return (e, e, a, b) if rng.integers(2) else (a, b, e, e)
        (x0, x1), (y0, y1) = np.sort(rng.integers(0, BIN, 2)), np.sort(rng.integers(0, BIN, 2))
        return (x0, x1, y0, y1)
    out = []
    for cnt in (1, 2, 63, 64, 1, 2, 63, 64, 7, 33):
        out.append(np.array([rect(int(rng.integers(0, 4))) for _ in range(cnt)], np.int64))
    # bit 63 alone in some tiles: 63 single pixels at (0, 0), the last entry at (7, 7)
    out.append(np.array([(0, 0, 0, 0)] * 63 + [(7, 7, 7, 7)], np.int64))
    # ... and bit 63 everywhere: the last entry covers the bin
    out.append(np.array([(3, 3, 3, 3)] * 63 + [(0, 7, 0, 7)], np.int64))
    return out


@pytest.mark.parametrize("tw,th", SHAPES)
def test_tile_words(dump, tw, th):
    rng = np.random.default_rng(1000 * tw + th)
    lists = _lists(rng)
    path = dump.dir / f"lists_{tw}x{th}.txt"
    path.write_text("".join(
        " ".join([str(tw), str(th), str(len(l))] + ["%x" % pack_rect(*r) for r in l]) + "\n" for l in lists))
    got = [[int(t, 16) for t in line.split()] for line in dump("words", path).splitlines()]
    assert len(got) == len(lists)
    top = 0
    for l, g in zip(lists, got):
        want = tile_words(l, tw, th)
        assert g == want, (tw, th, len(l))
        assert all(w < (1 << len(l)) for w in g)                 # no bit past the list
        assert [k for k in range(len(l)) if not any(w >> k & 1 for w in g)] == []   # every entry in some tile
        top += sum(w >> 63 & 1 for w in g)
    assert top > 0      # bit 63 was exercised
