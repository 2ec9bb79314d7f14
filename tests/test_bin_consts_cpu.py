"""The frame-constant word of the screen-space bins (csrc/rt_bins_math.h,
DESIGN.md 5.1 round 19) on the CPU: the frame kernel reads the build's fallback
flag, the wide list's length and the logarithms of the wave tile's sides once
per wave and carries them in one word.  tests/native/bin_consts_dump.cpp, built
with the address and undefined-behaviour sanitizers, packs and unpacks every
legal combination; what does not fit is refused.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE_CAP, SHIFT = 32, 3            # kBinWideCap, kBinShift


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bin_consts") / "bin_consts_dump")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "bin_consts_dump.cpp")])

    def run(*args):
        r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, r.stderr   # a sanitizer report fails the test
        return r.stdout
    return run


def test_every_legal_word_round_trips(dump):
    rows = [line.split() for line in dump("all").splitlines()]
    seen = {}
    legal = set()
    for f, wide, ltw, lth, word, f2, wide2, ltw2, lth2 in rows:
        flag, word = int(f, 16), int(word, 16)
        key = (1 if flag else 0, int(wide), int(ltw), int(lth))
        assert key == (int(f2), int(wide2), int(ltw2), int(lth2)), (f, wide, ltw, lth, word)
        # one scalar register, and no two meanings share a word
        assert word < 1 << 32 and seen.setdefault(word, key) == key
        legal.add((flag, *key[1:]))
    # the program skipped nothing that is legal: every flag word it was given
    # times every wide count, ltw and lth within the limits
    flags = {flag for flag, *_ in legal}
    assert {0, 1, 2, 4, 7, 0xFFFFFFFF} <= flags
    assert len(legal) == len(flags) * (WIDE_CAP + 1) * (SHIFT + 1) ** 2
    assert len(seen) == 2 * (WIDE_CAP + 1) * (SHIFT + 1) ** 2


@pytest.mark.parametrize("wide,ltw,lth,fits", [
    (0, 0, 0, 1), (WIDE_CAP, SHIFT, SHIFT, 1),
    (WIDE_CAP + 1, 0, 0, 0), (64, 0, 0, 0), (0xFFFFFFFF, 0, 0, 0),
    (0, SHIFT + 1, 0, 0), (0, 0, SHIFT + 1, 0), (0, 0xFFFFFFFF, 0, 0), (0, 0, 0xFFFFFFFF, 0),
])
def test_what_does_not_fit_is_refused(dump, wide, ltw, lth, fits):
    assert dump("fit", wide, ltw, lth).strip() == str(fits)
