"""The pure helpers of raytracingstudy_amd/renderer.py that pack a batch query's
input and unpack its output words: no GPU, no torch device.
"""
import numpy as np
import pytest

from raytracingstudy_amd.renderer import _overlap_words, _records, _split_pairs

RAYS_MSG = "rays must be an (n, 8) float32 array in rt_ray layout"
PROBES_MSG = "probes must be an (n, 4) float32 array in rt_probe layout"
# a NaN with a payload, all ones (a NaN as a float, RT_NO_HIT as an index), -0.0, +inf
WORDS = np.array([0x7FC00001, 0xFFFFFFFF, 0x80000000, 0x7F800000], np.uint32)


def _rays(a):
    return _records(a, 8, "rays", "rt_ray")


def _probes(a):
    return _records(a, 4, "probes", "rt_probe")


def _is_upload_ready(a, shape):
    return (a.dtype == np.float32 and a.shape == shape and a.flags.c_contiguous and a.flags.writeable)


def test_records_accepts_what_callers_hold():
    values = np.arange(24, dtype=np.float64).reshape(3, 8) / 7.0
    exp = values.astype(np.float32)
    for given in (values.tolist(), values, exp):
        got = _rays(given)
        assert _is_upload_ready(got, (3, 8)) and np.array_equal(got, exp)
    assert _rays(exp) is exp  # already as wanted: no copy
    wide = np.arange(48, dtype=np.float32).reshape(3, 16)
    got = _rays(wide[:, ::2])  # a non-contiguous slice
    assert _is_upload_ready(got, (3, 8)) and np.array_equal(got, wide[:, ::2])
    pr = np.arange(12, dtype=np.float32).reshape(3, 4)
    got = _probes(pr[::-1])
    assert _is_upload_ready(got, (3, 4)) and np.array_equal(got, pr[::-1])


def test_records_copies_a_read_only_array_and_leaves_it_alone():
    ro = np.arange(24, dtype=np.float32).reshape(3, 8)
    ro.setflags(write=False)
    before = ro.copy()
    got = _rays(ro)
    assert _is_upload_ready(got, (3, 8)) and not np.shares_memory(got, ro)
    got[:] = -1.0
    assert np.array_equal(ro, before) and not ro.flags.writeable


def test_records_accepts_no_records():
    assert _is_upload_ready(_rays(np.zeros((0, 8), np.float32)), (0, 8))
    assert _is_upload_ready(_probes(np.zeros((0, 4), np.float32)), (0, 4))


@pytest.mark.parametrize("make, bad, msg", [
    (_rays, np.zeros((3, 7), np.float32), RAYS_MSG),
    (_rays, np.zeros(8, np.float32), RAYS_MSG),
    (_probes, np.zeros((3, 3), np.float32), PROBES_MSG),
    (_probes, np.zeros(4, np.float32), PROBES_MSG),
], ids=["rays-3x7", "rays-1d", "probes-3x3", "probes-1d"])
def test_records_rejects_other_shapes(make, bad, msg):
    with pytest.raises(ValueError) as e:
        make(bad)
    assert str(e.value) == msg


def _pairs(shape):
    """int32 records of `shape` + (2,): both words of each run through WORDS, out of step."""
    m = int(np.prod(shape))
    words = np.empty(shape + (2,), np.uint32)
    words[..., 0] = WORDS[np.arange(m) % 4].reshape(shape)
    words[..., 1] = WORDS[(np.arange(m) + 1) % 4].reshape(shape)
    return words.view(np.int32)


@pytest.mark.parametrize("shape", [(n, k) for n in (0, 1, 3) for k in (1, 3)] + [(0,), (1,), (3,), (4,)],
                         ids=lambda s: "x".join(map(str, s)))
def test_split_pairs_is_bit_exact(shape):
    """(n, k, 2) as the multi-hit and closest queries hold it, (n, 2) as trace_rays does."""
    words = _pairs(shape)
    before = words.copy()
    f, u = _split_pairs(words)
    assert f.dtype == np.float32 and u.dtype == np.uint32
    assert f.shape == shape and u.shape == shape
    assert f.flags.c_contiguous and u.flags.c_contiguous
    assert np.array_equal(f.view(np.uint32), words[..., 0].view(np.uint32))
    assert np.array_equal(u, words[..., 1].view(np.uint32))
    # arrays of their own, and of no one else's
    assert f.flags.owndata or f.base.flags.owndata
    assert not np.shares_memory(f, words) and not np.shares_memory(u, words)
    assert np.array_equal(words, before)


def test_split_pairs_keeps_the_special_values():
    f, u = _split_pairs(_pairs((4,)))
    assert np.isnan(f[0]) and np.isnan(f[1]) and f[3] == np.inf
    assert f[2] == 0.0 and np.signbit(f[2])
    assert list(u) == [0xFFFFFFFF, 0x80000000, 0x7F800000, 0x7FC00001]


def test_overlap_words():
    for given in ([0, 5, 0x80000010, 0x80000000], np.array([0, 5, 0x80000010, 0x80000000], np.uint32)):
        count, more = _overlap_words(given)
        assert count.dtype == np.uint32 and more.dtype == np.bool_
        assert list(count) == [0, 5, 16, 0] and list(more) == [False, False, True, True]
    count, more = _overlap_words(0x80000003)  # one word, as overlaps_at holds it
    assert (int(count), bool(more)) == (3, True)
    count, more = _overlap_words(np.zeros(0, np.uint32))
    assert count.shape == (0,) and more.shape == (0,)
