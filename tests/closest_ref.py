"""The CPU reference of the closest-sphere query (rt_query_closest, DESIGN.md
5.12) and the probe mixes its tests share (test_closest_cpu.py,
test_gpu_closest.py, test_gpu_closest_fuzz.py).  The scenes and trees are
overlap_ref's.

The key of probe point p and sphere (c, r) is sqrtf(d2) - r with dx = p.x - c.x
(likewise dy, dz) and d2 = (dx*dx + dy*dy) + dz*dz: every operation one IEEE
f32 operation, which numpy restates exactly on float32 arrays (no fused
multiply-add, no wider intermediate, a correctly rounded sqrt), so no native
program is needed.  The accepted set is key <= R, the answer its k smallest
members by (key, sphere index).
"""
import functools

import numpy as np

import overlap_ref as ov

NO_HIT = 0xFFFFFFFF
K_MAX = 16
INF = np.float32(np.inf)
CUTOFF = np.float32(0.05)


def with_cutoffs(pr):
    """A probe list with column 3 reused as the search radius: probe i keeps its
    own for i % 3 == 0, gets +inf (unbounded) for i % 3 == 1 and 0.05 for
    i % 3 == 2."""
    out = np.array(pr, np.float32)
    i = np.arange(len(out))
    out[i % 3 == 1, 3] = INF
    out[i % 3 == 2, 3] = CUTOFF
    return out


@functools.lru_cache(maxsize=None)
def probes(name):
    """with_cutoffs(overlap_ref.probes(name)): (1024, 4) float32, read-only."""
    out = with_cutoffs(ov.probes(name))
    out.setflags(write=False)
    return out


def probe_ok(pr):
    """(n,) bool: a finite centre and R >= 0 (R = -0 and +inf included, NaN not)."""
    pr = np.asarray(pr, np.float32)
    with np.errstate(all="ignore"):
        return np.isfinite(pr[:, :3]).all(axis=1) & (pr[:, 3] >= 0)


def keys(sp, pr):
    """(n_probes, n_spheres) float32: the key, in f32, in the spec's order."""
    sp = np.ascontiguousarray(sp, np.float32)
    pr = np.ascontiguousarray(pr, np.float32)
    with np.errstate(all="ignore"):
        dx = pr[:, None, 0] - sp[None, :, 0]
        dy = pr[:, None, 1] - sp[None, :, 1]
        dz = pr[:, None, 2] - sp[None, :, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        key = np.sqrt(d2) - sp[None, :, 3]
    assert key.dtype == np.float32
    return key


def reference(sp, pr, k=K_MAX, skip_self=False):
    """Brute force over all of `sp` for every probe: (dist (n, k) float32, sphere
    (n, k) uint32, count (n,) uint32, total (n,) int64) in the layout of
    rt_query_closest: slots past a probe's count hold {its radius as given,
    NO_HIT}; `total` is the size of each probe's accepted set."""
    sp = np.ascontiguousarray(sp, np.float32)
    pr = np.ascontiguousarray(pr, np.float32)
    n = len(pr)
    dist = np.repeat(pr[:, 3:4], k, axis=1)
    sphere = np.full((n, k), NO_HIT, np.uint32)
    total = np.zeros(n, np.int64)
    ok = probe_ok(pr)
    for a in range(0, n, 128):  # (in slices: the temporaries stay small)
        key = keys(sp, pr[a:a + 128])
        with np.errstate(all="ignore"):
            member = (key <= pr[a:a + 128, 3:4]) & ok[a:a + 128, None]
        if skip_self:
            i = np.arange(a, min(a + len(key), len(sp)))
            member[i - a, i] = False
        total[a:a + 128] = member.sum(axis=1)
        for m in np.flatnonzero(total[a:a + 128]):
            idx = np.flatnonzero(member[m])
            kv = key[m, idx]
            if len(idx) > 4 * k:  # only the members up to the k-th key (ties included) can be listed
                idx = idx[kv <= np.partition(kv, k - 1)[k - 1]]
                kv = key[m, idx]
            order = np.lexsort((idx, kv))[:k]
            dist[a + m, :len(order)] = kv[order]
            sphere[a + m, :len(order)] = idx[order]
    return dist, sphere, np.minimum(total, k).astype(np.uint32), total


@functools.lru_cache(maxsize=None)
def expected(name):
    """reference() of scene `name`'s probe mix at k = 16, computed once
    (read-only).  A smaller k's answer is its first k columns: cut()."""
    out = reference(ov.spheres(name), probes(name), K_MAX)
    for a in out:
        a.setflags(write=False)
    return out


def cut(ref, k):
    """The answer for k <= the reference's k from its (dist, sphere, count, total):
    the order is total, so the first k columns are the k nearest."""
    dist, sphere, _, total = ref
    assert k <= dist.shape[1]
    return (np.ascontiguousarray(dist[:, :k]), np.ascontiguousarray(sphere[:, :k]),
            np.minimum(total, k).astype(np.uint32))


def mix_counts(ref):
    """What a mix exercises, from its k = 16 reference: probes with an empty set,
    with more than 16 members, with 1..16, with a negative key among their
    answers, and with two equal keys among their answers."""
    dist, sphere, count, total = ref
    held = sphere != NO_HIT
    tied = (dist[:, 1:] == dist[:, :-1]) & held[:, 1:]
    return dict(empty=int((total == 0).sum()), truncated=int((total > K_MAX).sum()),
                partial=int(((total > 0) & (total <= K_MAX)).sum()),
                negative=int(((dist < 0) & held).any(axis=1).sum()), tied=int(tied.any(axis=1).sum()))
