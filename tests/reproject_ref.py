"""The reference of a layer carried across camera motion (rt_reproject_layer;
DESIGN.md 5.17), shared by test_reproject_cpu.py and test_gpu_reproject.py: the
specification of include/rt.h restated on numpy float32 arrays, one rounding per
operation.  The four taps are four gathers accumulated in the stated order (rows
outer, columns inner).  A skipped tap adds +0 to the sums, which changes no bit
of them: they start at +0, and x + 0 = x for every x but -0, which a sum that
started at +0 never is.
"""
import numpy as np

NO_HIT = 0xFFFFFFFF
DEFAULTS = dict(max_count=32.0, depth_tol=0.05)
_ZERO, _ONE = np.float32(0.0), np.float32(1.0)


def params_ok(channels, max_count, depth_tol, flags=0):
    """(all, channels, max_count, depth_tol) as the call checks them."""
    m, d = np.float32(max_count), np.float32(depth_tol)
    c = channels in (1, 4)
    mo = bool(np.isfinite(m) and m >= _ONE)
    do = bool(d > _ZERO)
    return (c and mo and do and flags == 0, c, mo, do)


def rays(orc, pose, K, w, h):
    """The pixel-centre rays (h, w, 3) float32 of a camera: oracle.get_ray."""
    d = np.zeros((h, w, 3), np.float32)
    for y in range(h):
        for x in range(w):
            d[y, x] = orc.get_ray(pose, K, float(x), float(y))
    return d


def project(pose, K, o, d, t):
    """A hit point o + t*d (o (3,), d (..., 3), t (...,), float32) in the previous
    camera (pose (16,) or (4, 4), K (9,) or (3, 3)) -> u0, v0, a, b, dist (float32)
    and front (bool), elementwise."""
    P = np.asarray(pose, np.float32).reshape(16)
    Kf = np.asarray(K, np.float32).reshape(9)
    o = np.asarray(o, np.float32).reshape(3)
    d = np.asarray(d, np.float32)
    t = np.asarray(t, np.float32)
    with np.errstate(all="ignore"):
        q = [(o[k] + t * d[..., k]) - P[12 + k] for k in range(3)]
        cx, cy, cz = ((P[4 * k] * q[0] + P[4 * k + 1] * q[1]) + P[4 * k + 2] * q[2] for k in range(3))
        dist = np.sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2])
        front = cz > _ZERO
        u = (cx / cz) * Kf[0] + Kf[2]
        v = (cy / cz) * Kf[4] + Kf[5]
        u0, v0 = np.floor(u), np.floor(v)
        a, b = u - u0, v - v0
    for x in (u0, v0, a, b, dist):
        assert x.dtype == np.float32
    return u0, v0, a, b, dist, front


def inside(coord, size):
    """A tap coordinate (float32) lies on an axis of `size` pixels, decided in float."""
    with np.errstate(all="ignore"):
        return (coord >= _ZERO) & (coord <= np.float32(size - 1))


def accepted(s, s_hist, dist, t_hist, depth_tol):
    with np.errstate(all="ignore"):
        return (s_hist == s) & (np.abs(dist - t_hist) <= np.float32(depth_tol) * t_hist)


def weight(i, j, a, b):
    return (a if i else _ONE - a) * (b if j else _ONE - b)


def reproject(cur, sphere, t, dirs, o, hist=None, max_count=32.0, depth_tol=0.05):
    """cur (h, w) or (h, w, 4) float32, this frame's layer, under the current hits
    sphere (h, w) uint32 and t (h, w) float32 along dirs (h, w, 3) from o (3,);
    hist: None or {"sphere", "t", "layer", "count", "pose", "K"} of the previous
    frame -> (out, count (h, w) float32, took (h, w) bool: pixels that accepted
    history)."""
    v = np.ascontiguousarray(cur, np.float32)
    flat = v.ndim == 2
    if flat:
        v = v[..., None]
    h, w, _ = v.shape
    sphere = np.asarray(sphere, np.uint32)
    count = np.ones((h, w), np.float32)
    took = np.zeros((h, w), bool)
    out = v.copy()
    if hist is not None:
        hs = np.asarray(hist["sphere"], np.uint32).reshape(-1)
        ht = np.asarray(hist["t"], np.float32).reshape(-1)
        hl = np.ascontiguousarray(hist["layer"], np.float32).reshape(h * w, -1)
        hc = np.asarray(hist["count"], np.float32).reshape(-1)
        u0, v0, a, b, dist, front = project(hist["pose"], hist["K"], o, dirs, np.asarray(t, np.float32))
        live = (sphere != NO_HIT) & front
        sw = np.zeros((h, w), np.float32)
        sc = np.zeros((h, w), np.float32)
        sv = np.zeros_like(v)
        with np.errstate(all="ignore"):
            for j in range(2):
                fv = v0 + np.float32(j)
                for i in range(2):
                    fu = u0 + np.float32(i)
                    on = live & inside(fu, w) & inside(fv, h)
                    q = np.where(on, fv, _ZERO).astype(np.int64) * w + np.where(on, fu, _ZERO).astype(np.int64)
                    on = on & accepted(sphere, hs[q], dist, ht[q], depth_tol)
                    wq = weight(i, j, a, b)
                    sw = sw + np.where(on, wq, _ZERO)
                    sv = sv + np.where(on[..., None], wq[..., None] * hl[q], _ZERO)
                    sc = sc + np.where(on, wq * hc[q], _ZERO)
            took = live & (sw > _ZERO)
            n = np.fmin(sc / sw + _ONE, np.float32(max_count))
            alpha = _ONE / n
            hv = sv / sw[..., None]
            blend = hv + (v - hv) * alpha[..., None]
        out = np.where(took[..., None], blend, v)
        count = np.where(took, n, _ONE)
        assert sw.dtype == sv.dtype == sc.dtype == np.float32
    assert out.dtype == count.dtype == np.float32
    return (out[..., 0] if flat else out), count, took
