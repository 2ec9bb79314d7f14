"""The reference of the guide-driven layer filter and the layer multiply
(rt_filter_layer, rt_apply_layer), shared by test_filter_cpu.py
and test_gpu_filter.py: the specification of include/rt.h restated on numpy
float32 arrays.  A pass's 25 taps are 25 shifted views of padded arrays,
accumulated in the stated order (rows outer, columns inner), one rounding per
operation.  A skipped tap adds +0 to the sums, which changes no bit of them:
they start at +0, and x + 0 = x for every x but -0, which a sum that started at
+0 never is.
"""
import numpy as np

NO_HIT = 0xFFFFFFFF
K = np.array([0.375, 0.25, 0.0625], np.float32)
DEFAULTS = dict(passes=3, depth_sigma=0.05, normal_power=5)
_ZERO, _ONE = np.float32(0.0), np.float32(1.0)


def inv_depth(depth_sigma, t_p):
    """iz of a pixel: 1 / (depth_sigma * t_p); 0 under depth_sigma = +inf."""
    with np.errstate(all="ignore"):
        return _ONE / (np.float32(depth_sigma) * np.asarray(t_p, np.float32))


def weight(k, n_p, n_q, t_p, t_q, iz, normal_power):
    """The weight of tap q from pixel p, elementwise: k, t_p, t_q, iz (...,) and
    n_p, n_q (..., 3), all float32."""
    k, t_p, t_q, iz = (np.asarray(a, np.float32) for a in (k, t_p, t_q, iz))
    n_p, n_q = np.asarray(n_p, np.float32), np.asarray(n_q, np.float32)
    with np.errstate(all="ignore"):
        dn = (n_p[..., 0] * n_q[..., 0] + n_p[..., 1] * n_q[..., 1]) + n_p[..., 2] * n_q[..., 2]
        wn = np.fmax(dn, _ZERO)            # fmaxf: a NaN gives 0
        for _ in range(int(normal_power)):
            wn = wn * wn
        e = (t_q - t_p) * iz
        wz = _ONE / (_ONE + e * e)
        w = (k * wn) * wz
    assert w.dtype == np.float32
    return w


def plan(passes):
    """[(step, source, destination)] per pass: "in", "out" or "scratch"; the last
    pass writes "out" whatever the parity, and the input is never written."""
    rows = []
    for s in range(passes):
        dst = "out" if (passes - 1 - s) % 2 == 0 else "scratch"
        rows.append((1 << s, "in" if s == 0 else rows[-1][2], dst))
    return rows


def _shift(a, pad, dy, dx, h, w):
    return a[pad + dy:pad + dy + h, pad + dx:pad + dx + w]


def filter_pass(v, sphere, t, normal, step, depth_sigma, normal_power):
    """One pass at tap spacing `step`: v (h, w, c) float32 -> the same shape."""
    h, w, _ = v.shape
    hit = sphere != NO_HIT
    pad = 2 * step
    grow = lambda a, fill: np.pad(a, [(pad, pad), (pad, pad)] + [(0, 0)] * (a.ndim - 2), constant_values=fill)
    hit_g, t_g, n_g, v_g = grow(hit, False), grow(t, _ZERO), grow(normal[..., :3], _ZERO), grow(v, _ZERO)
    n_p = normal[..., :3]
    iz = inv_depth(depth_sigma, t)
    sw = np.zeros((h, w), np.float32)
    sv = np.zeros_like(v)
    with np.errstate(all="ignore"):
        for j in range(-2, 3):
            for i in range(-2, 3):
                dy, dx = j * step, i * step
                on = hit & _shift(hit_g, pad, dy, dx, h, w)      # off-image taps are padding: not hits
                k = K[abs(i)] * K[abs(j)]
                wq = weight(k, n_p, _shift(n_g, pad, dy, dx, h, w), t, _shift(t_g, pad, dy, dx, h, w), iz,
                            normal_power)
                sw = sw + np.where(on, wq, _ZERO)
                sv = sv + np.where(on[..., None], wq[..., None] * _shift(v_g, pad, dy, dx, h, w), _ZERO)
        out = np.where((hit & (sw > _ZERO))[..., None], sv / sw[..., None], v)
    assert out.dtype == np.float32 and sw.dtype == np.float32
    return out


def filter_layer(layer, sphere, t, normal, passes=3, depth_sigma=0.05, normal_power=5):
    """layer (h, w) or (h, w, 4) float32 under the guides sphere (h, w) uint32,
    t (h, w) float32 and normal (h, w, >= 3) float32 -> the filtered layer."""
    v = np.ascontiguousarray(layer, np.float32)
    flat = v.ndim == 2
    if flat:
        v = v[..., None]
    sphere = np.asarray(sphere, np.uint32)
    t = np.asarray(t, np.float32)
    normal = np.asarray(normal, np.float32)
    for step, _, _ in plan(passes):
        v = filter_pass(v, sphere, t, normal, step, depth_sigma, normal_power)
    return v[..., 0] if flat else v


def apply_layer(rgba8, layer, floor):
    """rt_apply_layer: rgba8 (h, w, 4) uint8 and layer (h, w) float32 -> the
    multiplied pixels; m = floor + (1 - floor) * layer, R, G and B truncated, A kept."""
    f = np.float32(floor)
    with np.errstate(all="ignore"):
        m = f + (_ONE - f) * np.asarray(layer, np.float32)
        c = np.asarray(rgba8, np.uint8)[..., :3].astype(np.float32) * m[..., None]
        c = np.fmax(np.fmin(c, np.float32(255.0)), _ZERO)   # fminf: a NaN gives 255
    assert c.dtype == np.float32
    out = np.array(rgba8, np.uint8)
    out[..., :3] = c.astype(np.uint8)
    return out
