"""The reference of the one-bounce diffuse layer (rt_render_indirect and
rt_add_layer), shared by test_indirect_cpu.py,
test_gpu_indirect.py and the indirect fuzz: the bounce rays are ao_ref.rays_of's,
each ray's nearest hit and each lit hit's shadow bit are oracle.Scene.trace's
(nearest, then any_hit=True) with their counters, and the shading, the ordered
sum and add_layer are restated in numpy float32, one rounding per operation.
"""
import numpy as np

import ao_ref
import gbuffer_ref

NO_HIT = ao_ref.NO_HIT
SEED = ao_ref.SEED
SHADOW_EPS = ao_ref.SHADOW_EPS
LIGHT = (1.0, 1.0, -1.0)     # rt_config_default's light_dir and ambient
AMBIENT = 0.1
_ZERO, _ONE = np.float32(0.0), np.float32(1.0)
_SKY_R = np.float32(200.0) / np.float32(255.0)
_INV255 = _ONE / np.float32(255.0)
# what a bounce ray met: it escaped, hit a lit point, a shadowed one, one facing away from the light
ESCAPED, LIT, SHADOWED, AWAY = 0, 1, 2, 3


def scale_ok(s):
    """sky_scale and rt_add_layer's gain: finite and >= 0."""
    s = np.float32(s)
    return bool(s >= _ZERO and np.isfinite(s))


def params_ok(rays, radius, sky_scale, flags=0):
    """(all, rays, radius, sky_scale) as the call checks them."""
    a = rays in ao_ref.RAYS
    with np.errstate(all="ignore"):
        b = bool(np.float32(radius) > _ZERO)
    c = scale_ok(sky_scale)
    return a and b and c and flags == 0, a, b, c


def sat(x):
    x = np.asarray(x, np.float32)
    with np.errstate(all="ignore"):
        return np.where(x > _ZERO, np.where(x < _ONE, x, _ONE), _ZERO).astype(np.float32)


def light_toward(light_dir):
    """L (3,) float32: the handle's unit vector toward the light, as fill_shading makes it."""
    ld = np.asarray(light_dir, np.float32)
    ll = np.sqrt((ld[0] * ld[0] + ld[1] * ld[1]) + ld[2] * ld[2])
    return (-(ld / ll)).astype(np.float32)


def sky_color(d, sky_scale):
    """The frames' miss colour of directions d (m, 3), then one multiply each -> (m, 3)."""
    d = np.asarray(d, np.float32).reshape(-1, 3)
    s = np.float32(sky_scale)
    with np.errstate(all="ignore"):
        return np.stack([np.broadcast_to(_SKY_R * s, (len(d),)), sat(d[:, 1]) * s, sat(d[:, 2]) * s],
                        axis=1).astype(np.float32)


def hit_color(al, ambient, lam):
    """The frames' shading of albedo words al (m,) under the Lambert terms lam (m,) -> (m, 3)."""
    al = np.atleast_1d(np.asarray(al)).astype(np.uint32)
    lam = np.atleast_1d(np.asarray(lam, np.float32))
    amb = np.float32(ambient)
    with np.errstate(all="ignore"):
        f = amb + (_ONE - amb) * lam
        return np.stack([((al >> np.uint32(8 * k)) & np.uint32(0xFF)).astype(np.float32) * _INV255 * f
                         for k in range(3)], axis=1).astype(np.float32)


def tree_sum(v):
    """tree_sum's pairing over axis 1 of v (m, rays[, c]) float32: for m = 1, 2, 4,
    .. < rays every v[i] becomes v[i] + v[i ^ m] -> the whole array after the last
    step (element 0 is the sum)."""
    v = np.array(v, np.float32)
    rays = v.shape[1]
    i = np.arange(rays)
    m = 1
    with np.errstate(all="ignore"):
        while m < rays:
            v = v + v[:, i ^ m]
            m <<= 1
    assert v.dtype == np.float32
    return v


def mean_of(total, rays):
    with np.errstate(all="ignore"):
        return (np.asarray(total, np.float32) * (_ONE / np.float32(rays))).astype(np.float32)


def open_share(rays, hits):
    return (np.uint32(rays) - np.asarray(hits, np.uint32)).astype(np.float32) * (_ONE / np.float32(rays))


def color_of_ray(sc, sp, al, o, d, tmax, L, ambient, shadows, sky_scale):
    """One ray from o along d (float32 (3,)), tmin = 0, as rt_render_indirect
    shades it -> (colour (3,) float32, kind, the hit's t and sphere (NO_HIT: none),
    the shadow ray's record (8,) or None, rays cast (1 or 2), nodes, prims)."""
    o, d = np.asarray(o, np.float32), np.asarray(d, np.float32)
    hit, t2, idx, cnt = sc.trace(o, d, 0.0, float(tmax))
    nodes, prims = int(cnt[2]), int(cnt[3])
    if not hit:
        return sky_color(d, sky_scale)[0], ESCAPED, np.float32(tmax), NO_HIT, None, 1, nodes, prims
    t2 = np.float32(t2)
    rec = sp[idx]
    q = o + t2 * d
    m = (q - rec[:3]) * (_ONE / rec[3])
    ndl = (m[0] * L[0] + m[1] * L[1]) + m[2] * L[2]
    lam = ndl if ndl > _ZERO else _ZERO
    kind, srec, cast = (LIT if ndl > _ZERO else AWAY), None, 1
    if ndl > _ZERO and shadows:
        srec = np.zeros(8, np.float32)
        srec[:3] = q + m * SHADOW_EPS
        srec[4:7] = L
        srec[7] = np.inf
        shit, _, _, scnt = sc.trace(srec[:3], srec[4:7], 0.0, float("inf"), any_hit=True)
        nodes += int(scnt[2])
        prims += int(scnt[3])
        cast = 2
        if shit:
            lam, kind = _ZERO, SHADOWED
    assert q.dtype == m.dtype == np.float32 and np.float32(lam).dtype == np.float32
    return hit_color(al[idx], ambient, lam)[0], kind, t2, int(idx), srec, cast, nodes, prims


def expected(orc, sc, sp, al, P, K, w, h, rays, radius, salt=0, sky_scale=1.0, seed=SEED, light=LIGHT,
             ambient=AMBIENT, shadows=True, g=None):
    """layer (h, w, 4) float32, occluded (h, w) uint32, the summed counters (the
    primary walk once per pixel, every bounce ray's nearest walk, every shadow
    ray's any-hit walk), the rays cast (bounce + shadow), and per bounce ray its
    record, kind, hit and shadow record."""
    if g is None:
        g = gbuffer_ref.expected(orc, sc, sp, al, P, K, w, h)
    pixel, recs, _ = ao_ref.rays_of(g, P, sp, rays, radius, salt, seed)
    L = light_toward(light)
    n = len(pixel)
    col = np.zeros((n, rays, 3), np.float32)
    kind = np.zeros((n, rays), np.int64)
    hit_t = np.full((n, rays), np.float32(radius), np.float32)
    hit_s = np.full((n, rays), NO_HIT, np.uint32)
    shadow_recs = []
    nodes, prims, cast = g["nodes"], g["prims"], 0
    for a in range(n):
        for i in range(rays):
            r = recs[a, i]
            col[a, i], kind[a, i], hit_t[a, i], hit_s[a, i], srec, c, nn, pp = color_of_ray(
                sc, sp, al, r[0:3], r[4:7], r[7], L, ambient, shadows, sky_scale)
            if srec is not None:
                shadow_recs.append(srec)
            cast += c
            nodes += nn
            prims += pp
    hits = (kind != ESCAPED).sum(axis=1).astype(np.uint32)
    layer = np.zeros((w * h, 4), np.float32)
    layer[:, 3] = _ONE
    occ = np.zeros(w * h, np.uint32)
    if n:
        layer[pixel, :3] = mean_of(tree_sum(col)[:, 0, :], rays)
        layer[pixel, 3] = open_share(rays, hits)
        occ[pixel] = hits
    out = dict(layer=layer.reshape(h, w, 4), occluded=occ.reshape(h, w), nodes=nodes, prims=prims, cast=cast,
               pixel=pixel, rays=recs, colors=col, kind=kind, hit_t=hit_t, hit_sphere=hit_s,
               shadow_rays=np.array(shadow_recs, np.float32).reshape(-1, 8), gbuffer=g, L=L)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def add_layer(rgba8, layer, albedo=None, gain=1.0):
    """rt_add_layer: rgba8 (h, w, 4) uint8, layer (h, w, 4) float32 and albedo
    (h, w) uint32 or None -> the pixels with the layer's r, g, b added; A kept."""
    px = np.asarray(rgba8, np.uint8)
    out = px.copy()
    lay = np.asarray(layer, np.float32)
    g = np.float32(gain)
    for k in range(3):
        if albedo is None:
            kk = np.ones(px.shape[:2], np.float32)
        else:
            kk = ((np.asarray(albedo, np.uint32) >> np.uint32(8 * k)) & np.uint32(0xFF)).astype(np.float32) * _INV255
        with np.errstate(all="ignore"):
            v = px[..., k].astype(np.float32) + ((kk * g) * lay[..., k]) * np.float32(255.0)
            v = np.fmin(np.fmax(v, _ZERO), np.float32(255.0))      # fmaxf / fminf: a NaN gives 0
        assert v.dtype == np.float32
        out[..., k] = v.astype(np.uint8)
    return out


# ---- the cases of test_indirect_cpu.py and test_gpu_indirect.py: ao_ref.CASES ----------
_KEPT = {}


def case_expected(orc, case, rays, radius, salt=0, sky_scale=1.0, light=LIGHT, ambient=AMBIENT, shadows=True,
                  seed=SEED):
    """expected() of a named ao_ref case, computed once and kept (read-only arrays)."""
    k = (case, rays, float(radius), salt, float(sky_scale), tuple(light), float(ambient), shadows, seed)
    if k not in _KEPT:
        scene, pname, w, h = ao_ref.CASES[case]
        sp, al = ao_ref.spheres(scene)
        sc = ao_ref.oracle_scene(orc, scene)
        g = ao_ref.case_expected(orc, case, 1, 0.1)["gbuffer"]   # the case's G-buffer, made once by ao_ref
        _KEPT[k] = expected(orc, sc, sp, al, ao_ref.pose(pname), ao_ref.intrinsic(orc, case), w, h, rays, radius, salt,
                            sky_scale, seed, light, ambient, shadows, g=g)
    return _KEPT[k]
