"""The oracle's first-hit G-buffer of one camera (rt_render_gbuffer, DESIGN.md
5.8), shared by test_gpu_gbuffer.py and the query fuzz (query_fuzz.py):
oracle.get_ray + oracle.Scene.trace per pixel centre; the normal restated in
numpy float32, one rounding per operation (hit_shade's operations); the albedo
gathered by sphere index.
"""
import numpy as np

NO_HIT = 0xFFFFFFFF


def expected(orc, sc, sp, al, P, K, w, h):
    """t (h, w) f32 (a miss: +inf), sphere (h, w) u32 (a miss: NO_HIT), normal
    (h, w, 4) f32, albedo (h, w) u32, the summed node / prim counters and the
    rays' directions (h, w, 3) f32, of oracle scene `sc` over spheres `sp` and
    albedo words `al`, seen with pose P and intrinsic K."""
    o = np.asarray(P, np.float32).reshape(4, 4)[3, :3].astype(np.float32)
    t = np.full((h, w), np.inf, np.float32)
    sphere = np.full((h, w), NO_HIT, np.uint32)
    d = np.zeros((h, w, 3), np.float32)
    nodes = prims = 0
    for y in range(h):
        for x in range(w):
            d[y, x] = orc.get_ray(P, K, float(x), float(y))
            hit, th, idx, cnt = sc.trace(o, d[y, x])
            if hit:
                t[y, x], sphere[y, x] = th, idx
            nodes += int(cnt[2])
            prims += int(cnt[3])
    hit = sphere != NO_HIT
    normal = np.zeros((h, w, 4), np.float32)
    rec = sp[sphere[hit]]
    p = o[None, :] + t[hit][:, None] * d[hit]           # float32 throughout: one rounding per operation
    ir = np.float32(1.0) / rec[:, 3]
    normal[hit, :3] = (p - rec[:, :3]) * ir[:, None]
    albedo = np.zeros((h, w), np.uint32)
    albedo[hit] = al[sphere[hit]]
    out = dict(t=t, sphere=sphere, normal=normal, albedo=albedo, nodes=nodes, prims=prims, dirs=d)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out
