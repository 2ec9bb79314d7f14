"""Seeded cases for the one-bounce diffuse layer (rt_render_indirect, DESIGN.md
5.18) and their expectations, shared by test_indirect_fuzz_cpu.py and
test_gpu_indirect_fuzz.py.

indirect_case(seed): plain_fuzz.plain_case(seed)'s scene, tree, camera,
intrinsic, light, ambient and shadow switch (a grown, non-cubic root box; radii
over three decades; cameras inside, beside and far from the cloud; negated
focal lengths; axis-aligned and random lights), its frame size capped at 24x17,
4 rays a pixel, a radius drawn per seed from the scene's mean sphere radius, 8
times it, and +inf, a salt, and sky_scale drawn from {0, 1}.

model(seed, oracle): indirect_ref.expected of the case, computed once and kept.
"""
import numpy as np

import indirect_ref
from plain_fuzz import SEEDS, oracle_scene, plain_case     # noqa: F401  (SEEDS: for the tests)

RAYS = 4
MAX_W, MAX_H = 24, 17


def indirect_case(seed: int) -> dict:
    c = plain_case(seed)
    c["w"], c["h"] = min(c["w"], MAX_W), min(c["h"], MAX_H)
    mean = float(c["sp"][:, 3].astype(np.float64).mean())
    g = np.random.default_rng(9800 + seed)
    c["radius"] = float(np.float32((mean, 8.0 * mean, np.inf)[int(g.integers(0, 3))]))
    c["salt"] = int(g.integers(0, 1 << 32))
    c["sky_scale"] = float(g.integers(0, 2))
    return c


_MODELS = {}


def model(seed, orc):
    m = _MODELS.get(seed)
    if m is None:
        c = indirect_case(seed)
        s = oracle_scene(orc, c)
        m = dict(case=c, exp=indirect_ref.expected(orc, s, c["sp"], c["al"], c["pose"], c["K"], c["w"], c["h"], RAYS,
                                                   c["radius"], c["salt"], c["sky_scale"], light=c["light"],
                                                   ambient=c["ambient"], shadows=c["shadows"]))
        s.close()
        _MODELS[seed] = m
    return m
