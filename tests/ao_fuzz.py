"""Seeded cases for the ambient-occlusion layer (rt_render_ao)
and their expectations, shared by test_ao_fuzz_cpu.py and test_gpu_ao_fuzz.py.

ao_case(seed): plain_fuzz.plain_case(seed)'s scene, tree, camera and intrinsic
(a grown, non-cubic root box; radii over three decades; cameras inside, beside
and far from the cloud; negated focal lengths), its frame size capped at 24x17,
8 rays a pixel, and a radius drawn per seed from the scene's mean sphere
radius, 8 times it, and +inf.

model(seed, oracle): ao_ref.expected of the case, computed once and kept.
"""
import numpy as np

import ao_ref
from plain_fuzz import SEEDS, oracle_scene, plain_case     # noqa: F401  (SEEDS: for the tests)

RAYS = 8
MAX_W, MAX_H = 24, 17


def ao_case(seed: int) -> dict:
    c = plain_case(seed)
    c["w"], c["h"] = min(c["w"], MAX_W), min(c["h"], MAX_H)
    mean = float(c["sp"][:, 3].astype(np.float64).mean())
    g = np.random.default_rng(9700 + seed)
    c["radius"] = float(np.float32((mean, 8.0 * mean, np.inf)[int(g.integers(0, 3))]))
    c["salt"] = int(g.integers(0, 1 << 32))
    return c


_MODELS = {}


def model(seed, orc):
    m = _MODELS.get(seed)
    if m is None:
        c = ao_case(seed)
        s = oracle_scene(orc, c)
        m = dict(case=c, exp=ao_ref.expected(orc, s, c["sp"], c["al"], c["pose"], c["K"], c["w"], c["h"], RAYS,
                                             c["radius"], c["salt"]))
        s.close()
        _MODELS[seed] = m
    return m
