"""The AO fuzz cases (ao_fuzz.py) are not vacuous, from the reference alone:
over the 64 seeds at least 48 scenes have a hit pixel and at least 32 a partly
occluded one (0 < occluded < rays).  The frame keeps the scene's own camera and
is cut to 24x17 at most, so a camera that looks past the cloud stays one.
"""
import numpy as np

import ao_ref
from ao_fuzz import RAYS, SEEDS, model


def test_cases_hit_and_are_partly_occluded(oracle):
    hit = partly = full = 0
    radii = set()
    for seed in range(SEEDS):
        m = model(seed, oracle)
        e = m["exp"]
        h = e["gbuffer"]["sphere"] != ao_ref.NO_HIT
        occ = e["occluded"]
        hit += bool(h.any())
        partly += bool(((occ > 0) & (occ < RAYS)).any())
        full += bool((occ == RAYS).any())
        radii.add(np.isinf(m["case"]["radius"]))
    print(f"ao fuzz: {hit} scenes with a hit pixel, {partly} with a partly occluded one, {full} with a fully "
          f"occluded one")
    assert hit >= 48 and partly >= 32
    assert radii == {True, False}
