"""The indirect fuzz cases (indirect_fuzz.py), from the reference alone: every
bounce ray's nearest hit equals the oracle's brute-force loop over all spheres,
and the generator covers what the layer is made of.  Over the 64 seeds (none is
skipped) it counts the bounce rays that escape, hit a lit point, hit a shadowed
one and hit one facing away from the light, and the pixels whose sum mixes sky
and hits; the counts it printed when the cases were written are the floors
asserted below (FLOORS): a change of the generator that loses coverage fails.
"""
import numpy as np

import indirect_ref as ir
from indirect_fuzz import RAYS, SEEDS, model
from plain_fuzz import oracle_scene

# measured on these 64 seeds (printed by the test): the asserted floor of each count
FLOORS = dict(escaped=34551, lit=2055, shadowed=3212, away=4910, mixed=2965, scenes_hit=49)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_bounce_hits_are_the_brute_force_and_the_cases_cover_the_layer(oracle):
    n = dict.fromkeys(FLOORS, 0)
    seen = 0
    sky, radii = set(), set()
    for seed in range(SEEDS):
        m = model(seed, oracle)
        c, e = m["case"], m["exp"]
        seen += 1
        sky.add(c["sky_scale"])
        radii.add(bool(np.isinf(c["radius"])))
        kind = e["kind"]
        n["scenes_hit"] += bool(len(e["pixel"]))
        for name, k in (("escaped", ir.ESCAPED), ("lit", ir.LIT), ("shadowed", ir.SHADOWED), ("away", ir.AWAY)):
            n[name] += int((kind == k).sum())
        if len(e["pixel"]):
            n["mixed"] += int(((kind == ir.ESCAPED).any(axis=1) & (kind != ir.ESCAPED).any(axis=1)).sum())
        s = oracle_scene(oracle, c)
        recs = e["rays"].reshape(-1, 8)
        for r, th, sh in zip(recs, e["hit_t"].reshape(-1), e["hit_sphere"].reshape(-1)):
            hit, tb, ib, _ = s.trace(r[0:3], r[4:7], float(r[3]), float(r[7]), brute=True)
            assert hit == (sh != ir.NO_HIT), seed
            if hit:
                assert (_bits(np.float32(tb))[0], ib) == (_bits(th)[0], sh), seed
        s.close()
        assert e["kind"].shape == (len(e["pixel"]), RAYS)
    print("indirect fuzz:", n)
    assert seen == SEEDS == 64
    assert sky == {0.0, 1.0} and radii == {True, False}
    for name, floor in FLOORS.items():
        assert floor > 0 and n[name] >= floor, (name, n[name], floor)
