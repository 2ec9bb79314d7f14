"""The query fuzz cases (query_fuzz.py) on the CPU, before a GPU sees them: on
every ray the oracle is given, its nearest walk equals the brute-force
reference's first slot, so the two references the GPU test compares against
agree on these scenes; and the 64 cases together reach the paths they are for
(the coverage table below), judged from the references alone.
"""
import numpy as np
import pytest

import multihit_ref as mr
from query_fuzz import (N_ORACLE, N_OWN, N_SURFACE, NO_HIT, SEEDS, model)


@pytest.mark.parametrize("seed", range(SEEDS))
def test_oracle_walk_is_the_brute_force_first_slot(oracle, seed):
    """Hit flag, sphere and t bits of oracle.Scene.trace (the octree walk) equal
    the first slot of multihit_ref's brute force over all spheres, on the 512
    rays the oracle is given; the 8 bad rays are empty in the reference."""
    m = model(seed, oracle)
    rays = m["case"]["rays"]
    hit, t, sphere, _, _ = m["nearest"]
    bt, bs, bc = mr.cut(m["multi"], rays, 1)
    n = N_ORACLE
    assert np.array_equal(bc[:n] == 1, hit[:n])
    assert np.array_equal(bs[:n, 0], sphere[:n])
    assert np.array_equal(bt[:n, 0].view(np.uint32), t[:n].view(np.uint32))
    assert np.all(m["multi"][3][n:] == 0) and np.all(bs[n:] == NO_HIT)
    assert np.array_equal(bt[n:, 0].view(np.uint32), rays[n:, 7].view(np.uint32))
    # any-hit answers the same question: the same rays hit
    assert np.array_equal(m["any"][0], hit)


def test_the_cases_reach_the_paths(oracle):
    """Conditions on the distribution, not on the product: where one fails,
    change query_case or add seeds, never the floors.  Over the 64 cases
    (32,768 rays given to the oracle, 33,280 probes), floor and measured:

      rays with a hit                                          >= 16000    23860
      rays with no hit                                         >=  4000     8908
      rays with 3 spheres or more                              >=  4000     7706
      rays with more than 16 spheres                           >=  1000     2443
        in scenes                                              >=     6       10
      rays whose any-hit sphere differs from the nearest       >=  2000     3873
      nearest hits on a sphere centred outside [0, 1.28]^3     >=  6000    12276
      surface rays whose set changes with the window (0, inf)  >=  1000     2294
      probes with a non-empty set                              >= 10000    20307
      probes with the MORE bit at k = 16                       >=  1500     3003
      own-sphere probes with a contact under skip_self         >=  1500     3461
      overlap-set members centred outside [0, 1.28]^3          >= 13000    26923
      scenes whose grown root box has unequal extents          == 64          64
      cases whose camera hits something                        >=    48       60
      overall pixel hit share                                  0.2 to 0.8 0.523
    """
    got = dict(hit=0, miss=0, three=0, over16=0, over16_scenes=0, any_differs=0, hit_outside=0, window=0,
               touching=0, more=0, contact=0, member_outside=0, unequal_root=0, camera_hits=0,
               pixels=0, pixel_hits=0)
    for seed in range(SEEDS):
        m = model(seed, oracle, gbuffer=True)
        c = m["case"]
        sp, rays = c["sp"], c["rays"]
        outside = np.any((sp[:, :3] < 0) | (sp[:, :3] > np.float32(1.28)), axis=1)
        hit, _, sphere, _, _ = m["nearest"]
        hit, sphere = hit[:N_ORACLE], sphere[:N_ORACLE]
        total = m["multi"][3][:N_ORACLE]
        got["hit"] += int(hit.sum())
        got["miss"] += int((~hit).sum())
        got["three"] += int((total >= 3).sum())
        got["over16"] += int((total > 16).sum())
        got["over16_scenes"] += bool((total > 16).any())
        got["any_differs"] += int((m["any"][2][:N_ORACLE] != sphere).sum())
        got["hit_outside"] += int(outside[sphere[hit]].sum())
        # the surface rays' short window against the open one: a sphere's root
        # behind 1e-5 or past 0.5 enters or leaves the set
        wide = rays[:N_SURFACE].copy()
        wide[:, 3], wide[:, 7] = 0.0, np.inf
        ws, wt = mr.reference(sp, wide, mr.K_MAX)[1::2]
        got["window"] += int(((wt != total[:N_SURFACE]) | np.any(ws != m["multi"][1][:N_SURFACE], axis=1)).sum())
        idx, _, _, ptotal = m["overlap"]
        got["touching"] += int((ptotal > 0).sum())
        got["more"] += int((ptotal > 16).sum())
        got["contact"] += int((m["overlap_skip"][3][:min(N_OWN, c["n"])] > 0).sum())
        got["member_outside"] += int(outside[idx[idx != NO_HIT]].sum())
        ext = m["root"][1].astype(np.float64) - m["root"][0].astype(np.float64)
        got["unequal_root"] += bool(ext.max() > ext.min())
        assert np.all(m["root"][0] <= c["lo"] + 1e-6) and np.all(m["root"][1] >= c["hi"] - 1e-6)
        px = m["gbuffer"]["sphere"] != NO_HIT
        got["camera_hits"] += bool(px.any())
        got["pixels"] += px.size
        got["pixel_hits"] += int(px.sum())
    share = got["pixel_hits"] / got["pixels"]
    print("query fuzz coverage:", got, f"pixel hit share {share:.3f}")
    assert got["hit"] >= 16000 and got["miss"] >= 4000, got
    assert got["three"] >= 4000, got
    assert got["over16"] >= 1000 and got["over16_scenes"] >= 6, got
    assert got["any_differs"] >= 2000, got
    assert got["hit_outside"] >= 6000, got
    assert got["window"] >= 1000, got
    assert got["touching"] >= 10000 and got["more"] >= 1500, got
    assert got["contact"] >= 1500, got
    assert got["member_outside"] >= 13000, got
    assert got["unequal_root"] == SEEDS, got
    assert got["camera_hits"] >= 48, got
    assert 0.2 <= share <= 0.8, share
