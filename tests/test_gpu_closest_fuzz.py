"""rt_query_closest on every query_fuzz.py case against the brute force of
tests/closest_ref.py.  The other closest tests run the
generator's cloud and hand-made lattices; these 64 scenes have a grown,
non-cubic root box, radii over three decades, leaf capacities 1..16, depths
1..8 and root-is-leaf trees.

Per seed, one renderer with the case's tree and a cell table picked by the
seed (auto, none, a fixed depth); the case's 520 probes with the mixes'
radius substitution (own, +inf, 0.05 by i % 3); k in {1, 4, 16}, with and
without skip_self.  No tolerance: every comparison is of bits or integers.
"""
import numpy as np
import pytest

import raytracingstudy_amd as rt

import closest_ref as cr
from query_fuzz import BAD_PROBES, NO_HIT, SEEDS, query_case
from test_gpu_closest import _assert_answer, _bits

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", range(SEEDS))
def test_closest_is_the_reference(gpu, seed):
    c = query_case(seed)
    pr = cr.with_cutoffs(c["probes"])
    cell_table = (None, 0, 1 + seed % c["depth"])[seed % 3]
    refs = {skip: cr.reference(c["sp"], pr, cr.K_MAX, skip_self=skip) for skip in (False, True)}
    with rt.KernelRenderer(c["w"], c["h"], mode="scene", cell_table=cell_table) as r:
        r.resize(c["w"], c["h"])
        r.setIntrinsic(c["K"])
        r.setPosition(c["pose"])
        info = r.set_scene(c["sp"], c["al"], max_depth=c["depth"], leaf_capacity=c["leaf"])
        for skip, ref in refs.items():
            for k in (1, 4, 16):
                dist, sphere, count, *st = r.query_closest(pr, k, skip_self=skip, stats=(k == 4))
                _assert_answer((dist, sphere, count), cr.cut(ref, k), pr, k, f"seed {seed} skip={skip} k={k}")
                # the case's bad probes that the substitution left bad (a centre component, R = -1)
                bad = ~cr.probe_ok(pr[BAD_PROBES])
                assert np.all(sphere[BAD_PROBES][bad] == NO_HIT) and not count[BAD_PROBES][bad].any()
                assert np.array_equal(_bits(dist[BAD_PROBES][bad]),
                                      _bits(np.repeat(pr[BAD_PROBES][bad, 3:4], k, axis=1)))
                for a in st:
                    assert int(count.sum()) <= a.prims_tested <= len(pr) * info["n_prim_refs"]
                    assert 0 < a.nodes_visited <= len(pr) * info["n_nodes"]
                    assert (a.primary_rays, a.shadow_rays) == (0, 0) and a.ms > 0.0
    assert (refs[False][3] > 0).sum() >= 200   # (a third of the probes is unbounded)
