"""rt_sweep_spheres on every query_fuzz.py case against the brute force of
tests/sweep_ref.py.  The other sweep tests run the generator's
cloud and hand-made scenes; these 64 scenes have a grown, non-cubic root box,
radii over three decades, leaf capacities 1..16, depths 1..8 and root-is-leaf
trees.

Per seed, one renderer with the case's tree and a cell table picked by the seed
(auto, none, a fixed depth); the case's 520 rays with directions renormalised
in f32 (its deliberately bad rays as they are, so that the miss rules run), as
radii its probes' radius column with every third radius 0; every combination of
the two flags.  No tolerance: every comparison is of bits or integers.  A seed
that disagrees is a finding about rt_sweep_math.h's slack derivation.

With RT_SWEEP_FUZZ_RECORD set to a path, the per-seed record is appended to it
as JSON lines (profiles/r23/sweep_fuzz_record.jsonl was written that way).
"""
import json
import os

import numpy as np
import pytest

import raytracingstudy_amd as rt

import sweep_ref as sr
from query_fuzz import N_ORACLE, NO_HIT, SEEDS, query_case
from query_scaffold import bits as _bits

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", range(SEEDS))
def test_sweep_is_the_reference(gpu, seed):
    c = query_case(seed)
    rays, radii = sr.fuzz_casts(c)
    cell_table = (None, 0, 1 + seed % c["depth"])[seed % 3]
    ok = sr.cast_ok(rays, radii)
    assert ok[:N_ORACLE].sum() >= 400 and not ok[N_ORACLE:].any()
    record = dict(seed=seed, n_spheres=len(c["sp"]), depth=c["depth"], leaf=c["leaf"], cell_table=cell_table,
                  casts=len(rays), valid=int(ok.sum()), flags={})
    with rt.KernelRenderer(c["w"], c["h"], mode="scene", cell_table=cell_table) as r:
        r.resize(c["w"], c["h"])
        r.setIntrinsic(c["K"])
        r.setPosition(c["pose"])
        info = r.set_scene(c["sp"], c["al"], max_depth=c["depth"], leaf_capacity=c["leaf"])
        for flags in range(4):
            kw = dict(entry_only=bool(flags & sr.ENTRY_ONLY), skip_self=bool(flags & sr.SKIP_SELF))
            et, es = sr.reference(c["sp"], rays, radii, flags)
            t, sphere, *st = r.sweep_spheres(rays, radii, stats=(flags == 1), **kw)
            wrong = np.flatnonzero((sphere != es) | (_bits(t) != _bits(et)))
            record["flags"][flags] = dict(hits=int((es != NO_HIT).sum()), disagree=[int(i) for i in wrong])
            assert not len(wrong), (seed, flags, wrong[:8])
            assert np.all(sphere[~ok] == NO_HIT) and np.array_equal(_bits(t[~ok]), _bits(rays[~ok, 7]))
            for a in st:
                assert 0 < a.nodes_visited <= len(rays) * info["n_nodes"]
                assert int((es != NO_HIT).sum()) <= a.prims_tested <= len(rays) * info["n_prim_refs"]
                assert (a.primary_rays, a.shadow_rays) == (len(rays), 0) and a.ms > 0.0
                record["nodes_visited"], record["prims_tested"] = int(a.nodes_visited), int(a.prims_tested)
    path = os.environ.get("RT_SWEEP_FUZZ_RECORD")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(record) + "\n")
