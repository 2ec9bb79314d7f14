"""rt_render_indirect on every indirect_fuzz.py case against
tests/indirect_ref.py, bit for bit, counters included.  The other tests run the
generator's cloud under the default light; these 64 scenes have a grown,
non-cubic root box, radii over three decades, leaf capacities 1..16, depths 1..8
and the plain fuzz's cameras, intrinsics, lights, ambient terms and shadow
switches.  Per seed, one renderer with the case's tree and a cell table picked by
the seed (auto, none, a fixed depth); a stats launch and a plain one.
"""
import pytest

import raytracingstudy_amd as rt

from indirect_fuzz import RAYS, SEEDS, model
from test_gpu_indirect import _assert_equal, _assert_stats, _run

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", range(SEEDS))
def test_layer_is_the_reference(gpu, oracle, seed):
    m = model(seed, oracle)
    c, exp = m["case"], m["exp"]
    cell_table = (None, 0, 1 + seed % c["depth"])[seed % 3]
    with rt.KernelRenderer(c["w"], c["h"], mode="scene", cell_table=cell_table, light_dir=c["light"],
                           ambient=c["ambient"], shadows=c["shadows"]) as r:
        r.resize(c["w"], c["h"])
        r.setIntrinsic(c["K"])
        r.setPosition(c["pose"])
        r.set_scene(c["sp"], c["al"], max_depth=c["depth"], leaf_capacity=c["leaf"])
        got = _run(r, c["w"], c["h"], RAYS, c["radius"], c["salt"], c["sky_scale"], stats=True)
        _assert_equal(got, exp)
        _assert_stats(got["stats"], exp, c["w"], c["h"])
        _assert_equal(_run(r, c["w"], c["h"], RAYS, c["radius"], c["salt"], c["sky_scale"]), exp)
