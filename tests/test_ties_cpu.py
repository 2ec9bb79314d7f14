"""The exact-tie scenes (tie_scenes.py) on the CPU: the constructions do tie,
the oracle resolves every tie to the lower index, and an image
under the reversed rule would differ, so the GPU half (test_gpu_ties.py) can
fail.
"""
import numpy as np
import pytest

import tie_scenes as ts


@pytest.fixture(scope="module")
def scenes():
    sc = {k: f() for k, f in ts.SCENES.items()}
    sc["T"] = ts.tangent_pairs()
    return sc


@pytest.mark.parametrize("name,floor", [("D", 200), ("M", 100), ("T", 324)])
def test_pairs_tie_and_the_lower_index_wins(oracle, scenes, name, floor):
    """Each member traced alone gives the bit-equal t on at least 90% of the
    intended rays, and there are at least `floor` such ties (M: the centre
    column and row; T: every ray); on every one of them where the pair is the
    nearest hit, the oracle's brute-force trace and its walk name the lower
    index at that t."""
    sc = scenes[name]
    rays = sc.get("rays")
    p, x, y, eq = ts.ties(oracle, sc, rays)
    assert eq.sum() >= 0.9 * eq.shape[0] and eq.sum() >= floor, (int(eq.sum()), eq.shape[0])
    if name == "T":
        assert eq.all() and eq.shape[0] == rays.shape[0]
    s = oracle.Scene(sc["sp"], sc["al"], **(ts.T_TREE if name == "T" else {}))
    o, P, K = np.array(ts.CAM, np.float32), ts.pose(), ts.intrinsic()
    pairs, decided, orders = sc["pairs"], 0, set()
    for k in np.flatnonzero(eq):
        if rays is None:
            oo, d = o, oracle.get_ray(P, K, float(x[k]), float(y[k]))
        else:
            oo, d = rays[x[k], 0:3], rays[x[k], 4:7]
        hb, tb, jb, _ = s.trace(oo, d, brute=True)
        hw, tw, jw, _ = s.trace(oo, d)
        assert hb and hw and jb == jw and tb == tw
        if jb in pairs[p[k]]:
            assert jb == pairs[p[k]].min(), f"pair {pairs[p[k]]}: the tie went to {jb}"
            decided += 1
            if name == "T":
                assert np.float32(tb) == sc["t"][x[k]]
                orders.add(bool(sc["sp"][jb, 3] < sc["sp"][pairs[p[k]].max(), 3]))
            elif name == "M":
                ax = sc["axis"][p[k]]
                orders.add(bool(sc["sp"][jb, ax] < ts.CAM[ax]))
    assert decided >= floor // 2
    if name != "D":
        assert orders == {False, True}    # the winner is the left / small sphere on some, the other on others
    s.close()


@pytest.mark.parametrize("name", ["D", "M"])
def test_the_reversed_rule_would_show(oracle, scenes, name):
    """The oracle's image of the same spheres in the opposite index order (the
    larger index wins every tie) differs on at least 100 pixels."""
    sc = scenes[name]
    img, _, _ = oracle.Scene(sc["sp"], sc["al"]).render(ts.W, ts.H, ts.pose(), ts.intrinsic(), spp=1,
                                                      jitter=False)
    rev, _, _ = oracle.Scene(*ts.reversed_scene(sc)).render(ts.W, ts.H, ts.pose(), ts.intrinsic(), spp=1,
                                                            jitter=False)
    assert int((img != rev).any(-1).sum()) >= 100
