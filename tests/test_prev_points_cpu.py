"""rtw_world_prev_points_host on the CPU: where a hit's surface
point lies under the previous frame's numbers.  Worlds: the small mixed world of
helpers.mixed_bvh_world (spheres, moving spheres, rects and boxes under
Translate / RotateY chains) and the Cornell box (boxes under Translate +
RotateY); hits: the oracle's records of query_helpers' ray sets.  Every hit of a
set enters every comparison (a record whose oracle root is NaN, scene 6's ray in
a rect's plane, is no hit: query_helpers.verified drops it).  No GPU."""
import numpy as np
import pytest

from helpers import _rot, chain_to_object, chain_to_world
from query_helpers import get_world, verified

TOL = 1e-9  # absolute: coordinates below 1e3, f64 carries 2e-16 relative over a handful of operations
DELTA = np.array([0.37, -0.21, 0.55])
PHI = 0.31


@pytest.fixture(scope="module")
def W(rtw):
    from rtw_amd import world
    return world


@pytest.fixture(scope="module", params=["small", "scene6"])
def case(request, rtw, oracle, W):
    w = get_world(rtw, oracle, W, request.param)
    rays, hits, _ = verified(w)
    a, xv = W.desc_numbers(w.desc)
    d = w.desc
    prims = [dict(kind=d.prims[i].kind, xform=d.prims[i].xform) for i in range(d.n_prims)]
    xf = [dict(n=d.xforms[i].n, op=list(d.xforms[i].op), v=[tuple(xv[i, k]) for k in range(4)]) for i in range(d.n_xforms)]
    assert (hits["prim"] > 0).sum() >= 100 and (hits["prim"] == 0).sum() >= 10
    return w, rays, hits, a, xv, prims, xf


def test_null_arrays_give_p(W, case):
    w, rays, hits, a, xv, prims, xf = case
    got = W.prev_points_host(w.desc, hits, 0.5)
    hit = hits["prim"] > 0
    assert got[hit].tobytes() == np.ascontiguousarray(hits["p"][hit]).tobytes()
    assert (got[~hit].view(np.uint64) == 0).all()


def test_same_numbers_give_p(W, case):
    """The arrays given, with this frame's values: the point itself, to rounding (each hit at its own ray's time)."""
    w, rays, hits, a, xv, prims, xf = case
    for i in np.nonzero(hits["prim"] > 0)[0]:
        got = W.prev_points_host(w.desc, hits[i:i + 1], float(rays["time"][i]), a, xv)
        assert np.abs(got[0] - hits["p"][i]).max() <= TOL, (i, got[0], hits["p"][i])


def assert_misses_are_zero(W, w, hits, a_prev, xv_prev):
    """The set in one call with the arrays given: every real miss (prim == 0) gets three +0.0, and a hit between
    misses the value it gets alone."""
    miss = hits["prim"] == 0
    assert miss.sum() >= 10
    got = W.prev_points_host(w.desc, hits, 0.5, a_prev, xv_prev)
    assert (got[miss].view(np.uint64) == 0).all()
    for i in np.nonzero(~miss)[0][:5]:
        alone = W.prev_points_host(w.desc, hits[i:i + 1], 0.5, a_prev, xv_prev)
        assert got[i].tobytes() == alone[0].tobytes()


def _linear(x, v):
    return chain_to_world(x, v) - chain_to_world(x, np.zeros(3))


def test_sphere_centres_moved_by_delta(W, case):
    """a_prev = every sphere centre (both ends of a moving sphere) minus DELTA: a sphere's point moves by -DELTA
    (through the linear part of its chain, if it has one); a rect's stays."""
    w, rays, hits, a, xv, prims, xf = case
    a_prev = a.copy()
    sph = np.array([p["kind"] <= 1 for p in prims])
    a_prev[sph, 0:3] -= DELTA
    a_prev[sph, 3:6] -= DELTA
    n = 0
    for i in np.nonzero(hits["prim"] > 0)[0]:
        got = W.prev_points_host(w.desc, hits[i:i + 1], float(rays["time"][i]), a_prev, None)[0]
        p = prims[hits["prim"][i] - 1]
        want = np.array(hits["p"][i])
        if p["kind"] <= 1:
            want = want - (_linear(xf[p["xform"]], DELTA) if p["xform"] >= 0 else DELTA)
            n += 1
        assert np.abs(got - want).max() <= TOL, (i, p, got, want)
    assert n > 0 or w.name == "scene6"  # (the Cornell box has no sphere: its rects must stay)
    assert_misses_are_zero(W, w, hits, a_prev, None)


def test_rotations_advanced_by_phi(W, case):
    """xv_prev = every RotateY angle advanced by PHI: the point taken to object space through the current
    chain and back to the world through the advanced one, stated with helpers.chain_to_object / chain_to_world."""
    w, rays, hits, a, xv, prims, xf = case
    xv_prev, xf_prev = xv.copy(), []
    for i, x in enumerate(xf):
        v = list(x["v"])
        for k in range(x["n"]):
            if x["op"][k] == 1:
                v[k] = _rot(v[k][2] + PHI)
                xv_prev[i, k] = v[k]
        xf_prev.append(dict(n=x["n"], op=x["op"], v=v))
    moved = 0
    for i in np.nonzero(hits["prim"] > 0)[0]:
        got = W.prev_points_host(w.desc, hits[i:i + 1], float(rays["time"][i]), None, xv_prev)[0]
        p = prims[hits["prim"][i] - 1]
        want = np.array(hits["p"][i])
        if p["xform"] >= 0:
            want = chain_to_world(xf_prev[p["xform"]], chain_to_object(xf[p["xform"]], want))
            moved += np.abs(want - hits["p"][i]).max() > 1e-3
        assert np.abs(got - want).max() <= TOL, (i, p, got, want)
    assert moved >= 10  # hits under a rotation did enter
    assert_misses_are_zero(W, w, hits, None, xv_prev)
    assert_misses_are_zero(W, w, hits, a, xv_prev)


def test_refused_arguments(rtw, W, case):
    w, rays, hits, a, xv, prims, xf = case
    with pytest.raises(rtw.RtwError) as e:
        W.prev_points_host(w.desc, hits, np.nan)
    assert e.value.status == rtw.RTW_EINVAL
    with pytest.raises(ValueError):
        W.prev_points_host(w.desc, hits, 0.5, a[:-1])
    beyond = hits[:4].copy()
    beyond["prim"] = w.desc.n_prims + 1  # a prim beyond the list: treated as a miss
    assert (W.prev_points_host(w.desc, beyond, 0.5, a, xv) == 0).all()
