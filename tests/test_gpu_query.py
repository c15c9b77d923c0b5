"""Ray queries on the GPU (rtw_hip.h "ray queries"): closest hit
and occlusion of caller-supplied rays over worlds and scenes, against the
oracle's rw_hit (OracleWorld.hit / TableWorld.hit) bit for bit — records are
compared as uint64 words, no tolerance, no ray left out.

Worlds: scene 6 (linear loop, rects, boxes under Translate / RotateY), 5
(rects + spheres), 4 with the synthetic map (sphere uv), 3, scene 1 as a world
(a BVH; moving spheres) and scene 7 (9,982 primitives) with the union and the
per-lane walk, helpers.mixed_bvh_world "small" and its swap twin (every kind,
chains, negative radii, coincident pairs; union walk) and "spheres_image" (520
spheres; both walks).  Ray sets: tests/query_helpers.py (feature rays with
their own times, bounces, inward rays, shadow rays with t_max = 1), plus for
scene 6 axis-aligned rays and one ray lying in a rect's plane (a 0/0 root),
and for the mixed worlds rays aimed at each coincident pair."""
import ctypes as C

import numpy as np
import pytest

import query_helpers as Q
from query_helpers import _assert_records, _trace

pytestmark = pytest.mark.gpu

import torch  # noqa: E402  (device buffers and streams)

# (world, traversal asked, traversal rtw_world_query_info must report)
CASES = [("scene6", "auto", "linear"), ("scene6", "lane", "linear"), ("scene5", "auto", "linear"),
         ("scene4", "auto", "linear"), ("scene3", "auto", "linear"),
         ("scene1", "union", "union"), ("scene1", "lane", "lane"), ("scene7", "union", "union"),
         ("scene7", "lane", "lane"), ("small", "auto", "union"), ("small", "lane", "union"),
         ("small_swap", "auto", "union"), ("spheres_image", "union", "union"), ("spheres_image", "lane", "lane")]
SIZES = (1, 63, 64, 65, 257)


@pytest.fixture(scope="module")
def W():
    from rtw_amd import world
    return world


@pytest.fixture(scope="module")
def worlds(rtw, oracle, W):
    def get(name):
        return Q.get_world(rtw, oracle, W, name)
    return get


def test_ray_sets_cannot_pass_vacuously(worlds):
    for name in ("scene1", "scene3", "scene4", "scene5", "scene6", "scene7", "small", "small_swap", "spheres_image"):
        w = worlds(name)
        main = slice(0, w.n_main)
        Q.check_conditions(w.rays[main], w.kinds[main], w.ref[main], w.moving if name in ("scene1", "scene7") else None)
        assert np.isnan(w.ref["t"]).sum() == (1 if name == "scene6" else 0), name
    w = worlds("scene6")
    assert (w.ref["prim"][w.kinds == "x"] > 0).all()  # the axis-aligned rays start inside the box: all hit
    assert (w.rays["dir"][w.kinds == "x"] == 0.0).any(axis=1).all()


@pytest.mark.parametrize("name,asked,runs", CASES, ids=[f"{c[0]}-{c[1]}" for c in CASES])
def test_trace_and_occluded_equal_the_oracle(rtw, worlds, name, asked, runs):
    w = worlds(name)
    opts = rtw.query_opts(asked)
    assert w.dev.query_info(opts)["traversal"] == runs
    n_all = len(w.rays)
    first = None
    for n in (*SIZES, n_all, n_all):  # prefixes of the same set; the full set twice
        got, guard = _trace(rtw, w.dev, w.d_rays, n, opts)
        assert (guard == 0xA5).all(), (name, n)
        _assert_records(got, w.ref[:n], (name, asked, n))
        if n == n_all:
            if first is None:
                first = got
            else:
                assert Q.words(first).tobytes() == Q.words(got).tobytes()  # the same input, the same bytes
        occ, guard = _trace(rtw, w.dev, w.d_rays, n, opts, occluded=True)
        assert (guard == 0xA5).all(), (name, n)
        assert (occ == (w.ref["prim"][:n] > 0).astype(np.uint8)).all(), (name, asked, n)


@pytest.mark.parametrize("name", ["scene1", "scene7", "spheres_image"])
def test_lane_walk_gives_the_union_walks_bytes(rtw, worlds, name):
    w = worlds(name)
    a, _ = _trace(rtw, w.dev, w.d_rays, len(w.rays), rtw.query_opts("union"))
    b, _ = _trace(rtw, w.dev, w.d_rays, len(w.rays), rtw.query_opts("lane"))
    c, _ = _trace(rtw, w.dev, w.d_rays, len(w.rays), None)  # AUTO, opts NULL
    assert Q.words(a).tobytes() == Q.words(b).tobytes() == Q.words(c).tobytes()


def _axis_rays(rtw, W, desc):
    """Rays whose direction has two components exactly 0 (+0 and -0), aimed at spheres spread over the list
    from outside them along each axis: a batch of nothing else, so no lane's box tests can lean on a
    neighbour's (the union walk descends where ANY lane's box test passes)."""
    idx = [i for i in range(desc.n_prims) if desc.prims[i].kind == W.PRIM_SPHERE and 0 < desc.prims[i].a[6] < 50]
    idx = idx[::max(1, len(idx) // 24)]
    rows = []
    for j, i in enumerate(idx):
        # (off the centre by a little: a ray in the plane y = r of spheres resting on the ground lies in the
        # plane of a rect placed there, the reference's 0/0 case, which scene 6's own ray covers)
        c, r = np.array(desc.prims[i].a[0:3]) + np.array([0.0137, 0.0071, -0.0113]), desc.prims[i].a[6]
        z = -0.0 if j % 2 else 0.0
        for axis in range(3):
            o, d = c.copy(), np.array([z, z, z])
            o[axis] += r + 2.5
            d[axis] = -1.0 - 0.25 * (j % 3)
            rows.append((o, d, 0.5, 0.001, np.inf if j % 4 else 3.0))
    return Q.make_rays(rtw, rows)


@pytest.mark.parametrize("name,asked", [("scene1", "union"), ("scene1", "lane"), ("scene7", "lane"), ("small", "auto"),
                                        ("spheres_image", "union"), ("spheres_image", "lane")])
def test_axis_aligned_rays_through_the_bvh(rtw, W, worlds, name, asked):
    w = worlds(name)
    rays = _axis_rays(rtw, W, w.desc)
    ref = Q.oracle_hits(rtw, w.oracle, rays)
    assert len(rays) >= 36 and 0.5 <= (ref["prim"] > 0).mean() and np.isfinite(ref["t"]).all()
    assert ((rays["dir"] == 0.0).sum(axis=1) == 2).all()
    d_rays = torch.from_numpy(np.frombuffer(rays.tobytes(), np.uint8).copy()).cuda()
    opts = rtw.query_opts(asked)
    for n in (1, len(rays)):
        got, guard = _trace(rtw, w.dev, d_rays, n, opts)
        assert (guard == 0xA5).all()
        _assert_records(got, ref[:n], (name, asked, n))
        occ, _ = _trace(rtw, w.dev, d_rays, n, opts, occluded=True)
        assert (occ == (ref["prim"][:n] > 0)).all(), (name, asked, n)


@pytest.mark.parametrize("name", ["small", "small_swap"])
def test_coincident_pairs_later_index_wins(rtw, worlds, name):
    w = worlds(name)
    got, _ = _trace(rtw, w.dev, w.d_rays, len(w.rays), None)
    assert len(w.pairs) == 3
    for cls, later, rows in w.pairs:
        prims = [int(w.ref["prim"][w.n_main + r]) - 1 for r in rows]
        in_pair = [p for p in prims if p >= 0 and w.tables[0][p]["cls"] == cls]
        assert in_pair, (cls, prims)  # at least one ray's winner belongs to the pair ...
        assert all(p == later for p in in_pair), (cls, prims, later)  # ... and is its later list index
        assert [int(got["prim"][w.n_main + r]) - 1 for r in rows] == prims


def test_scene_api_equals_the_world_of_scene_1(rtw, worlds):
    w = worlds("scene1")
    sph, mats, _ = rtw.cover_scene(42)
    sc = rtw.DeviceScene(sph, mats)
    n = len(w.rays)
    a, ga = _trace(rtw, sc, w.d_rays, n, is_world=False)
    b, _ = _trace(rtw, w.dev, w.d_rays, n, None)
    assert (ga == 0xA5).all()
    assert Q.words(a).tobytes() == Q.words(b).tobytes()
    oa, ga = _trace(rtw, sc, w.d_rays, n, occluded=True, is_world=False)
    ob, _ = _trace(rtw, w.dev, w.d_rays, n, None, occluded=True)
    assert (ga == 0xA5).all() and (oa == ob).all() and (oa == (w.ref["prim"] > 0)).all()
    for m in (1, 65):
        c, g = _trace(rtw, sc, w.d_rays, m, is_world=False)
        assert (g == 0xA5).all() and Q.words(c).tobytes() == Q.words(a[:m]).tobytes()
    assert Q.words(sc.trace_host(w.rays[:70])).tobytes() == Q.words(a[:70]).tobytes()
    sc.close()


@pytest.mark.parametrize("name", ["scene6", "scene7"])
def test_torch_tracer_and_host_form(rtw, worlds, name):
    from rtw_amd.device import TorchTracer
    w = worlds(name)
    ok = ~np.isnan(w.ref["t"])
    rays, ref = w.rays[ok], w.ref[ok]
    tr = TorchTracer(w.dev)
    o, d = torch.from_numpy(rays["origin"].copy()).cuda(), torch.from_numpy(rays["dir"].copy()).cuda()
    time, t_max = torch.from_numpy(rays["time"].copy()).cuda(), torch.from_numpy(rays["t_max"].copy())
    h = tr.trace(o, d, time=time, t_min=0.001, t_max=t_max)
    torch.cuda.synchronize()
    assert h["prim"].dtype == torch.int64 and h["front"].dtype == torch.bool
    assert (h["prim"].cpu().numpy() == ref["prim"].astype(np.int64) - 1).all()
    assert (h["prim"].cpu().numpy()[ref["prim"] == 0] == -1).all()
    assert Q.words(h["records"].cpu().numpy().view(rtw.HIT_DTYPE).reshape(-1)).tobytes() == Q.words(ref).tobytes()
    for key, field in (("t", "t"), ("p", "p"), ("normal", "normal")):
        assert h[key].cpu().numpy().tobytes() == np.ascontiguousarray(ref[field]).tobytes(), key
    assert (h["uv"].cpu().numpy() == np.stack([ref["u"], ref["v"]], axis=1)).all()
    assert (h["front"].cpu().numpy() == (ref["front"] != 0)).all()
    occ = tr.occluded(o, d, time=time, t_max=t_max)
    assert occ.dtype == torch.bool and (occ.cpu().numpy() == (ref["prim"] > 0)).all()
    assert tr.trace(o[:0], d[:0])["prim"].numel() == 0
    # the host form (rtw_world_trace) on one batch
    assert Q.words(w.dev.trace_host(rays[:300])).tobytes() == Q.words(ref[:300]).tobytes()


def test_errors(rtw, worlds):
    w = worlds("scene5")
    L = rtw.lib()
    n = 64
    out = torch.full((n * 80 + 8,), 0xA5, dtype=torch.uint8, device="cuda")
    rp, op = w.d_rays.data_ptr(), out.data_ptr()

    def trace(world, rays, count, hits, opts=None):
        return L.rtw_world_trace_device(world, C.c_void_p(rays), count, opts, C.c_void_p(hits), None)

    def msg():
        return (L.rtw_last_error() or b"").decode()

    for args in ((None, rp, n, op), (w.dev.h, None, n, op), (w.dev.h, rp, n, None),      # null pointers
                 (w.dev.h, rp + 4, n, op), (w.dev.h, rp, n, op + 4),                        # misaligned
                 (w.dev.h, rp, (1 << 31) + 1, op)):                                        # n > 2^31
        assert trace(*args) == rtw.RTW_EINVAL and "rtw_world_trace_device" in msg(), args
    assert trace(w.dev.h, rp, n, op, C.byref(rtw.QueryOpts(3, 0))) == rtw.RTW_EINVAL
    assert L.rtw_world_occluded_device(w.dev.h, None, n, None, C.c_void_p(op), None) == rtw.RTW_EINVAL
    assert L.rtw_world_trace(w.dev.h, None, n, None, C.c_void_p(op)) == rtw.RTW_EINVAL
    sph, mats, _ = rtw.cover_scene(42)
    sc = rtw.DeviceScene(sph, mats)
    assert L.rtw_scene_trace_device(sc.h, C.c_void_p(rp + 4), n, C.c_void_p(op), None) == rtw.RTW_EINVAL
    assert "rtw_scene_trace_device" in msg()
    assert L.rtw_scene_occluded_device(sc.h, C.c_void_p(rp), n, None, None) == rtw.RTW_EINVAL
    # n == 0: RTW_OK, nothing launched, the output untouched
    assert trace(w.dev.h, rp, 0, op) == rtw.RTW_OK
    assert L.rtw_world_occluded_device(w.dev.h, C.c_void_p(rp), 0, None, C.c_void_p(op), None) == rtw.RTW_OK
    assert L.rtw_scene_trace_device(sc.h, C.c_void_p(rp), 0, C.c_void_p(op), None) == rtw.RTW_OK
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0xA5).all()
    sc.close()
