"""Rebuilds of dynamic worlds on the GPU (rtw_hip.h "rebuild"):
rtw_world_rebuild / rtw_world_rebuild_device give an uploaded world a new tree
from new numbers (csrc/rtw_world_rebuild.hip), rtw_world_bvh_cost measures a tree.

  * the device tables, cull scalars, bounds and bvh_info after a rebuild are,
    byte for byte, what the host build (rtw_world_rebuild_tables_host) computes,
    through the host-array and the device-array entry; an update after a rebuild
    equals host rebuild + host refit; a rebuild after an update equals the
    rebuild alone (history does not matter);
  * every render, guide buffer, query and accumulator pass of a rebuilt world
    equals that of a world freshly created from the same numbers, and the
    oracle's linear list (bar: test_gpu_parity.assert_parity); the per-lane walk
    stays available;
  * rebuild, then update back: the original world's image;
  * three degenerate worlds (every centre equal, every centre on one line,
    coincident pairs) rebuild and render as fresh worlds;
  * refusals leave the world as it was;
  * bvh_cost equals the same sum in numpy within n_nodes * 2^-52, relative;
  * rtw_render --rebuild-above writes the frames of the run without it.

Inputs: tests/test_gpu_world_update.py's cases (helpers.mixed_bvh_world moved by
update_helpers.displace) and rebuild_helpers.degenerate_world.  Frames: 64x36 at
20 and 40 spp."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from helpers import MIXED_CAMERA, _to_desc, to_oracle_camera
from rebuild_helpers import DEGENERATE, degenerate_world
from test_gpu_parity import SEEDS, assert_parity
from test_gpu_world_update import FH, FW, SKY, Case, apply, assert_same, render, same_tables
from update_helpers import blob_nodes, numbers

pytestmark = pytest.mark.gpu

RTW_EINVAL, RTW_UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def W():
    from rtw_amd import world
    return world


@pytest.fixture(scope="module")
def earth(W):
    return W.earth_map()


@pytest.fixture(scope="module")
def cases(W, oracle, earth):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Case(W, oracle, earth, name)
        return cache[name]
    return get


@pytest.fixture(scope="module")
def cam(rtw, oracle):
    m = MIXED_CAMERA
    c = rtw.camera_init(m["look_from"], m["look_at"], (0, 1, 0), m["vfov"], 16 / 9, m["aperture"], m["focus"], 0.0, 1.0)
    return c, to_oracle_camera(oracle, c)


def rebuild(W, case, dw, entry, a, xv):
    """One rebuild through the host-array or the device-array entry."""
    if entry == "host":
        d, keep = case.desc(W, a, xv)
        dw.rebuild(d)
    else:
        import torch

        from rtw_amd.device import rebuild_world
        rebuild_world(dw, torch.from_numpy(np.ascontiguousarray(a)).cuda(),
                      torch.from_numpy(np.ascontiguousarray(xv)).cuda() if len(xv) else None)


def xv_or_none(xv):
    return xv if len(xv) else None


def same_world(dw, want, what):
    same_tables(dw.read_tables(), want, what)
    assert dw.bvh_info() == want["info"], (what, dw.bvh_info(), want["info"])


# ------------------------------------------------------------------ 1. bytes ----
@pytest.mark.parametrize("entry", ["host", "device"])
@pytest.mark.parametrize("name", ["large", "spheres_image"])
def test_tables_equal_the_host_rebuild(rtw, W, cases, name, entry):
    c = cases(name)
    flags = W.WORLD_DYNAMIC
    dw = W.DeviceWorld(c.desc0, dynamic=True)
    try:
        n = dw.table_bytes()
        info = dw.bvh_info()
        assert info["max_leaf"] == 1 and info["nodes"] == c.desc0.n_prims - 1 > 256, info
        created = dw.read_tables()
        host1 = W.rebuild_tables_host(c.desc0, flags, n, c.a1, xv_or_none(c.xv1))
        assert (host1["blob"] != created["blob"]).sum() > 1000
        rebuild(W, c, dw, entry, c.a1, c.xv1)
        same_world(dw, host1, "rebuild(a1)")
        # an update after a rebuild refits the new topology
        rebuild(W, c, dw, entry, c.a0, c.xv0)
        same_world(dw, W.rebuild_tables_host(c.desc0, flags, n, c.a0, xv_or_none(c.xv0)), "rebuild(a0)")
        apply(W, c, dw, entry, c.a1, c.xv1)
        same_world(dw, W.rebuild_tables_host(c.desc0, flags, n, c.a0, xv_or_none(c.xv0), then_a=c.a1, then_xv=xv_or_none(c.xv1)),
                   "rebuild(a0), update(a1)")
        # history does not matter
        rebuild(W, c, dw, entry, c.a1, c.xv1)
        same_world(dw, host1, "rebuild(a0), update(a1), rebuild(a1)")
        assert dw.table_bytes() == n
        got = dw.bvh_info()
        assert {k: got[k] for k in ("nodes", "leaves", "max_leaf")} == {k: info[k] for k in ("nodes", "leaves", "max_leaf")}
    finally:
        dw.close()


def test_update_then_rebuild_of_a_fresh_world(rtw, W, cases):
    c = cases("large")
    dw = W.DeviceWorld(c.desc0, dynamic=True)
    try:
        apply(W, c, dw, "device", c.a1, c.xv1)
        rebuild(W, c, dw, "device", c.a1, c.xv1)
        same_world(dw, W.rebuild_tables_host(c.desc0, W.WORLD_DYNAMIC, dw.table_bytes(), c.a1, c.xv1), "update(a1), rebuild(a1)")
    finally:
        dw.close()


# ----------------------------------------------------- 2. images, fresh world ----
@pytest.mark.parametrize("name,trav", [("large", "union"), ("spheres_image", "union"), ("spheres_image", "lane")])
def test_rebuilt_world_renders_as_a_fresh_one_and_the_oracle(rtw, W, cases, cam, name, trav):
    c = cases(name)
    dyn = W.DeviceWorld(c.desc0, dynamic=True)
    d1, keep = c.desc(W, c.a1, c.xv1)
    fresh = W.DeviceWorld(d1)
    try:
        rebuild(W, c, dyn, "device", c.a1, c.xv1)
        assert dyn.bvh_info()["max_depth"] <= 16  # kLaneStack
        for spp, seed in ((20, SEEDS[1]), (40, SEEDS[2])):
            p = rtw.make_params(FW, FH, spp, 50, seed, background=SKY, world_traversal=trav)
            assert dyn.launch_info(p)["traversal"] == trav
            got, want = render(rtw, dyn, cam[0], p), render(rtw, fresh, cam[0], p)
            assert_same(got, want, (name, trav, spp))
            assert got[0].std() > 5
            ref = c.oracle1().render_tier_b(cam[1], FW, FH, spp, seed=seed, bg=SKY, threads=16)[0]
            assert_parity(got[0], ref, f"rebuilt {name} {trav} {FW}x{FH}x{spp}")
    finally:
        dyn.close(), fresh.close()


# ------------------------------------------- 3. queries, guides, accumulator ----
def test_queries_guides_and_passes_of_a_rebuilt_world(rtw, oracle, W, cases, cam):
    from query_helpers import _assert_records, _trace, check_conditions, oracle_hits, ray_set, to_device
    from test_gpu_accum import same_image
    from test_gpu_accum_world import accumulate
    from test_gpu_guides import device_guides
    c = cases("large")
    dyn = W.DeviceWorld(c.desc0, dynamic=True)
    d1, keep = c.desc(W, c.a1, c.xv1)
    fresh = W.DeviceWorld(d1)
    try:
        rebuild(W, c, dyn, "host", c.a1, c.xv1)
        rays, kinds = ray_set(rtw, c.oracle1(), cam[0], MIXED_CAMERA["look_from"], 77)
        ref = oracle_hits(rtw, c.oracle1(), rays)
        check_conditions(rays, kinds, ref)
        hits = dyn.trace_host(rays)
        _assert_records(hits, ref, "rebuilt world's queries")
        assert hits.tobytes() == fresh.trace_host(rays).tobytes()
        d_rays = to_device(rays)
        occ = [_trace(rtw, w_, d_rays, rays.size, occluded=True)[0] for w_ in (dyn, fresh)]
        assert (occ[0] == occ[1]).all() and (occ[0] == (ref["prim"] != 0)).all() and 0 < int(occ[0].sum()) < rays.size
        p1 = rtw.make_params(FW, FH, 1, background=SKY)
        g, gf = device_guides(rtw, dyn, cam[0], p1), device_guides(rtw, fresh, cam[0], p1)
        assert g.tobytes() == gf.tobytes() and len(np.unique(g["prim"])) > 10
        p = rtw.make_params(FW, FH, 40, 50, SEEDS[0], background=SKY)
        one_shot = render(rtw, dyn, cam[0], p, counts=False)
        assert same_image(accumulate(rtw, dyn, cam[0], p, [20, 20]), one_shot)
        assert_same(one_shot, render(rtw, fresh, cam[0], p, counts=False), "one shot")
    finally:
        dyn.close(), fresh.close()


# ------------------------------------------------- 4. refit after a rebuild ----
@pytest.mark.parametrize("name,trav", [("large", "union"), ("spheres_image", "lane")])
def test_rebuild_then_update_back_gives_the_original_image(rtw, W, cases, cam, name, trav):
    c = cases(name)
    orig, dyn = W.DeviceWorld(c.desc0), W.DeviceWorld(c.desc0, dynamic=True)
    try:
        p = rtw.make_params(FW, FH, 20, 50, SEEDS[3], background=SKY, world_traversal=trav)
        want = render(rtw, orig, cam[0], p)
        rebuild(W, c, dyn, "device", c.a1, c.xv1)
        moved = render(rtw, dyn, cam[0], p)
        assert (moved[0] != want[0]).any(axis=2).mean() > 0.2  # (the rebuild did change the frame)
        apply(W, c, dyn, "host", c.a0, c.xv0)
        assert_same(render(rtw, dyn, cam[0], p), want, (name, "rebuild, update back"))  # (node visits may differ)
    finally:
        orig.close(), dyn.close()


# --------------------------------------------------------- 5. degenerate worlds ----
@pytest.mark.parametrize("trav", ["union", "lane"])
@pytest.mark.parametrize("kind", DEGENERATE)
def test_degenerate_worlds_rebuild_and_render_as_fresh_ones(rtw, W, cam, kind, trav):
    t0, t1 = degenerate_world(W, kind), degenerate_world(W, kind, moved=True)
    d0, keep0 = _to_desc(W, *t0)
    d1, keep1 = _to_desc(W, *t1)
    a1, xv1 = numbers(t1)
    dyn, fresh = W.DeviceWorld(d0, dynamic=True), W.DeviceWorld(d1)
    try:
        dyn.rebuild(d1)
        same_world(dyn, W.rebuild_tables_host(d0, W.WORLD_DYNAMIC, dyn.table_bytes(), a1), kind)
        p = rtw.make_params(FW, FH, 20, 50, SEEDS[1], background=SKY, world_traversal=trav)
        assert dyn.launch_info(p)["traversal"] == trav
        got = render(rtw, dyn, cam[0], p)
        assert_same(got, render(rtw, fresh, cam[0], p), (kind, trav))
        assert got[0].std() > 2
    finally:
        dyn.close(), fresh.close()


# ---------------------------------------------------------------- 6. refusals ----
def test_refusals_leave_the_world_untouched(rtw, W, cases):
    def refused(dw, f, status, what):
        before = dw.read_tables()
        with pytest.raises(rtw.RtwError) as e:
            f()
        assert e.value.status == status, (what, e.value)
        same_tables(dw.read_tables(), before, what)

    # worlds a rebuild does not support: leaves of two, no BVH; and a frozen world
    for name, kw, status in (("small", dict(dynamic=True), RTW_UNSUPPORTED), ("globe300", dict(dynamic=True), RTW_UNSUPPORTED),
                             ("large", dict(dynamic=True, linear=True), RTW_UNSUPPORTED), ("large", dict(), RTW_EINVAL)):
        c = cases(name)
        dw = W.DeviceWorld(c.desc0, **kw)
        try:
            for entry in ("host", "device"):
                refused(dw, lambda: rebuild(W, c, dw, entry, c.a1, c.xv1), status, (name, kw, entry))
        finally:
            dw.close()
    # numbers an update refuses, and a changed kind
    c = cases("large")
    prims = c.tables0[0]
    sphere = next(i for i, q in enumerate(prims) if q["kind"] == 0)
    moving = next(i for i, q in enumerate(prims) if q["kind"] == 1)
    dw = W.DeviceWorld(c.desc0, dynamic=True)
    try:
        def with_number(i, k, v, entry):
            a = c.a1.copy()
            a[i, k] = v
            return lambda: rebuild(W, c, dw, entry, a, c.xv1)
        for entry in ("host", "device"):
            refused(dw, with_number(sphere, 1, np.nan, entry), RTW_EINVAL, "NaN centre")
            refused(dw, with_number(sphere, 6, np.inf, entry), RTW_EINVAL, "Inf radius")
            refused(dw, with_number(moving, 8, c.a1[moving, 7], entry), RTW_EINVAL, "time1 == time0")
            refused(dw, with_number(moving, 8, c.a1[moving, 7] - 1.0, entry), RTW_EINVAL, "time1 < time0")
        d, keep = c.desc(W, c.a1, c.xv1)
        keep[0][sphere].kind = 1
        refused(dw, lambda: dw.rebuild(d), RTW_EINVAL, "changed kind")
        # the refused rebuilds left the refit's tables alone too: an update still refits the created topology
        apply(W, c, dw, "device", c.a1, c.xv1)
        same_tables(dw.read_tables(), W.refit_tables_host(c.desc0, W.WORLD_DYNAMIC, dw.table_bytes(), c.a1, c.xv1), "update after refusals")
    finally:
        dw.close()


# -------------------------------------------------------------------- 7. cost ----
def numpy_cost(desc, n_nodes, blob):
    b = blob_nodes(desc, n_nodes, blob)[:, 0:12].copy().view(np.float32).astype(np.float64)

    def half_area(lo, hi):
        d = hi - lo
        return (d[..., 0] * d[..., 1] + d[..., 1] * d[..., 2]) + d[..., 2] * d[..., 0]
    lo = np.stack([b[:, 0:6:2], b[:, 1:6:2]], axis=1)   # (n, child, axis)
    hi = np.stack([b[:, 6:12:2], b[:, 7:12:2]], axis=1)
    total = (half_area(lo[:, 0], hi[:, 0]) + half_area(lo[:, 1], hi[:, 1])).sum()
    return total / half_area(lo[0].min(axis=0), hi[0].max(axis=0))


@pytest.mark.parametrize("name", ["large", "spheres_image", "small"])
def test_bvh_cost_is_the_sum_over_the_node_table(rtw, W, cases, name):
    c = cases(name)
    dw = W.DeviceWorld(c.desc0, dynamic=True)
    try:
        n_nodes = dw.bvh_info()["nodes"]
        steps = [("created", lambda: None), ("updated", lambda: apply(W, c, dw, "device", c.a1, c.xv1))]
        if name != "small":
            steps.append(("rebuilt", lambda: rebuild(W, c, dw, "device", c.a1, c.xv1)))
        costs = {}
        for what, f in steps:
            f()
            got, again = dw.bvh_cost(), dw.bvh_cost()
            want = numpy_cost(c.desc0, n_nodes, dw.read_tables()["blob"])
            print(name, what, "bvh_cost", got, "numpy", want, "relative", abs(got - want) / want)
            assert got == again and got > 0.0
            assert abs(got - want) <= n_nodes * 2.0 ** -52 * want, (name, what, got, want)
            costs[what] = got
        assert costs["updated"] != costs["created"]
    finally:
        dw.close()


def test_bvh_cost_of_frozen_and_treeless_worlds(rtw, W, cases):
    c = cases("small")
    frozen, lin = W.DeviceWorld(c.desc0), W.DeviceWorld(c.desc0, linear=True)
    try:
        n_nodes = frozen.bvh_info()["nodes"]
        want = numpy_cost(c.desc0, n_nodes, frozen.read_tables()["blob"])
        assert abs(frozen.bvh_cost() - want) <= n_nodes * 2.0 ** -52 * want
        with pytest.raises(rtw.RtwError) as e:
            lin.bvh_cost()
        assert e.value.status == RTW_UNSUPPORTED
    finally:
        frozen.close(), lin.close()


# ------------------------------------------------------------------------ CLI ----
def test_cli_rebuild_above(rtw, W, earth, tmp_path):
    """bin/rtw_render --frames 3 --orbit 40 on the globe (9,982 primitives): --rebuild-above 0 rebuilds after
    every update (frames 1 and 2) and writes the bytes of the run without the option; with 1e9 nothing
    rebuilds."""
    from test_gpu_world import _write_png
    exe = os.path.join(os.path.dirname(rtw.__file__), "..", "bin", "rtw_render")
    png = str(tmp_path / "earth.png")
    _write_png(png, earth)
    base = [exe, "--scene", "7", "--image", png, "--width", "64", "--spp", "4", "--frames", "3", "--orbit", "40"]
    frames = ["frame_0000.ppm", "frame_0001.ppm", "frame_0002.ppm"]
    out = {}
    for n, extra in (("plain", []), ("always", ["--rebuild-above", "0"]), ("never", ["--rebuild-above", "1e9"])):
        d = tmp_path / n
        d.mkdir()
        r = subprocess.run(base + ["--out", str(d / "out.ppm")] + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        out[n] = ([(d / f).read_bytes() for f in frames], [ln for ln in r.stderr.splitlines() if ln.startswith("rebuild frame=")])
    assert len(set(out["plain"][0])) == 3
    assert out["always"][0] == out["plain"][0] and out["never"][0] == out["plain"][0]
    assert out["plain"][1] == [] and out["never"][1] == []
    assert [ln.split()[1] for ln in out["always"][1]] == ["frame=1", "frame=2"], out["always"][1]
    for ln in out["always"][1]:
        kv = dict(t.split("=") for t in ln.split()[1:])
        assert float(kv["cost_before"]) > 0 and float(kv["cost_after"]) > 0
    r = subprocess.run(base[:-4] + ["--rebuild-above", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--rebuild-above" in r.stderr
