"""Deforming meshes: updates and rebuilds of a DYNAMIC world that holds triangles.

A level-3 icosphere (1280 triangles) among spheres; its vertices are rotated and deformed in a torch (n, 9) float64
tensor (a triangle's row is its three vertices).  After rtw_amd.device.update_world the tables equal
rtw_world_refit_tables_host's byte for byte — the derived n, h come from the device's fill_record — and renders and
queries equal a freshly created world's; the same after rebuild_world (tables: the rebuild's host twin).  An
update that holds one degenerate and one NaN triangle is RTW_EINVAL and leaves the tables as they were."""
import numpy as np
import pytest

from helpers import _to_desc
import query_helpers as Q
from test_gpu_world_general import Dev, assert_same
from test_gpu_world_update import same_tables
import tri_helpers as T

pytestmark = pytest.mark.gpu

SKY = (0.7, 0.8, 1.0)


@pytest.fixture(scope="module")
def W():
    from rtw_amd import world
    return world


def build(W, v, f, seed=5):
    rng = np.random.default_rng(seed)
    tex = [dict(kind=W.TEX_CHECKER, odd=(0.2, 0.3, 0.1), even=(0.9, 0.9, 0.9)), dict(kind=W.TEX_SOLID, color=(0.7, 0.4, 0.3))]
    mats = [dict(kind=W.WMAT_LAMBERT, tex=0), dict(kind=W.WMAT_LAMBERT, tex=1), dict(kind=W.WMAT_METAL, albedo=(0.9, 0.9, 0.9), fuzz=0.0)]
    prims = [dict(kind=W.PRIM_SPHERE, mat=0, xform=-1, a=[0, -1000, 0, 0, -1000, 0, 1000.0, 0, 0])]
    for i in range(60):
        r = float(rng.uniform(0.2, 0.5))
        c = (float(rng.uniform(-8, 8)), r, float(rng.uniform(-6, 6)))
        prims.append(dict(kind=W.PRIM_SPHERE, mat=1 + i % 2, xform=-1, a=[*c, *c, r, 0, 0]))
    prims += T.mesh_dicts(W, v, f, 1)
    return prims, [], tex, mats, [], []


def deform(v, phase):
    w = T.rot_y(v - np.array([0.0, 2.5, 0.0]), 0.6 * phase)
    w = w * (1.0 + 0.25 * np.sin(3.0 * w[:, 1:2] + phase))
    return w + np.array([0.5 * phase, 2.5, 0.0])


def probe(rtw, W, desc_or_dev, cam, rays):
    """(render, records) of a world: a 40x40x8 frame and a batch of rays."""
    dev = desc_or_dev
    p = rtw.make_params(40, 40, 8, background=SKY)
    hits, _ = Q._trace(rtw, dev.dw, Q.to_device(rays), len(rays))
    return dev.render(rtw, cam, p), hits


def test_update_and_rebuild_of_a_deforming_mesh(rtw, W):
    import torch
    from rtw_amd.device import rebuild_world, update_world
    v0, f = T.icosphere(3)
    v0 = v0 * 2.0 + np.array([0.0, 2.5, 0.0])
    assert len(f) == 1280
    tables0 = build(W, v0, f)
    desc0, keep0 = _to_desc(W, *tables0)
    a0, _ = W.desc_numbers(desc0)
    cam = rtw.camera_init((0.0, 4.0, 12.0), (0.0, 2.0, 0.0), (0, 1, 0), 40.0, 1.0, 0.0, 12.0, 0.0, 1.0)
    rows = []
    for y in range(24):
        for x in range(24):
            rows.append(((0.0, 4.0, 12.0), (-4.5 + 9.0 * x / 23, 2.5 - 6.0 * y / 23, -12.0), 0.5, 0.001, np.inf))
    rays = Q.make_rays(rtw, rows)
    dyn = Dev.__new__(Dev)  # (Dev's render and close over a DYNAMIC world)
    dyn.dw = W.DeviceWorld(desc0, dynamic=True)
    try:
        n = dyn.dw.table_bytes()
        assert dyn.dw.bvh_info()["max_leaf"] == 1 and dyn.dw.launch_info(rtw.make_params(40, 40, 8))["feature_set"] & 64
        same_tables(dyn.dw.read_tables(), W.refit_tables_host(desc0, W.WORLD_DYNAMIC, n), "as created")
        for step, entry in ((1, "update"), (2, "rebuild"), (3, "update")):
            tables1 = build(W, deform(v0, 0.7 * step), f)
            desc1, keep1 = _to_desc(W, *tables1)
            a1, _ = W.desc_numbers(desc1)
            assert not np.array_equal(a1, a0)
            t = torch.from_numpy(a1).cuda()
            (update_world if entry == "update" else rebuild_world)(dyn.dw, t)
            torch.cuda.synchronize()
            got = dyn.dw.read_tables()
            if entry == "update" and step == 1:
                same_tables(got, W.refit_tables_host(desc0, W.WORLD_DYNAMIC, n, a1), "update")
            elif entry == "rebuild":
                same_tables(got, W.rebuild_tables_host(desc0, W.WORLD_DYNAMIC, n, a1), "rebuild")
                a_rb = a1
            else:
                same_tables(got, W.rebuild_tables_host(desc0, W.WORLD_DYNAMIC, n, a_rb, then_a=a1), "update after rebuild")
            fresh = Dev(W, desc1)
            try:
                (r_got, h_got), (r_want, h_want) = probe(rtw, W, dyn, cam, rays), probe(rtw, W, fresh, cam, rays)
                assert_same(r_got, r_want, f"{entry} {step}: render against a fresh world")
                Q._assert_records(h_got, h_want, f"{entry} {step}: records against a fresh world")
                tri_hits = (h_want["prim"] > 61).mean()
                assert tri_hits > 0.1, tri_hits
            finally:
                fresh.close()
        # one degenerate and one NaN triangle: refused, nothing written
        before = dyn.dw.read_tables()
        bad = a1.copy()
        bad[100, 3:6], bad[100, 6:9] = bad[100, 0:3], bad[100, 0:3]
        bad[900, 4] = np.nan
        for entry in (update_world, rebuild_world):
            with pytest.raises(rtw.RtwError) as e:
                entry(dyn.dw, torch.from_numpy(bad).cuda())
            assert e.value.status == rtw.RTW_EINVAL and "100" in str(e.value), str(e.value)
            torch.cuda.synchronize()
            same_tables(dyn.dw.read_tables(), before, "a refused update left the tables")
    finally:
        dyn.close()
