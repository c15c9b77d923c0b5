"""Feature buffers on the GPU: rtw_scene_guides_device and
rtw_world_guides_device against the oracle, pixel by pixel — World.hit and
rw_texture_value on the feature ray of rtw_hip.h (tests/denoise_helpers.py).

prim is compared exactly; normal, depth and albedo to 1e-6 absolute-or-relative
(f32 rounding is 6e-8; the rest is margin for equal formulas in another
operation order).  At most 2 pixels of a frame may disagree, and each of those
must have a 4-neighbour whose oracle primitive differs — a silhouette, where a
grazing root may flip.  Anything else fails."""
import numpy as np
import pytest

from denoise_helpers import oracle_guides

pytestmark = pytest.mark.gpu

TOL = 1e-6


@pytest.fixture(scope="module")
def Wd():
    from rtw_amd import world
    return world


def device_guides(rtw, target, cam, p):
    import torch
    g = torch.full((p.row_count, p.width, 32), 0xA5, dtype=torch.uint8, device="cuda:0")
    target.guides(cam, p, g.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return g.cpu().numpy().view(rtw.GUIDE_DTYPE)[..., 0]


def compare(got, want, what):
    """The issue's rule; returns the number of silhouette pixels that disagreed."""
    prim = want["prim"]
    bad = got["prim"].astype(np.int64) != prim
    for f in ("normal", "depth", "albedo"):
        w = want[f]
        d = np.abs(got[f].astype(np.float64) - w) > TOL * np.maximum(1.0, np.abs(w))
        bad |= d if d.ndim == 2 else d.any(axis=-1)
    ys, xs = np.nonzero(bad)
    print(f"{what}: {len(ys)} of {bad.size} pixels disagree; prims hit {len(np.unique(prim))}, misses {(prim == 0).sum()}")
    assert len(ys) <= 2, (what, len(ys), list(zip(ys, xs))[:8])
    h, w = prim.shape
    for y, x in zip(ys, xs):
        nb = [prim[j, i] for j, i in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)) if 0 <= j < h and 0 <= i < w]
        assert any(n != prim[y, x] for n in nb), (what, "a disagreement away from any silhouette", int(y), int(x),
                                                  got[y, x], {k: want[k][y, x] for k in want})
    return len(ys)


def world_case(rtw, oracle, Wd, scene_id, w, h, image=None, rows=None, want_bvh=None):
    b = Wd.BuiltScene(scene_id, 42, image=image)
    ow = oracle.OracleWorld(scene_id, 42, image=image)
    cam = b.camera(w / h)
    kw = {} if rows is None else dict(row_begin=rows[0], row_stride=rows[1], row_count=rows[2])
    p = rtw.make_params(w, h, 1, background=b.background, **kw)
    dw = Wd.DeviceWorld(b.desc)
    if want_bvh is not None:
        assert (dw.bvh_info()["nodes"] > 0) == want_bvh
    got = device_guides(rtw, dw, cam, p)
    image_rows = None if rows is None else [rows[0] + k * rows[1] for k in range(rows[2])]
    want = oracle_guides(oracle, ow, cam, w, h, b.background, image_rows)
    compare(got, want, f"world scene {scene_id} {w}x{h} rows {rows}")
    dw.close()
    return got, want


def test_cover_scene_through_both_apis(rtw, oracle, Wd):
    w, h = 60, 33
    got_w, want = world_case(rtw, oracle, Wd, 1, w, h)
    assert (want["prim"] == 0).any() and len(np.unique(want["prim"])) > 20  # sky, ground and many spheres
    ow = oracle.OracleWorld(1, 42)
    kinds = {ow.w.mats[ow.w.prims[int(k) - 1].mat].kind for k in np.unique(want["prim"]) if k}
    assert kinds >= {oracle.RW_LAMBERT, oracle.RW_METAL, oracle.RW_DIELECTRIC}
    sph, mats, _ = rtw.cover_scene(42)
    cam = rtw.cover_camera(w / h)
    sc = rtw.DeviceScene(sph, mats)
    got_s = device_guides(rtw, sc, cam, rtw.make_params(w, h, 1))
    compare(got_s, want, "scene API cover 60x33")
    sc.close()


def test_cover_scene_row_block(rtw, oracle, Wd):
    w, h = 60, 33
    sph, mats, _ = rtw.cover_scene(42)
    cam = rtw.cover_camera(w / h)
    sc = rtw.DeviceScene(sph, mats)
    p = rtw.make_params(w, h, 1, row_begin=5, row_stride=1, row_count=9)
    got = device_guides(rtw, sc, cam, p)
    assert got.shape == (9, w)
    want = oracle_guides(oracle, oracle.OracleWorld(1, 42), cam, w, h, rtw.COVER_BACKGROUND, range(5, 14))
    compare(got, want, "scene API rows 5..13")
    sc.close()
    world_case(rtw, oracle, Wd, 1, w, h, rows=(5, 1, 9))
    world_case(rtw, oracle, Wd, 6, 40, 40, rows=(3, 4, 9))  # a strided shard too


@pytest.mark.parametrize("scene_id,w,h", [(3, 48, 27), (4, 48, 27), (5, 48, 27), (6, 40, 40)])
def test_world_scenes(rtw, oracle, Wd, scene_id, w, h):
    image = Wd.synthetic_world_map() if scene_id == 4 else None
    got, want = world_case(rtw, oracle, Wd, scene_id, w, h, image=image)
    assert (want["prim"] > 0).sum() > w * h // 4
    if scene_id in (3, 4):  # a texture that varies over the surface
        assert len(np.unique(want["albedo"][want["prim"] > 0].round(6), axis=0)) > 20
    if scene_id == 5:  # the rect light and the sphere light are seen, with their emit colour
        assert (want["albedo"].max(axis=-1) > 1.0).any()
    if scene_id == 6:  # boxes under Translate / RotateY: normals that are no axis
        n = want["normal"][want["prim"] > 0]
        assert ((np.abs(n) > 0.05).sum(axis=-1) >= 2).any()


def test_sphere_world_with_a_bvh(rtw, oracle, Wd):
    """The cover scene as a world: a few hundred spheres, so rtw_world_create builds a BVH
    (the guide kernel walks the list itself and must not depend on it)."""
    world_case(rtw, oracle, Wd, 1, 37, 21, want_bvh=True)
