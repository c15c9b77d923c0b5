"""Triangles in the world render (RTW_PRIM_TRIANGLE).

The oracle cannot express a triangle.  An axis-aligned triangle computes the bits of the rect it tiles
(csrc/rtw_tri.hpp), so the oracle's own worlds are exact references for worlds whose rects the device holds as two
triangles each (tri_helpers.rect_tris, wound so that n = +e_k):
  T1  the Cornell box (scene 6), every rect as two triangles (36 primitives: a BVH by default), against the
      oracle's Tier B of scene 6 byte for byte — rgb, the f32 mean, samples, segments;
  T2  helpers.mixed_bvh_world small and large, likewise (rects under an image texture read u, v and stay rects);
  T3  >= kLeafOneMin untransformed spheres plus axis-aligned cards as triangle pairs: linear, union, per lane;
General triangles have no oracle:
  T4a linear == union == lane == features ALL on jittered meshes under every material, some under chains;
  T4b a closed mesh of lights around the camera: every pixel is the quantised emit colour; also with the mesh
      under a 3-op chain, and for a 64-gon bipyramid with the camera aimed at an apex of valence 64.
On the parent every one of these worlds is RTW_EINVAL (kind 5)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import MIXED_CAMERA, MIXED_SIZES, _to_desc, diff_stats, mixed_bvh_world, to_oracle_camera
from test_gpu_world_general import Dev, assert_same
import tri_helpers as T

pytestmark = pytest.mark.gpu

SKY = (0.7, 0.8, 1.0)
FRAMES = ((8, 8, 8), (24, 16, 8), (40, 40, 8))
FS_TRI = 64  # kFeatTri
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEASURE_LIB = os.path.join(REPO, "raytracinginoneweekend.zig_amd", "lib_m", "librtw_hip.so")
# this process is test_plain_ref_lane_sets' child: the development library with RTW_WORLD_UNPACKED=1, under which
# the per-lane walk loads the refs (feature set 64 | 2 | 16 = 82) instead of gathering them from the bounds (114)
UNPACKED = os.environ.get("RTW_WORLD_UNPACKED") == "1"
FS_LANE = 82 if UNPACKED else 114


@pytest.fixture(scope="module")
def W():
    from rtw_amd import world
    return world


@pytest.fixture(scope="module")
def earth(W):
    return W.earth_map()


def assert_oracle(got, ref, what):
    """(rgb, mean, counts) of the device against (rgb, mean, stats) of the oracle: byte for byte."""
    (rg, mg, cg), (ro, mo, so) = got, ref
    assert (rg == ro).all(), (what, diff_stats(rg, ro))
    assert np.array_equal(mg.view(np.uint32), mo.view(np.uint32)), what
    assert cg["samples"] == so["samples"] and cg["segments"] == so["segments"], (what, cg, so)


# ------------------------------------------------------------------------------- T1 ----
@pytest.fixture(scope="module")
def cornell(W, oracle):
    b = W.BuiltScene(6, 42)
    t = b.table()
    tables, n = T.triangulate(W, (t["prims"], t["xforms"], t["textures"], t["materials"], t["perlins"], []))
    assert n == 18 and len(tables[0]) == 36 and all(p["kind"] == W.PRIM_TRIANGLE for p in tables[0])
    desc, keep = _to_desc(W, *tables)
    o = oracle.OracleWorld(6, 42)
    return dict(b=b, desc=desc, keep=keep, o=o, ocam=o.camera(), refs={})


def cornell_ref(c, w, h, spp, depth):
    key = (w, h, spp, depth)
    if key not in c["refs"]:
        c["refs"][key] = c["o"].render_tier_b(c["ocam"], w, h, spp, depth=depth, threads=16, want_mean=True)
    return c["refs"][key]


@pytest.mark.parametrize("linear", [False, True])
def test_t1_cornell_box_of_triangles_equals_the_oracle(rtw, W, cornell, linear):
    b = cornell["b"]
    dev = Dev(W, cornell["desc"], linear=linear)
    try:
        info = dev.dw.bvh_info()
        assert (info["nodes"] == 0) == linear, info
        for w, h, spp in FRAMES:
            for trav, feat in (("auto", "auto"), ("union", "auto"), ("lane", "auto"), ("auto", "all")):
                if linear and (trav, feat) != ("auto", "auto"):
                    continue
                p = rtw.make_params(w, h, spp, 50, 42, background=b.background, world_traversal=trav, world_features=feat)
                got = dev.render(rtw, b.camera(), p)
                assert dev.dw.launch_info(p)["feature_set"] & FS_TRI
                assert_oracle(got, cornell_ref(cornell, w, h, spp, 50), f"cornell {w}x{h} linear {linear} {trav} {feat}")
        for depth in (0, 1, 3):
            w, h, spp = FRAMES[1]
            p = rtw.make_params(w, h, spp, depth, 42, background=b.background)
            assert_oracle(dev.render(rtw, b.camera(), p), cornell_ref(cornell, w, h, spp, depth), f"cornell depth {depth}")
    finally:
        dev.close()


# ------------------------------------------------------------------------------- T2 ----
@pytest.mark.parametrize("size", ["small", "large"])
def test_t2_mixed_world_with_rects_as_triangles_equals_the_oracle(rtw, oracle, W, earth, size):
    orig = mixed_bvh_world(W, earth, *MIXED_SIZES[size], 5)
    tables, n = T.triangulate(W, orig, keep=T.reads_uv(W, orig))
    kinds = [p["kind"] for p in tables[0]]
    assert n >= 60 and W.PRIM_TRIANGLE in kinds and W.PRIM_XY_RECT in kinds and W.PRIM_MOVING_SPHERE in kinds
    assert sum(p.get("cls", "").startswith("pair_") and p["kind"] == W.PRIM_TRIANGLE for p in tables[0]) >= 4
    desc, keep = _to_desc(W, *tables)
    ow = oracle.TableWorld(*orig, background=SKY)
    m = MIXED_CAMERA
    cam = rtw.camera_init(m["look_from"], m["look_at"], (0, 1, 0), m["vfov"], 16 / 9, m["aperture"], m["focus"], 0.0, 1.0)
    ocam = to_oracle_camera(oracle, cam)
    bvh, lin = Dev(W, desc), Dev(W, desc, linear=True)
    try:
        assert bvh.dw.bvh_info()["nodes"] > 0
        for w, h, spp in FRAMES[1:] if size == "large" else FRAMES:
            ref = ow.render_tier_b(ocam, w, h, spp, bg=SKY, threads=16, want_mean=True)
            for dev, trav, feat in ((bvh, "auto", "auto"), (bvh, "union", "all"), (lin, "auto", "auto")):
                p = rtw.make_params(w, h, spp, background=SKY, world_traversal=trav, world_features=feat)
                assert_oracle(dev.render(rtw, cam, p), ref, f"mixed {size} {w}x{h} {trav} {feat} linear {dev is lin}")
    finally:
        bvh.close()
        lin.close()


# ------------------------------------------------------------------------------- T3 ----
def test_t3_cards_among_spheres_walk_per_lane(rtw, oracle, W, earth):
    orig = T.cards_world(W, earth)
    tables, n = T.triangulate(W, orig)
    assert n >= 20 and len(tables[0]) >= 512 + 2 * n
    desc, keep = _to_desc(W, *tables)
    ow = oracle.TableWorld(*orig, background=SKY)
    m = MIXED_CAMERA
    cam = rtw.camera_init(m["look_from"], m["look_at"], (0, 1, 0), m["vfov"], 16 / 9, m["aperture"], m["focus"], 0.0, 1.0)
    ocam = to_oracle_camera(oracle, cam)
    bvh, lin = Dev(W, desc), Dev(W, desc, linear=True)
    try:
        info = bvh.dw.bvh_info()
        assert info["max_leaf"] == 1 and info["nodes"] >= 256, info
        p_lane = rtw.make_params(40, 40, 8, background=SKY, world_traversal="lane")
        li = bvh.dw.launch_info(p_lane)
        assert li["traversal"] == "lane" and li["feature_set"] == FS_LANE, li
        assert bvh.dw.launch_info(rtw.make_params(40, 40, 8, background=SKY))["traversal"] == "lane"  # AUTO too
        seen = set()
        for w, h, spp in FRAMES:
            ref = ow.render_tier_b(ocam, w, h, spp, bg=SKY, threads=16, want_mean=True)
            for dev, trav in ((lin, "auto"), (bvh, "union"), (bvh, "lane")):
                p = rtw.make_params(w, h, spp, background=SKY, world_traversal=trav)
                got = dev.render(rtw, cam, p)
                seen.add((got[2]["traversal"], dev.dw.launch_info(p)["feature_set"]))
                assert_oracle(got, ref, f"cards {w}x{h} {trav} linear {dev is lin}")
        assert {t for t, _ in seen} == {"linear", "union", "lane"}, seen
        print("T3 traversals and feature sets:", sorted(seen))
    finally:
        bvh.close()
        lin.close()


# ------------------------------------------------------------------------------- T4 ----
@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("shutter", [(0.0, 1.0), (0.25, 0.5)])
def test_t4a_general_triangles_every_traversal_agrees(rtw, W, earth, seed, shutter):
    tables = T.general_world(W, seed, earth=earth)  # (with two image-textured meshes: the render's u, v of a triangle)
    assert sum(p["mat"] == len(tables[3]) - 1 for p in tables[0]) == 24
    tri = sum(p["kind"] == W.PRIM_TRIANGLE for p in tables[0])
    assert tri >= 150 and any(p["kind"] == W.PRIM_TRIANGLE and p["xform"] >= 0 for p in tables[0])
    desc, keep = _to_desc(W, *tables)
    c = T.T4_CAMERA
    cam = rtw.camera_init(c["look_from"], c["look_at"], (0, 1, 0), c["vfov"], 1.5, c["aperture"], c["focus"], *shutter)
    bvh, lin = Dev(W, desc), Dev(W, desc, linear=True)
    try:
        assert bvh.dw.bvh_info()["nodes"] > 0
        for w, h, spp in FRAMES[1:]:
            ref = lin.render(rtw, cam, rtw.make_params(w, h, spp, background=SKY))
            assert ref[0].std() > 5 and ref[2]["segments"] > 1.5 * ref[2]["samples"]  # (the frame is not flat, and paths bounce)
            for trav, feat in (("union", "auto"), ("lane", "auto"), ("auto", "all")):
                p = rtw.make_params(w, h, spp, background=SKY, world_traversal=trav, world_features=feat)
                assert_same(bvh.render(rtw, cam, p), ref, f"general seed {seed} {w}x{h} {trav} {feat}")
    finally:
        bvh.close()
        lin.close()


@pytest.mark.parametrize("seed", [1, 2])
def test_t4a_meshes_among_spheres_per_lane(rtw, W, seed):
    """Untransformed meshes among >= 512 spheres: the per-lane walk's triangle sets (packed and plain refs are
    the same tables; AUTO picks packed) against the union walk and the linear loop."""
    rng = np.random.default_rng(seed)
    tex = [dict(kind=W.TEX_SOLID, color=(0.6, 0.5, 0.4)), dict(kind=W.TEX_SOLID, color=(3.0, 3.0, 2.5))]
    mats = [dict(kind=W.WMAT_LAMBERT, tex=0), dict(kind=W.WMAT_METAL, albedo=(0.8, 0.8, 0.9), fuzz=0.1),
            dict(kind=W.WMAT_DIELECTRIC, ir=1.5), dict(kind=W.WMAT_LIGHT, tex=1)]
    prims = [dict(kind=W.PRIM_SPHERE, mat=0, xform=-1, a=[0, -1000, 0, 0, -1000, 0, 1000.0, 0, 0])]
    for i in range(520):
        r = float(rng.uniform(0.15, 0.4))
        c = (float(rng.uniform(-10, 10)), r, float(rng.uniform(-8, 6)))
        prims.append(dict(kind=W.PRIM_SPHERE, mat=i % 3, xform=-1, a=[*c, *c, r, 0, 0]))
    for i in range(10):
        v, f = T.icosphere(1) if i % 2 else T.tetrahedron()
        v = v * rng.uniform(0.6, 1.1) * (1 + 0.1 * rng.uniform(-1, 1, v.shape)) + np.array([rng.uniform(-7, 7), rng.uniform(1.2, 3), rng.uniform(-5, 4)])
        prims += T.mesh_dicts(W, v, f, i % 4)
    desc, keep = _to_desc(W, prims, [], tex, mats, [], [])
    c = T.T4_CAMERA
    cam = rtw.camera_init(c["look_from"], c["look_at"], (0, 1, 0), c["vfov"], 1.5, c["aperture"], c["focus"], 0.0, 1.0)
    bvh, lin = Dev(W, desc), Dev(W, desc, linear=True)
    try:
        w, h, spp = FRAMES[2]
        ref = lin.render(rtw, cam, rtw.make_params(w, h, spp, background=SKY))
        for trav in ("union", "lane"):
            p = rtw.make_params(w, h, spp, background=SKY, world_traversal=trav)
            got = bvh.render(rtw, cam, p)
            assert got[2]["traversal"] == trav and bvh.dw.launch_info(p)["feature_set"] == (FS_LANE if trav == "lane" else 66)
            assert_same(got, ref, f"meshes among spheres seed {seed} {trav}")
    finally:
        bvh.close()
        lin.close()


@pytest.mark.parametrize("seed,linear", [(3, False), (4, False), (3, True)])
def test_t4b_a_closed_mesh_of_lights_leaks_nothing(rtw, W, seed, linear):
    tables = T.enclosure_world(W, seed)
    assert len(tables[0]) == 320
    desc, keep = _to_desc(W, *tables)
    want = np.array([int(256 * min(max(np.sqrt(c), 0.0), 0.999)) for c in T.ENCLOSURE_EMIT], np.uint8)
    dev = Dev(W, desc, linear=linear)
    try:
        for k, (look_at, vfov) in enumerate((((0, 0, -1), 120.0), ((1, 0.3, 0.2), 150.0), ((-0.2, 1, 0.1), 90.0))):
            cam = rtw.camera_init((0.3, -0.2, 0.4), look_at, (0, 1, 0) if k < 2 else (1, 0, 0), vfov, 1.0, 0.2, 1.0, 0.0, 1.0)
            for trav in ("union", "lane"):
                p = rtw.make_params(40, 40, 8, background=(0.0, 0.0, 0.0), world_traversal=trav)
                rgb, mean, counts = dev.render(rtw, cam, p)
                bad = (rgb != want).any(axis=2)
                assert not bad.any(), (seed, linear, k, trav, int(bad.sum()), rgb[bad][:4].tolist(), want.tolist())
                assert counts["segments"] == counts["samples"]  # every sample ends at its first hit
    finally:
        dev.close()


def _assert_all_emit(rtw, W, tables, cams, frame, what):
    """Every pixel of every camera is the quantised emit colour, through the BVH (union and lane requests) and
    the linear loop; every sample ends at its first hit."""
    desc, keep = _to_desc(W, *tables)
    want = np.array([int(256 * min(max(np.sqrt(c), 0.0), 0.999)) for c in T.ENCLOSURE_EMIT], np.uint8)
    w, h, spp = frame
    for linear in (False, True):
        dev = Dev(W, desc, linear=linear)
        try:
            assert (dev.dw.bvh_info()["nodes"] == 0) == linear
            for k, cam in enumerate(cams):
                for trav in ("union",) if linear else ("union", "lane"):
                    p = rtw.make_params(w, h, spp, background=(0.0, 0.0, 0.0), world_traversal=trav)
                    rgb, mean, counts = dev.render(rtw, cam, p)
                    bad = (rgb != want).any(axis=2)
                    assert not bad.any(), (what, linear, k, trav, int(bad.sum()), rgb[bad][:4].tolist(), want.tolist())
                    assert counts["segments"] == counts["samples"]
        finally:
            dev.close()


def test_t4b_closed_mesh_under_a_chain_leaks_nothing(rtw, W):
    """T4b's enclosure held in the object space of a 3-op chain (RotateY, Translate, RotateY) that puts it back
    around the camera: the rays reach the inside test through to_object's roundings."""
    from helpers import chain_to_object
    prims, _, tex, mats, perl, imgs = T.enclosure_world(W, 5)
    xf = dict(n=3, op=[W.XF_ROTATE_Y, W.XF_TRANSLATE, W.XF_ROTATE_Y],
              v=[(float(np.sin(0.8)), float(np.cos(0.8)), 0.8), (1.5, -0.75, 2.25), (float(np.sin(-1.9)), float(np.cos(-1.9)), -1.9)])
    for q in prims:
        q["xform"] = 0
        q["a"] = [float(c) for v in np.array(q["a"]).reshape(3, 3) for c in chain_to_object(xf, v)]
    assert len(prims) == 320
    cams = [rtw.camera_init((0.3, -0.2, 0.4), look_at, (0, 1, 0) if k < 2 else (1, 0, 0), vfov, 1.0, 0.2, 1.0, 0.0, 1.0)
            for k, (look_at, vfov) in enumerate((((0, 0, -1), 120.0), ((1, 0.3, 0.2), 150.0), ((-0.2, 1, 0.1), 90.0)))]
    _assert_all_emit(rtw, W, (prims, [xf], tex, mats, perl, imgs), cams, (40, 40, 8), "enclosure under a chain")


def test_t4b_bipyramid_apex_of_valence_64_leaks_nothing(rtw, W):
    """A 64-gon bipyramid of lights around the camera, the camera aimed at an apex where 64 triangles meet (and
    once at the other): 64x64 at 4 spp, every sample inside the fan."""
    from tri_exact import bipyramid
    v, f = bipyramid(64, 6.0, 5.0)
    rng = np.random.default_rng(6)
    v = T.rot_y(v * (1 + 0.03 * rng.uniform(-1, 1, v.shape)), 0.37)[:, [1, 2, 0]] * np.array([1.0, 1.2, 0.9])  # (no face axis-aligned)
    tex = [dict(kind=W.TEX_SOLID, color=T.ENCLOSURE_EMIT)]
    mats = [dict(kind=W.WMAT_LIGHT, tex=0)]
    tables = (T.mesh_dicts(W, v, f, 0), [], tex, mats, [], [])
    assert len(tables[0]) == 128
    eye = (0.2, 0.1, -0.15)
    cams = [rtw.camera_init(eye, tuple(float(c) for c in v[64 + k]), (0, 1, 0), vfov, 1.0, 0.05, 1.0, 0.0, 1.0)
            for k, vfov in ((0, 20.0), (0, 90.0), (1, 2.0))]
    _assert_all_emit(rtw, W, tables, cams, (64, 64, 4), "bipyramid")


@pytest.mark.skipif(UNPACKED, reason="this is the child")
@pytest.mark.skipif(not os.path.exists(MEASURE_LIB), reason="no development library (make lib_m/librtw_hip.so)")
def test_plain_ref_lane_sets():
    """The per-lane triangle set with plain refs (82) is reachable only through the development library's
    RTW_WORLD_UNPACKED knob: T3 and the meshes-among-spheres cases once more in a child process under it, where
    they assert that set and the same frames (the oracle's; the linear loop's)."""
    env = dict(os.environ, RTW_LIB_PATH=MEASURE_LIB, RTW_WORLD_UNPACKED="1")
    p = subprocess.run([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider", os.path.abspath(__file__), "-m", "gpu",
                        "-k", "t3_cards or meshes_among_spheres"], env=env, capture_output=True, text=True)
    assert p.returncode == 0 and "3 passed" in p.stdout, p.stdout[-3000:] + p.stderr[-2000:]
