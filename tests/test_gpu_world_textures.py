"""Texture tables past index 0 on the GPU.  Every other world of the suite
names image 0 and Perlin table 0; helpers.textured_world names images 0-3 (a
1x1, a PORTRAIT 5x9 whose rows the reference clamps against width - 1, the
earth map, a 7x3 with alpha-0 texels) and Perlin tables 0-2 (noise scales 4,
0, -2.5), on spheres, rects of each orientation, lights and under Translate /
RotateY chains — so the kernel's table strides, the images' running byte
offsets (pack_world) and the 64-bit pixel offset of tex_value are met away
from 0.  tests/test_world_cpu.py shows on the oracle alone that exchanging any
two tables changes the frame, that the row clamp bites and that the alpha-0
colour is seen.

  * against oracle.TableWorld Tier B at 96x54x8, bar as
    test_gpu_parity.assert_parity, for the world as listed (<= 32 primitives:
    the linear loop), with filler spheres (> 32: a BVH), its noise-only and
    image-only reductions and the spheres-only image world (the feature set
    compiled for such worlds; with filler, the per-lane walk's), each under
    world_features auto and all;
  * BVH == linear, bit for bit (rgb and the f32 mean), as
    test_gpu_world_general.test_mixed_bvh_equals_linear."""
import pytest

from helpers import TEXTURED_BG, TEXTURED_CAMERA, _to_desc, textured_world, to_oracle_camera
from test_gpu_parity import assert_parity
from test_gpu_world_general import Dev, assert_same

pytestmark = pytest.mark.gpu

FW, FH, SPP = 96, 54, 8
# name -> (variant, filler spheres)
WORLDS = {"listed": (None, 0), "filler": (None, 40), "noise": ("noise", 0), "image": ("image", 0),
          "image_spheres": ("image_spheres", 0), "image_spheres_filler": ("image_spheres", 40)}
FEAT_IMAGE, FEAT_ALL = 2, 15  # csrc/rtw_world.hip kFeatImage, kFeatAll


@pytest.fixture(scope="module")
def W():
    from rtw_amd import world
    return world


@pytest.fixture(scope="module")
def cam(rtw, oracle):
    m = TEXTURED_CAMERA
    c = rtw.camera_init(m["look_from"], m["look_at"], (0, 1, 0), m["vfov"], 16 / 9, m["aperture"], m["focus"], 0.0, 1.0)
    return c, to_oracle_camera(oracle, c)


@pytest.fixture(scope="module")
def textured(W, oracle, cam):
    """name -> (desc, oracle Tier-B frame); each world built and its reference rendered once."""
    earth = W.earth_map()
    cache = {}

    def get(name):
        if name not in cache:
            variant, filler = WORLDS[name]
            t = textured_world(W, earth, variant=variant, filler=filler)
            desc, keep = _to_desc(W, *t)
            ref = oracle.TableWorld(*t, background=TEXTURED_BG).render_tier_b(cam[1], FW, FH, SPP, bg=TEXTURED_BG,
                                                                             threads=16)[0]
            ref.setflags(write=False)
            cache[name] = (desc, ref, keep)
        return cache[name][:2]
    return get


@pytest.mark.parametrize("feat", ["auto", "all"])
@pytest.mark.parametrize("name", list(WORLDS))
def test_textured_world_equals_oracle(rtw, W, textured, cam, name, feat):
    desc, ref = textured(name)
    p = rtw.make_params(FW, FH, SPP, background=TEXTURED_BG, world_features=feat)
    d = Dev(W, desc)
    try:
        li = d.dw.launch_info(p)
        nodes = d.dw.bvh_info()["nodes"]
        rgb, _, c = d.render(rtw, cam[0], p)
    finally:
        d.close()
    print(name, feat, "primitives", desc.n_prims, "bvh nodes", nodes, li)
    assert (nodes > 0) == (desc.n_prims > 32)
    if feat == "all" or not name.startswith("image_spheres"):
        assert li["feature_set"] == FEAT_ALL, li
    else:  # spheres with image textures only: the feature set of its own (plus the lane walk's bits, if chosen)
        assert li["feature_set"] & FEAT_IMAGE and li["feature_set"] != FEAT_ALL and not li["feature_set"] & (FEAT_ALL & ~FEAT_IMAGE), li
    assert c["samples"] == FW * FH * SPP
    assert_parity(rgb, ref, f"textured {name} features {feat}")
    assert rgb.std() > 5


@pytest.mark.parametrize("name", ["filler", "image_spheres_filler"])
def test_textured_bvh_equals_linear(rtw, W, textured, cam, name):
    """The BVH render of the textured world equals the linear loop's bit for
    bit — rgb, the f32 mean, samples, segments — under every traversal request
    and both feature sets."""
    desc, _ = textured(name)
    lin, bvh = Dev(W, desc, linear=True), Dev(W, desc)
    try:
        assert lin.dw.bvh_info()["nodes"] == 0 and bvh.dw.bvh_info()["nodes"] > 0
        ref = lin.render(rtw, cam[0], rtw.make_params(FW, FH, SPP, background=TEXTURED_BG))
        assert ref[2]["samples"] == FW * FH * SPP and ref[0].std() > 5
        seen = set()
        for trav in ("auto", "union", "lane"):
            for feat in ("auto", "all"):
                p = rtw.make_params(FW, FH, SPP, background=TEXTURED_BG, world_traversal=trav, world_features=feat)
                got = bvh.render(rtw, cam[0], p)
                assert_same(got, ref, f"{name} traversal {trav} features {feat}")
                seen.add(got[2]["traversal"])
        print(name, "traversals run:", sorted(seen))
        assert "union" in seen
        if name == "image_spheres_filler":  # (the per-lane walk is compiled for spheres-only worlds)
            assert "lane" in seen
    finally:
        lin.close()
        bvh.close()
