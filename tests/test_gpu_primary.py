"""The megakernel's primary-first loop (TraceCfg::kPrimaryFirst): a lane
resolves its camera ray itself from the mask of its tile (csrc/rtw_beam.hpp)
and shades that hit in the same iteration.  Every case is bit-identical
(max|d| = 0) to oracle Tier B, as the rotated loop is, and the counts pass
proves which loop ran (primary_rounds) and that the device's tile masks are
the host's (primary_mask_popcount == the host evaluation of rtw_beam.hpp).
tests/test_gpu_primary_fuzz.py has the cameras and scenes away from the cover's."""
import numpy as np
import pytest

from helpers import diff_stats, host_masks, to_oracle_camera, to_oracle_scene

pytestmark = pytest.mark.gpu

ASPECT = 16 / 9


@pytest.fixture(scope="module")
def cover(rtw, oracle):
    sph, mats, _ = rtw.cover_scene(42)
    return sph, mats, to_oracle_scene(oracle, sph, mats)


def check(rtw, oracle, sph, mats, osc, cam, what, primary=True, **kw):
    """GPU f64 megakernel == oracle Tier B on every channel; the loop that ran; and, when it was the
    primary-first loop, the kernel's mask popcount (one per fetched batch = (tile, chunk)) == the host
    evaluation of rtw_beam.hpp over the tiles, times the chunks."""
    from rtw_amd.device import TorchRenderer
    params = rtw.make_params(**kw)
    g = rtw.render(cam, sph, mats, params)
    okw = dict(kw)
    w, h, spp = okw.pop("width"), okw.pop("height"), okw.pop("spp")
    depth = okw.pop("max_depth", 50)
    if "background" in okw:
        okw["bg"] = okw.pop("background")
    o, _ = oracle.render_tier_b(osc, to_oracle_camera(oracle, cam), w, h, spp, depth=depth, **okw)
    d = diff_stats(g, o)
    print(what, d)
    assert d["max"] == 0, (what, d)
    st = TorchRenderer(sph, mats, 0).stats(cam, rtw.make_params(**kw))
    print(what, st)
    assert st["samples"] == g.shape[0] * g.shape[1] * spp
    if primary and depth > 0:
        # every sample's camera ray went through the primary phase; the ones that missed ended there
        assert st["primary_rounds"] > 0 and st["primary_idle_lanes"] < st["samples"], st
        assert st["primary_mask_popcount"] > 0, st  # some tile's camera rays can hit a narrow sphere
    if primary:
        chunk =min(params.chunk or rtw.DEFAULT_CHUNK, spp)
        hm = host_masks(sph, cam, params)
        print(what, hm)
        assert st["primary_mask_popcount"] == -(-spp // chunk) * hm["popcount"], (st, hm)
    else:
        assert st["primary_rounds"] == 0 and st["primary_idle_lanes"] == 0 and st["primary_mask_popcount"] == 0, st
    return g, st


def spheres(rtw, specs):
    sph = (rtw.Sphere * len(specs))()
    for s, (c0, c1, r, t0, t1, mv, m) in zip(sph, specs):
        s.c0[:], s.c1[:] = c0, c1
        s.radius, s.t0, s.t1, s.moving, s.mat = r, t0, t1, mv, m
    return sph


def materials(rtw):
    M = rtw.Material
    mats = (M * 5)()
    mats[0].kind = rtw.LAMBERT_CHECKER
    mats[0].albedo[:] = (0.9, 0.9, 0.9)
    mats[0].albedo_odd[:] = (0.2, 0.3, 0.1)
    mats[1].kind = rtw.LAMBERT_SOLID
    mats[1].albedo[:] = (0.6, 0.3, 0.2)
    mats[2].kind, mats[2].fuzz = rtw.METAL, 0.2
    mats[2].albedo[:] = (0.8, 0.8, 0.7)
    mats[3].kind, mats[3].ir = rtw.DIELECTRIC, 1.5
    mats[4].kind = rtw.LAMBERT_SOLID
    mats[4].albedo[:] = (0.2, 0.5, 0.8)
    return mats


def scattered(rtw, n_narrow, seed, groups=((0.0, 1.0),), extra=()):
    """The ground, `extra`, and n_narrow small spheres: static ones and movers
    along x, y and z over the time ranges `groups` (all contain the shutter)."""
    rng = np.random.default_rng(seed)
    specs = [((0, -1000, 0), (0, -1000, 0), 1000.0, 0.0, 0.0, 0, 0), *extra]
    for k in range(n_narrow):
        x, z = -6 + 12 * rng.random(), -6 + 12 * rng.random()
        r = 0.15 + 0.3 * rng.random()
        c0 = (x, r, z)
        if k % 4 == 0:
            specs.append((c0, c0, r, 0.0, 0.0, 0, 1 + k % 4))
            continue
        dv = [0.0, 0.0, 0.0]
        dv[k % 4 - 1] = 0.2 + 0.4 * rng.random()
        t0, t1 = groups[k % len(groups)]
        specs.append((c0, tuple(c + d for c, d in zip(c0, dv)), r, t0, t1, 1, 1 + k % 4))
    return spheres(rtw, specs)


def test_tile_padding(rtw, oracle, cover):
    sph, mats, osc = cover
    check(rtw, oracle, sph, mats, osc, rtw.cover_camera(1.0), "9x9 spp 40 chunk 7", width=9, height=9, spp=40, chunk=7)


def test_row_shard(rtw, oracle, cover):
    sph, mats, osc = cover
    check(rtw, oracle, sph, mats, osc, rtw.cover_camera(ASPECT), "48x27 rows 1::3", width=48, height=27, spp=20,
          row_begin=1, row_stride=3)


@pytest.mark.parametrize("depth", [0, 1, 2])
def test_depth_limit(rtw, oracle, cover, depth):
    sph, mats, osc = cover
    g, _ = check(rtw, oracle, sph, mats, osc, rtw.cover_camera(1.0), f"max_depth {depth}", width=16, height=16, spp=8,
                 max_depth=depth)
    if depth == 0:
        assert (g == 0).all()  # rayColor(depth 0) is black (main.zig:105-108)


def test_wide_beam(rtw, oracle, cover):
    sph, mats, osc = cover
    cam = rtw.camera_init((13, 2, 3), (0, 0, 0), (0, 1, 0), 20.0, 1.0, 2.0, 10.0, 0.0, 1.0)
    check(rtw, oracle, sph, mats, osc, cam, "aperture 2.0", width=16, height=16, spp=16)


def test_camera_in_glass(rtw, oracle):
    """The camera inside a narrow glass sphere (and inside a hollow one's shell):
    every camera ray's first hit is that sphere, from inside."""
    extra = [((13.1, 2.0, 3.0), (13.1, 2.0, 3.0), 1.2, 0.0, 0.0, 0, 3),
             ((13.0, 2.1, 3.0), (13.0, 2.1, 3.0), -0.7, 0.0, 0.0, 0, 3)]
    sph, mats = scattered(rtw, 20, 3, extra=extra), materials(rtw)
    g, st = check(rtw, oracle, sph, mats, to_oracle_scene(oracle, sph, mats), rtw.cover_camera(1.0),
                  "camera in glass", width=16, height=16, spp=16)
    assert g.std() > 2
    assert st["primary_idle_lanes"] == 0, st  # no camera ray misses the sphere around the lens


def test_three_time_groups(rtw, oracle):
    groups = ((0.0, 1.0), (-0.5, 1.5), (-1.0, 2.0))
    sph, mats = scattered(rtw, 37, 7, groups=groups), materials(rtw)
    cam = rtw.camera_init((13, 2, 3), (0, 0.3, 0), (0, 1, 0), 30.0, 1.0, 0.1, 10.0, 0.0, 1.0)
    check(rtw, oracle, sph, mats, to_oracle_scene(oracle, sph, mats), cam, "three time groups", width=16, height=16,
          spp=16)


def test_fallback_more_than_one_slot_block(rtw, oracle):
    """70 narrow spheres need more than one 64-slot block: the kernel runs the rotated loop."""
    sph, mats = scattered(rtw, 70, 11), materials(rtw)
    cam = rtw.camera_init((13, 2, 3), (0, 0.3, 0), (0, 1, 0), 30.0, 1.0, 0.1, 10.0, 0.0, 1.0)
    check(rtw, oracle, sph, mats, to_oracle_scene(oracle, sph, mats), cam, "70 narrow spheres", primary=False, width=16,
          height=16, spp=16)


def test_second_batch_mask(rtw, oracle, cover):
    """96x54 at 20 spp: 84 tiles of one chunk each, so the lanes of a wave take
    units of a current and of a newly fetched batch at once, each with the mask
    of its own tile."""
    sph, mats, osc = cover
    check(rtw, oracle, sph, mats, osc, rtw.cover_camera(ASPECT), "96x54 spp 20", width=96, height=54, spp=20)
