"""The megakernel finishes the units of a tile no camera ray can hit a sphere from without tracing
them (TraceArgs::empty_on): each sample adds the background once, with the additions
a traced miss performs.  Every frame is bit-identical (max|d| = 0) to oracle Tier B, the counting
pass's samples, segments and sphere tests are the oracle's, and the units and samples finished
without tracing (untraced_units, untraced_samples) are those of the HOST evaluation of the rule
(tests/native/beam_empty_check.cpp, checked against exact rays by tests/test_beam_empty_host.py),
so no case passes without the shortcut and none with a tile too many."""
import numpy as np
import pytest

from helpers import to_oracle_scene
from sky_helpers import GROUND, HOLLOW, MOVER, gpu_check, host_empty_for, narrow
from tail_helpers import materials, spheres

pytestmark = pytest.mark.gpu

ASPECT = 16 / 9


@pytest.fixture(scope="module")
def cover(rtw, oracle):
    from rtw_amd.device import TorchRenderer
    sph, mats, _ = rtw.cover_scene(42)
    return sph, to_oracle_scene(oracle, sph, mats), TorchRenderer(sph, mats, 0), rtw.cover_camera(ASPECT)


def test_a_cover_frame_chunks_3_3_1(rtw, oracle, cover):
    sph, osc, rend, cam = cover
    _, st, empty = gpu_check(rtw, oracle, rend, sph, osc, cam, "A", width=128, height=72, spp=7, chunk=3)
    assert len(empty) == 9
    assert st["untraced_units"] == 9 * 64 * 3 and st["untraced_samples"] == 9 * 64 * 7
    # the same counts from a launch that cannot take the shortcut (the wavefront engine)
    ref = rend.counts(cam, rtw.make_params(width=128, height=72, spp=7, chunk=3, engine="wavefront", wf_paths=4096))
    got = rend.counts(cam, rtw.make_params(width=128, height=72, spp=7, chunk=3))
    for k in ("samples", "segments", "static_tests", "moving_tests"):
        assert got[k] == ref[k], (k, got, ref)


@pytest.mark.parametrize("depth", [0, 1, 2])
def test_b_depth_limits(rtw, oracle, cover, depth):
    """Depth 0: a sample adds nothing, not the background, so nothing is finished untraced and the frame is black."""
    sph, osc, rend, cam = cover
    g, st, _ = gpu_check(rtw, oracle, rend, sph, osc, cam, f"B depth {depth}", width=128, height=72, spp=7, chunk=3,
                         max_depth=depth)
    if depth == 0:
        assert st["untraced_units"] == 0 and (g == 0).all()
    else:
        assert st["untraced_units"] == 9 * 64 * 3


@pytest.mark.parametrize("kw,some", [(dict(width=100, height=72), True),
                                     (dict(width=128, height=72, row_begin=1, row_stride=3), False),
                                     (dict(width=128, height=72, row_begin=0, row_stride=2), None),
                                     (dict(width=384, height=216, row_begin=1, row_stride=3), True)],
                         ids=["width 100", "rows 1::3", "rows 0::2", "384x216 rows 1::3"])
def test_c_padded_tiles_and_row_shards(rtw, oracle, cover, kw, some):
    """A padded tile column (its padding units are not counted); row shards, where a tile's 8 rows span 8 *
    row_stride image rows: in rows 1::3 of 128x72 the first tile row reaches below the horizon and the host
    rule proves no tile, so the larger frame has that shard with proven tiles."""
    sph, osc, rend, cam = cover
    _, st, empty = gpu_check(rtw, oracle, rend, sph, osc, cam, f"C {kw}", spp=7 if kw["width"] < 200 else 4, chunk=3, **kw)
    if some is not None:
        assert (st["untraced_units"] > 0 and len(empty) > 0) == some


def test_d_only_background(rtw, oracle, cover):
    """The cover camera turned upwards: every unit is finished untraced, no closest hit runs, and the frame is
    the quantised background."""
    sph, osc, rend, _ = cover
    cam = rtw.camera_init((13, 2, 3), (13, 12, 3), (0, 0, 1), 20.0, ASPECT, 0.1, 10.0, 0.0, 1.0)
    bg = (0.1, 0.7, 1 / 3)
    g, st, empty = gpu_check(rtw, oracle, rend, sph, osc, cam, "D", width=100, height=50, spp=7, chunk=3, background=bg)
    assert len(empty) == 13 * 7
    assert st["untraced_units"] == 100 * 50 * 3 and st["untraced_samples"] == st["samples"] == 100 * 50 * 7
    assert st["sphere_loop_wave_iters"] == 0 and st["primary_rounds"] == 0 and st["primary_idle_lanes"] == 0
    s = [0.0, 0.0, 0.0]
    for c in (3, 3, 1):  # the chunk sums as the kernel adds them, then the finalize kernel's additions
        for k in range(3):
            t = 0.0
            for _ in range(c):
                t += bg[k]
            s[k] += t
    want = [int(256.0 * max(0.0, min(float(np.sqrt(x * (1.0 / 7))), 0.999))) for x in s]
    assert (g.reshape(-1, 3) == np.array(want, np.uint8)).all(), (want, g[0, 0])


def test_e_f64_sums_are_the_masked_kernels(rtw, cover):
    """The f64 chunk sums themselves, which 8-bit pixels round away: a 20-sample pass of one unit per pixel with
    bg = (0.1, 0.7, 1/3) against the same pass through the masked kernel (the rotated loop, no shortcut), on
    all pixels but one.  20 additions of 0.1 are not 20 * 0.1."""
    import torch
    from rtw_amd.device import TorchAccumulator
    sph, _, rend, cam = cover
    bg = (0.1, 0.7, 1 / 3)
    p = rtw.make_params(width=128, height=72, spp=20, chunk=20, background=bg)
    st = rend.stats(cam, p)
    assert st["untraced_units"] == 9 * 64
    a = TorchAccumulator(rend.scene, p)
    a.render_pass(cam, 20)
    torch.cuda.synchronize()
    sa, _ = a.read()
    a.close()
    mask = np.ones((72, 128), np.uint8)
    mask[71, 127] = 0
    b = TorchAccumulator(rend.scene, p)
    b.set_mask(mask)
    b.render_pass(cam, 20)
    torch.cuda.synchronize()
    sb, _ = b.read()
    b.close()
    empty = host_empty_for(sph, cam, p)["empty"]
    t = empty[0]
    px = sa.reshape(72, 128, 3)[8 * (t // 16), 8 * (t % 16)]
    acc = [0.0, 0.0, 0.0]
    for _ in range(20):
        acc = [x + y for x, y in zip(acc, bg)]
    assert list(px) == acc and acc[0] != 20 * 0.1
    assert np.array_equal(sb[mask != 0], sa[mask != 0])


@pytest.fixture(scope="module")
def big_spheres(rtw, oracle):
    from rtw_amd.device import TorchRenderer
    mats = materials(rtw)
    out = {}
    for name, extra in (("hollow", (HOLLOW[:2] + (HOLLOW[2], 0.0, 0.0, 0, 3))), ("mover", MOVER[:2] + (MOVER[2], 0.0, 1.0, 1, 1))):
        specs = [GROUND[:2] + (1000.0, 0.0, 0.0, 0, 0), extra]
        specs += [(c0, c1, r, t0, t1, mv, 1 + k % 3) for k, (c0, c1, r, t0, t1, mv) in enumerate(narrow(14, 21))]
        sph = spheres(rtw, specs)
        out[name] = (sph, to_oracle_scene(oracle, sph, mats), TorchRenderer(sph, mats, 0))
    return out


def test_f_hollow_and_moving_wide_spheres(rtw, oracle, cover, big_spheres):
    """A glass shell of radius -150 around the camera: no tile is untraced.  A radius-120 sphere moving into the
    right part of the sky: the tiles under its travel are traced (the count is the host rule's, which
    tests/test_beam_empty_host.py holds inside the empty tiles of both shutter ends), the others are not."""
    cam = cover[3]
    sph, osc, rend = big_spheres["hollow"]
    _, st, empty = gpu_check(rtw, oracle, rend, sph, osc, cam, "F hollow", width=128, height=72, spp=4, chunk=3)
    assert empty == [] and st["untraced_units"] == 0 and st["primary_rounds"] > 0
    sph, osc, rend = big_spheres["mover"]
    _, st, empty = gpu_check(rtw, oracle, rend, sph, osc, cam, "F mover", width=128, height=72, spp=4, chunk=3)
    still = spheres(rtw, [(s.c0[:], s.c1[:], s.radius, s.t0, s.t1, s.moving, s.mat) for i, s in enumerate(sph) if i != 1])
    without = host_empty_for(still, cam, rtw.make_params(width=128, height=72, spp=4))["empty"]
    assert 0 < len(empty) < len(without) and set(empty) < set(without)


@pytest.mark.parametrize("at_y,tiles", [(0.0, 0), (1.5, 32)])
def test_g_defocus(rtw, oracle, cover, at_y, tiles):
    """Aperture 2.0: with the cover camera's aim the lens disk of radius 1 widens every beam of the top tile row
    down to the ground, and the host rule proves no tile; aimed 1.5 higher it proves two tile rows."""
    sph, osc, rend, _ = cover
    cam = rtw.camera_init((13, 2, 3), (0, at_y, 0), (0, 1, 0), 20.0, ASPECT, 2.0, 10.0, 0.0, 1.0)
    _, st, empty = gpu_check(rtw, oracle, rend, sph, osc, cam, f"G aperture 2 at y {at_y}", width=128, height=72, spp=7,
                             chunk=3)
    assert len(empty) == tiles and st["untraced_units"] == tiles * 64 * 3


def test_h_with_tail_dealing(rtw, oracle, cover):
    sph, osc, rend, cam = cover
    _, st, _ = gpu_check(rtw, oracle, rend, sph, osc, cam, "H", width=128, height=72, spp=40)
    assert st["tail_helped_samples"] > 0 and st["untraced_units"] == 9 * 64 * 2
