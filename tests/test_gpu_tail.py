"""The megakernel's tail dealing (TraceArgs::tail_on): once a wave's queue is dry,
its lanes without a unit trace the next samples of the wave's other units, and the owner adds them
in sample order.  Every frame is bit-identical (max|d| = 0) to oracle Tier B; the counting pass
traced every sample once (samples, segments = the oracle's) and proves that samples were handed
out (tail_helped_samples).  These frames have fewer units than the launch has lanes, so a wave's
queue is dry from its second take on and the tail copy of the loop runs for most of the launch."""
import numpy as np
import pytest

from helpers import to_oracle_scene
from tail_helpers import check, materials, oracle_frame, scattered

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cover(rtw, oracle):
    from rtw_amd.device import TorchRenderer
    sph, mats, _ = rtw.cover_scene(42)
    return sph, mats, to_oracle_scene(oracle, sph, mats), TorchRenderer(sph, mats, 0), rtw.cover_camera(1.0)


FRAMES = [
    ("sky, ground and spheres", dict(width=16, height=16, spp=40), True),
    ("padded tiles, chunk 7", dict(width=9, height=9, spp=40, chunk=7), True),
    ("one-sample units", dict(width=8, height=8, spp=45, chunk=1), False),
    ("chunk 33 of 140", dict(width=8, height=8, spp=140, chunk=33), True),
    ("chunk 70 of 140", dict(width=8, height=8, spp=140, chunk=70), True),
    ("row shard 1::3", dict(width=48, height=27, spp=20, row_begin=1, row_stride=3), True),
    ("two full tiles, one chunk", dict(width=16, height=8, spp=20), True),
]


@pytest.mark.parametrize("what,kw,helped", FRAMES, ids=[f[0] for f in FRAMES])
def test_cover_frames(rtw, oracle, cover, what, kw, helped):
    sph, mats, osc, rend, cam = cover
    check(rtw, oracle, rend, sph, mats, osc, cam, what, helped=helped, **kw)


@pytest.mark.parametrize("depth", [0, 1, 2, 50])
def test_depth_limits(rtw, oracle, cover, depth):
    """Depth 0: every sample ends at once, black.  Depth 1 and 2: a sample whose path reaches the
    limit adds nothing.  (At depth 0 and 1 every sample takes one iteration and the frame's 512
    units fill the 8 waves, so all lanes end together and nothing is left to hand out: the next
    test has these depths with helpers.)"""
    sph, mats, osc, rend, cam = cover
    g, _ = check(rtw, oracle, rend, sph, mats, osc, cam, f"max_depth {depth}", helped=True if depth == 50 else None,
                 width=16, height=16, spp=40, max_depth=depth)
    if depth == 0:
        assert (g == 0).all()


@pytest.mark.parametrize("depth", [1, 2])
def test_depth_limits_with_helpers(rtw, oracle, cover, depth):
    """The same on padded tiles: waves with lanes free from the first take on, so samples whose
    path ends at the depth limit are traced by helpers and the owner's sum takes their + 0.0."""
    sph, mats, osc, rend, cam = cover
    check(rtw, oracle, rend, sph, mats, osc, cam, f"9x9 max_depth {depth}", width=9, height=9, spp=40, chunk=7,
          max_depth=depth)


@pytest.fixture(scope="module")
def movers(rtw, oracle):
    from rtw_amd.device import TorchRenderer
    sph, mats = scattered(rtw), materials(rtw)
    cam = rtw.camera_init((13, 2, 3), (0, 0.3, 0), (0, 1, 0), 30.0, 1.0, 0.1, 10.0, 0.0, 1.0)
    return sph, mats, to_oracle_scene(oracle, sph, mats), TorchRenderer(sph, mats, 0), cam


def test_movers_glass_and_mirrors(rtw, oracle, movers):
    """Long (glass, mirror) and short units in one wave; a helper traces the owner's pixel with
    the sample's own time."""
    sph, mats, osc, rend, cam = movers
    g, _ = check(rtw, oracle, rend, sph, mats, osc, cam, "scattered 24x24", width=24, height=24, spp=40)
    assert g.std() > 2


def test_wavefront_engine_gives_the_same_bytes(rtw, cover, movers):
    """Every byte of rgb and every float of the linear mean."""
    for sph, mats, _, _, cam in (cover, movers):
        kw = dict(width=24, height=24, spp=40)
        a = rtw.render(cam, sph, mats, rtw.make_params(**kw), want_mean=True)
        b = rtw.render(cam, sph, mats, rtw.make_params(engine="wavefront", wf_paths=4096, **kw), want_mean=True)
        assert np.array_equal(a[0], b[0])
        assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def test_accumulator_passes(rtw, cover):
    """Two unmasked passes of 20 run the frame kernel, tail included: the running sum is the
    one-shot frame's (its f32 mean and bytes).  A masked second pass, through the untouched masked
    kernel, gives the masked pixels the same sums and leaves the others at the first pass's."""
    import torch
    from rtw_amd.device import TorchAccumulator
    sph, mats, _, rend, cam = cover
    kw = dict(width=16, height=16)
    p = rtw.make_params(spp=40, **kw)
    rgb, mean = rtw.render(cam, sph, mats, p, want_mean=True)
    a = TorchAccumulator(rend.scene, p)
    a.render_pass(cam, 20)
    torch.cuda.synchronize()
    s1, _ = a.read()
    a.render_pass(cam, 20)
    torch.cuda.synchronize()
    s2, _ = a.read()
    assert np.array_equal(a.rgb.cpu().numpy(), rgb)
    assert np.array_equal(np.float32(s2 * (1.0 / 40)).view(np.uint32), mean.view(np.uint32))
    assert np.array_equal(a.mean.cpu().numpy().view(np.uint32), mean.view(np.uint32))
    a.close()
    mask = np.zeros((16, 16), np.uint8)
    mask[3:11, 2:13:2] = 1
    b = TorchAccumulator(rend.scene, p)
    b.render_pass(cam, 20)
    b.set_mask(mask)
    b.render_pass(cam, 20)
    torch.cuda.synchronize()
    sb, _ = b.read()
    b.close()
    assert np.array_equal(sb[mask != 0], s2[mask != 0])
    assert np.array_equal(sb[mask == 0], s1[mask == 0])


@pytest.mark.parametrize("which", ["cover", "movers"])
def test_f64_sums_are_the_masked_kernels(rtw, cover, movers, which):
    """The f64 chunk sums themselves, which pixels and the f32 mean round away: a 40-sample pass
    with the dealing against the same pass through the masked kernel (the rotated loop, a lane
    keeps its unit), on all pixels but one.  The order in which an owner adds its helpers'
    samples shows here and nowhere in an 8-bit image."""
    import torch
    from rtw_amd.device import TorchAccumulator
    _, _, _, rend, cam = cover if which == "cover" else movers
    p = rtw.make_params(width=24, height=24, spp=40, chunk=40)
    a = TorchAccumulator(rend.scene, p)
    a.render_pass(cam, 40)
    torch.cuda.synchronize()
    sa, _ = a.read()
    a.close()
    mask = np.ones((24, 24), np.uint8)
    mask[0, 0] = 0
    b = TorchAccumulator(rend.scene, p)
    b.set_mask(mask)
    b.render_pass(cam, 40)
    torch.cuda.synchronize()
    sb, _ = b.read()
    b.close()
    assert (sa[mask != 0] > 0).any()
    assert np.array_equal(sb[mask != 0], sa[mask != 0])


def test_two_streams_with_their_own_workspaces(rtw, cover):
    import torch
    from rtw_amd.device import TorchRenderer
    sph, mats, _, rend, cam = cover
    p = rtw.make_params(width=24, height=24, spp=40)
    want = rend.render(cam, p).cpu().numpy()
    other = TorchRenderer(sph, mats, 0)  # (its own scene tables and workspace)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        g1 = rend.render(cam, p)
    with torch.cuda.stream(s2):
        g2 = other.render(cam, p)
    torch.cuda.synchronize()
    assert np.array_equal(g1.cpu().numpy(), want) and np.array_equal(g2.cpu().numpy(), want)


def test_large_tables_keep_the_loop_without_the_tail(rtw, oracle):
    """200 more materials (64 B each in f64, staged whether used or not) put the scene tables
    between the LDS a workgroup may use at four workgroups per CU (40 KB of 160 KB) with the tail
    blocks (7 KB) and without them: the launch keeps its workgroups and the primary-first loop,
    and deals nothing."""
    from rtw_amd.device import TorchRenderer
    sph, mats0, _ = rtw.cover_scene(42)
    mats = (rtw.Material * (len(mats0) + 200))()
    for i, m in enumerate(mats0):
        mats[i] = m
    for i in range(len(mats0), len(mats)):
        mats[i].kind = rtw.LAMBERT_SOLID
        mats[i].albedo[:] = (0.5, 0.5, 0.5)
    osc = to_oracle_scene(oracle, sph, mats)
    _, st = check(rtw, oracle, TorchRenderer(sph, mats, 0), sph, mats, osc, rtw.cover_camera(1.0), "large tables",
                  helped=False, width=16, height=16, spp=40)
    assert st["primary_rounds"] > 0, st
