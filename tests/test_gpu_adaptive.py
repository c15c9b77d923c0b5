"""Adaptive sampling on the GPU: masked passes and the
per-pixel noise budget keep the bit-exact contract per pixel — a pixel that
holds n samples has the one-shot render's bytes with spp = n there, for both
precisions and engines, an odd chunk and a row shard; an inactive pixel's state
is never touched and its workspace values never read; the active set is the
criterion of rtw_hip.h evaluated after every fold; a saved state resumes.

The cover scene at 60x33: 7.5 x 4.125 tiles of 8x8, 40 tiles, padded on both
edges."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ASPECT = 16 / 9
W, H = 60, 33
BASE = dict(width=W, height=H)


@pytest.fixture(scope="module")
def cover(rtw):
    import torch
    from rtw_amd.device import TorchRenderer
    sph, mats, _ = rtw.cover_scene(42)
    cam = rtw.cover_camera(ASPECT)
    torch.cuda.set_device(0)
    return sph, mats, cam, TorchRenderer(sph, mats, 0).scene


@pytest.fixture(scope="module")
def one_shot(rtw, cover):
    """rtw.render of the params with spp = n -> (rgb, mean); each rendered once for the module."""
    sph, mats, cam, _ = cover
    cache = {}

    def f(n, **kw):
        key = (n, tuple(sorted(kw.items())))
        if key not in cache:
            cache[key] = rtw.render(cam, sph, mats, rtw.make_params(spp=n, **kw), want_mean=True)
        return cache[key]
    return f


def run_pass(ta, cam, n, poison=False):
    """One pass + resolve -> (rgb, mean) on the host; poison: the workspace filled with NaN first."""
    import torch
    if poison:
        ta.workspace(n).fill_(0xFF)  # (every f64 / f32 word a NaN)
    ta.render_pass(cam, n)
    torch.cuda.synchronize()
    return ta.rgb.cpu().numpy(), ta.mean.cpu().numpy()


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_pixels_equal_their_one_shot(one_shot, got, counts, kw, what):
    """For every distinct count n: rgb and the mean's bits at the pixels with that count = the one-shot's with spp = n."""
    rgb, mean = got
    for n in np.unique(counts):
        sel = counts == n
        if n == 0:
            assert not rgb[sel].any() and not mean[sel].any(), what
            continue
        want = one_shot(int(n), **kw)
        assert np.array_equal(rgb[sel], want[0][sel]), (what, int(n), int((rgb[sel] != want[0][sel]).sum()))
        assert np.array_equal(u32(mean)[sel], u32(want[1])[sel]), (what, int(n))


def tile_masks(rows):
    """(checkerboard of pixels, of the parity that keeps the last pixel; every other 8x8 tile off and the
    corner edge tile cut to its last pixel).  Inactive is sticky, so the last pixel has to survive the
    checkerboard to be the corner tile's one live pixel in the passes after the second mask."""
    y, x = np.mgrid[0:rows, 0:W]
    checker = (x + y) % 2 == (W - 1 + rows - 1) % 2
    tx, ty = x // 8, y // 8
    ctx, cty = (W - 1) // 8, (rows - 1) // 8
    tiles = (tx + ty) % 2 == (ctx + cty) % 2  # (keeps the corner tile)
    corner = (tx == ctx) & (ty == cty)
    tiles &= ~corner | ((x == W - 1) & (y == rows - 1))
    return checker, tiles


WF = dict(engine="wavefront", wf_paths=4096)
MASK_CASES = [
    ("f64-megakernel", dict(precision="f64"), [20, 20, 20, 10]),
    ("f32-megakernel", dict(precision="f32"), [20, 20, 20, 10]),
    ("f64-wavefront", dict(precision="f64", **WF), [20, 20, 20, 10]),
    ("f32-wavefront", dict(precision="f32", **WF), [20, 20, 20, 10]),
    ("chunk7-f64-megakernel", dict(chunk=7), [14, 7, 21, 8]),
    ("shard-f64-megakernel", dict(row_begin=1, row_stride=3), [20, 20, 20, 10]),
]


@pytest.mark.parametrize("name,kw,passes", MASK_CASES, ids=[c[0] for c in MASK_CASES])
def test_masked_passes_equal_the_one_shot_render_per_pixel(rtw, cover, one_shot, name, kw, passes):
    from rtw_amd.device import TorchAccumulator
    _, _, cam, scene = cover
    kw = dict(BASE, **kw)
    p = rtw.make_params(spp=sum(passes), **kw)
    rows = p.row_count
    if "row_stride" not in kw:
        assert rows == 33 and (W - 1, rows - 1) == (59, 32)
    checker, tiles = tile_masks(rows)
    assert tiles[rows - 1, W - 1] and tiles[(rows - 1) // 8 * 8:, (W - 1) // 8 * 8:].sum() == 1
    corner = (slice((rows - 1) // 8 * 8, None), slice((W - 1) // 8 * 8, None))  # the padded corner edge tile
    ta = TorchAccumulator(scene, p)
    active = np.ones((rows, W), bool)
    want_cnt = np.zeros((rows, W), np.uint32)
    done = 0
    for k, n in enumerate(passes):
        if k == 1:
            ta.set_mask(checker)
            active &= checker
        if k == 2:
            ta.set_mask(tiles.astype(np.uint8) * 7)  # (any non-zero byte keeps a pixel)
            active &= tiles
            # the case the masks are for: an edge tile dealt with ONE live bit, at lane 8 * (row % 8) + column % 8
            assert active[rows - 1, W - 1] and active[corner].sum() == 1
        if k >= 1:
            n_tiles = len({(y // 8, x // 8) for y, x in zip(*np.nonzero(active))})
            assert ta.active() == (int(active.sum()), n_tiles), (name, k)
        before = ta.read() if k else None
        got = run_pass(ta, cam, n, poison=k >= 1)
        done += n
        want_cnt[active] += n
        assert ta.samples() == done
        cnt = ta.counts()
        assert np.array_equal(cnt, want_cnt), (name, k)
        s, st = ta.read()
        assert not np.isnan(s).any() and not np.isnan(st).any() and not np.isnan(got[1]).any(), (name, k)
        if before is not None:
            assert np.array_equal(s[~active], before[0][~active]) and np.array_equal(st[~active], before[1][~active])
            assert not np.array_equal(s[active], before[0][active])
        assert_pixels_equal_their_one_shot(one_shot, got, cnt, kw, (name, k))
    assert len(np.unique(want_cnt)) == 3
    assert cnt[rows - 1, W - 1] == sum(passes) and (cnt[corner] == sum(passes)).sum() == 1  # the corner pixel ran on alone
    ta.close()


def test_a_pass_with_no_active_pixel_changes_nothing(rtw, cover):
    from rtw_amd.device import TorchAccumulator
    _, _, cam, scene = cover
    ta = TorchAccumulator(scene, rtw.make_params(spp=60, **BASE))
    run_pass(ta, cam, 20)
    ta.set_mask(np.zeros((H, W), np.uint8))
    assert ta.active() == (0, 0)
    before = ta.read(), ta.counts(), ta.rgb.cpu().numpy(), ta.mean.cpu().numpy()
    rgb, mean = run_pass(ta, cam, 20, poison=True)
    assert ta.samples() == 20 and ta.active() == (0, 0)
    s, st = ta.read()
    assert np.array_equal(s, before[0][0]) and np.array_equal(st, before[0][1])
    assert np.array_equal(ta.counts(), before[1]) and (before[1] == 20).all()
    assert np.array_equal(rgb, before[2]) and np.array_equal(u32(mean), u32(before[3]))
    ta.close()


def luminance_se2(stat, cnt, chunk):
    """se2 of rtw_hip.h per pixel (numpy f64, the header's operation order); 0 where m < 2."""
    m = (cnt // chunk).astype(np.float64)
    ok = m >= 2
    ms = np.where(ok, m, 2.0)
    sy, sy2 = stat[..., 0], stat[..., 1]
    var = np.maximum(0.0, sy2 - sy * sy / ms)
    return np.where(ok, var / (ms * (ms - 1.0) * np.float64(chunk) * np.float64(chunk)), 0.0), ok


def adaptive_run(rtw, cover, one_shot, kw, spp, tol, min_spp, pass_spp=20, chunk=20, stop_after=None):
    """Drives adaptive passes, checking the library's active set against the criterion in numpy after every
    pass.  Returns (ta, per-pass active() list, final (rgb, mean))."""
    from rtw_amd.device import TorchAccumulator
    _, _, cam, scene = cover
    kw = dict(BASE, **kw)
    ta = TorchAccumulator(scene, rtw.make_params(spp=spp, **kw))
    ta.set_adaptive(tol, min_spp)
    assert ta.active() == (W * H, 40)
    active = np.ones((H, W), bool)
    want_cnt = np.zeros((H, W), np.uint32)
    seen, got, k = [], None, 0
    while ta.samples() < spp and (stop_after is None or k < stop_after):
        done = ta.samples()
        got = run_pass(ta, cam, pass_spp)
        k += 1
        if not active.any():  # the pass was a no-op
            assert ta.samples() == done
            seen.append(ta.active())
            break
        want_cnt[active] += pass_spp
        cnt = ta.counts()
        assert np.array_equal(cnt, want_cnt), k  # the pass covered exactly the pixels numpy found active
        _, st = ta.read()
        se2, ok = luminance_se2(st, cnt, chunk)
        active &= ~(ok & (cnt >= min_spp) & (se2 <= np.float64(tol) * np.float64(tol)))
        n_tiles = len({(y // 8, x // 8) for y, x in zip(*np.nonzero(active))})
        assert ta.active() == (int(active.sum()), n_tiles), k
        seen.append(ta.active())
    return ta, seen, got


ADAPT_CASES = [("f64-megakernel", dict(), 100), ("f32-megakernel", dict(precision="f32"), 50),
               ("f64-wavefront", dict(WF), 50)]


@pytest.mark.parametrize("name,kw,floor", ADAPT_CASES, ids=[c[0] for c in ADAPT_CASES])
def test_adaptive_budget_follows_the_criterion(rtw, cover, one_shot, name, kw, floor):
    """tol 0.02, chunk 20, spp 100, passes of 20.  Tier B on the CPU gives the f64 classes 40 / 60 / 80 / 100 =
    1163 / 154 / 121 / 542 pixels and 36 active tiles after the second pass; the floors keep a frame where
    nothing adapted from passing."""
    ta, seen, got = adaptive_run(rtw, cover, one_shot, kw, 100, 0.02, 0)
    cnt = ta.counts()
    classes = {n: int((cnt == n).sum()) for n in (40, 60, 80, 100)}
    print(name, "classes", classes, "active per pass", seen)
    assert sum(classes.values()) == W * H
    assert all(v >= floor for v in classes.values()), classes
    assert seen[1][1] < 40, seen
    assert_pixels_equal_their_one_shot(one_shot, got, cnt, dict(BASE, **kw), name)
    ta.close()


def test_budget_met_makes_the_next_pass_a_no_op(rtw, cover, one_shot):
    """tol 0.05, spp 120: on the CPU every pixel has converged after the fifth pass."""
    ta, seen, got = adaptive_run(rtw, cover, one_shot, {}, 120, 0.05, 0)
    print("active per pass", seen)
    assert len(seen) == 6 and seen[4] == (0, 0) and seen[5] == (0, 0)  # (the sixth pass ran, and did nothing)
    assert ta.active()[0] == 0 and ta.samples() == 100
    cnt = ta.counts()
    assert cnt.max() <= 100
    assert_pixels_equal_their_one_shot(one_shot, got, cnt, BASE, "budget met")
    ta.close()


def test_min_spp_is_a_floor(rtw, cover, one_shot):
    ta, seen, got = adaptive_run(rtw, cover, one_shot, {}, 100, 0.02, 60)
    cnt = ta.counts()
    print("classes", {int(n): int((cnt == n).sum()) for n in np.unique(cnt)})
    assert cnt.min() >= 60 and (cnt == 60).sum() >= 100
    assert set(np.unique(cnt)) == {60, 80, 100}
    assert_pixels_equal_their_one_shot(one_shot, got, cnt, BASE, "min_spp")
    ta.close()


def test_saved_state_with_counts_resumes(rtw, cover, one_shot):
    from rtw_amd.device import TorchAccumulator
    _, _, cam, scene = cover
    a, _, _ = adaptive_run(rtw, cover, one_shot, {}, 100, 0.02, 0, stop_after=3)
    assert a.samples() == 60
    s, st = a.read()
    cnt = a.counts()
    assert len(np.unique(cnt)) == 2
    p = rtw.make_params(spp=100, **BASE)
    b = TorchAccumulator(scene, p)
    b.set_adaptive(0.02, 0)
    b.load(s, st, 60, counts=cnt)
    assert b.samples() == 60 and b.active() == a.active()
    assert np.array_equal(b.counts(), cnt)
    for _ in range(2):
        ga, gb = run_pass(a, cam, 20), run_pass(b, cam, 20)
        assert np.array_equal(ga[0], gb[0]) and np.array_equal(u32(ga[1]), u32(gb[1]))
        assert np.array_equal(a.counts(), b.counts())
    (sa, sta), (sb, stb) = a.read(), b.read()
    assert np.array_equal(sa, sb) and np.array_equal(sta, stb)
    assert len(np.unique(b.counts())) == 4

    def refused(c, done):
        before = b.read(), b.counts(), b.samples(), b.active()
        with pytest.raises(rtw.RtwError) as e:
            b.load(s, st, done, counts=c)
        assert e.value.status == rtw.RTW_EINVAL
        after = b.read(), b.counts(), b.samples(), b.active()
        assert np.array_equal(before[0][0], after[0][0]) and np.array_equal(before[0][1], after[0][1])
        assert np.array_equal(before[1], after[1]) and before[2:] == after[2:]

    bad = cnt.copy()
    bad[3, 5] = 80  # above samples_done
    refused(bad, 60)
    bad = cnt.copy()
    bad[3, 5] = 30  # off the chunk grid
    refused(bad, 60)
    refused(cnt, 50)  # samples_done itself off the grid
    a.close()
    b.close()


def test_noise_unmasked_keeps_its_bits_and_masked_uses_each_pixels_m(rtw, cover):
    from rtw_amd.device import TorchAccumulator
    _, _, cam, scene = cover
    p = rtw.make_params(spp=80, **BASE)
    plain, same = TorchAccumulator(scene, p), TorchAccumulator(scene, p)
    for _ in range(3):
        run_pass(plain, cam, 20)  # none of the new calls
        run_pass(same, cam, 20)
        # the new entry points that must not put an accumulator in the masked state, between the passes
        assert same.active() == (W * H, 40) and (same.counts() == same.samples()).all()
        same.set_adaptive(0.0)
        with pytest.raises(rtw.RtwError):
            same.set_adaptive(-1.0)
    a, b = plain.noise(), same.noise()
    assert np.float64(a).view(np.uint64) == np.float64(b).view(np.uint64)
    (sa, sta), (sb, stb) = plain.read(), same.read()
    assert np.array_equal(sa, sb) and np.array_equal(sta, stb)
    # today's formula with the frame's m (tests/test_gpu_accum.py), which a never-masked accumulator keeps
    _, st = plain.read()
    npix = W * H
    se2, _ = luminance_se2(st, np.full((H, W), 60, np.uint32), 20)
    want = np.sqrt(se2.sum() / npix)
    assert abs(a - want) <= (npix + 8) * 2.0 ** -52 * want
    # masked: a checkerboard stops after 60 samples, the rest goes on to 80; rows 0-7 x columns 0-7 never pass m = 1
    m = TorchAccumulator(scene, p)
    run_pass(m, cam, 20)
    early = np.ones((H, W), bool)
    early[:8, :8] = False
    m.set_mask(early)
    run_pass(m, cam, 20)
    run_pass(m, cam, 20)
    y, x = np.mgrid[0:H, 0:W]
    m.set_mask((x + y) % 2 == 0)
    run_pass(m, cam, 20, poison=True)
    cnt = m.counts()
    assert set(np.unique(cnt)) == {20, 60, 80}
    _, st = m.read()
    se2, ok = luminance_se2(st, cnt, 20)
    assert ok.sum() == npix - 64
    want = np.sqrt(se2[ok].sum() / ok.sum())
    got = m.noise()
    print("masked noise", got, "numpy", want, "rel", abs(got - want) / want)
    assert want > 0 and abs(got - want) <= (npix + 8) * 2.0 ** -52 * want
    assert np.float64(got).view(np.uint64) == np.float64(m.noise()).view(np.uint64)
    # no pixel with two full chunks: refused
    z = TorchAccumulator(scene, p)
    z.set_mask(np.ones((H, W), np.uint8))
    run_pass(z, cam, 20)
    with pytest.raises(rtw.RtwError) as e:
        z.noise()
    assert e.value.status == rtw.RTW_EINVAL
    for t in (plain, same, m, z):
        t.close()


def test_bad_budgets_are_refused(rtw, cover):
    from rtw_amd.device import TorchAccumulator
    _, _, cam, scene = cover
    ta = TorchAccumulator(scene, rtw.make_params(spp=40, **BASE))
    run_pass(ta, cam, 20)
    for tol in (-0.01, float("nan"), float("inf")):
        with pytest.raises(rtw.RtwError) as e:
            ta.set_adaptive(tol)
        assert e.value.status == rtw.RTW_EINVAL
    assert ta.active() == (W * H, 40) and (ta.counts() == 20).all()
    ta.close()


def _read_pnm(path):
    data = open(path, "rb").read()
    magic, dims, maxval, body = data.split(b"\n", 3)
    w, h = map(int, dims.split())
    if magic == b"P6":
        return np.frombuffer(body, np.uint8).reshape(h, w, 3)
    assert magic == b"P5"
    return np.frombuffer(body, np.uint8 if int(maxval) < 256 else ">u2").reshape(h, w).astype(np.uint32)


def test_cli_pixel_noise_writes_the_library_paths_image_and_map(rtw, cover, tmp_path):
    """bin/rtw_render --pass-spp 20 --pixel-noise 0.02 --spp-map: the image and the count map of the same
    passes through the library."""
    import os
    import subprocess
    from rtw_amd.device import TorchAccumulator
    _, _, cam, scene = cover
    exe = os.path.join(os.path.dirname(rtw.__file__), "..", "bin", "rtw_render")
    out, spp_map = tmp_path / "adaptive.ppm", tmp_path / "spp.pgm"
    r = subprocess.run([exe, "--scene", "1", "--width", "64", "--aspect", "16:9", "--spp", "100", "--out", str(out),
                        "--pass-spp", "20", "--pixel-noise", "0.02", "--spp-map", str(spp_map)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    img, counts = _read_pnm(str(out)), _read_pnm(str(spp_map))
    h = img.shape[0]
    assert h == rtw.image_height(64, ASPECT)  # (the fixture's camera)
    ta = TorchAccumulator(scene, rtw.make_params(64, h, 100))
    ta.set_adaptive(0.02, 0)
    for rgb in ta.passes(cam, 20):
        pass
    import torch
    torch.cuda.synchronize()
    assert np.array_equal(counts, ta.counts())
    assert len(np.unique(counts)) >= 3
    assert np.array_equal(img, ta.rgb.cpu().numpy())
    ta.close()
