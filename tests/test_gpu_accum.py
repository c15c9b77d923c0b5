"""Progressive rendering on the GPU (rtw_accum_*): a frame
accumulated over chunk-aligned sample passes is the one-shot frame, byte for
byte — after every pass, for both precisions, both engines, an odd chunk and a
row shard; the running sum and the luminance statistic are the sequential f64
folds of the chunk sums; a saved state resumes; the noise estimate is the
formula of rtw_hip.h, deterministic; refused calls change nothing.

The cover scene at 60x33: neither side is a multiple of the 8x8 tile, so the
unit queue holds padding units."""
import numpy as np
import pytest

from helpers import to_oracle_camera, to_oracle_scene
from test_gpu_parity import assert_parity

pytestmark = pytest.mark.gpu

ASPECT = 16 / 9
W, H = 60, 33


@pytest.fixture(scope="module")
def cover(rtw):
    import torch
    from rtw_amd.device import TorchRenderer
    sph, mats, _ = rtw.cover_scene(42)
    cam = rtw.cover_camera(ASPECT)
    torch.cuda.set_device(0)
    return sph, mats, cam, TorchRenderer(sph, mats, 0).scene


def one_shot(rtw, cover, n, **kw):
    """rtw.render of the same params with spp = n: (rgb, mean)."""
    sph, mats, cam, _ = cover
    return rtw.render(cam, sph, mats, rtw.make_params(spp=n, **kw), want_mean=True)


def run_pass(ta, cam, n):
    """One pass + resolve through rtw_amd.device.TorchAccumulator -> (rgb, mean) on the host."""
    import torch
    ta.render_pass(cam, n)
    torch.cuda.synchronize()
    return ta.rgb.cpu().numpy(), ta.mean.cpu().numpy()


def same_image(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


BASE = dict(width=W, height=H)
CASES = [
    ("f64-megakernel", dict(precision="f64", engine="megakernel"), [20, 20, 10]),
    ("f32-megakernel", dict(precision="f32", engine="megakernel"), [20, 20, 10]),
    ("f64-wavefront", dict(precision="f64", engine="wavefront", wf_paths=4096), [20, 20, 10]),
    ("f32-wavefront", dict(precision="f32", engine="wavefront", wf_paths=4096), [20, 20, 10]),
    ("chunk7-f64-megakernel", dict(chunk=7), [14, 7, 21, 8]),
    ("chunk7-f32-wavefront", dict(chunk=7, precision="f32", engine="wavefront", wf_paths=4096), [14, 7, 21, 8]),
    ("shard-f64-megakernel", dict(row_begin=1, row_stride=3), [20, 20, 10]),
    ("shard-f64-wavefront", dict(row_begin=1, row_stride=3, engine="wavefront", wf_paths=4096), [20, 20, 10]),
]


@pytest.mark.parametrize("name,kw,passes", CASES, ids=[c[0] for c in CASES])
def test_passes_equal_the_one_shot_render(rtw, oracle, cover, name, kw, passes):
    from rtw_amd.device import TorchAccumulator
    sph, mats, cam, scene = cover
    kw = dict(BASE, **kw)
    assert sum(passes) == 50
    ta = TorchAccumulator(scene, rtw.make_params(spp=50, **kw))
    done = 0
    for n in passes:
        got = run_pass(ta, cam, n)
        done += n
        assert ta.samples() == done
        want = one_shot(rtw, cover, done, **kw)
        assert same_image(got, want), (name, done, int((got[0] != want[0]).sum()))
    ta.close()
    okw = {k: v for k, v in kw.items() if k in ("chunk", "row_begin", "row_stride")}
    o, _ = oracle.render_tier_b(to_oracle_scene(oracle, sph, mats), to_oracle_camera(oracle, cam), W, H, 50,
                                precision=1 if kw.get("precision") == "f32" else 0, **okw)
    assert_parity(got[0], o, f"accumulated {name}")


def test_passes_iterator_yields_every_pass(rtw, cover):
    """The torch-side helper: the image tensor after each pass, the last pass shortened to the frame."""
    import torch
    from rtw_amd.device import TorchAccumulator
    _, _, cam, scene = cover
    ta = TorchAccumulator(scene, rtw.make_params(spp=50, **BASE))
    seen = []
    for img in ta.passes(cam, 20):
        torch.cuda.synchronize()
        seen.append((ta.samples(), img.cpu().numpy()))
    assert [s for s, _ in seen] == [20, 40, 50]
    assert np.array_equal(seen[-1][1], one_shot(rtw, cover, 50, **BASE)[0])
    ta.close()


def luminance(c):
    return (0.2126 * c[..., 0] + 0.7152 * c[..., 1]) + 0.0722 * c[..., 2]


def test_sum_and_stat_are_the_sequential_folds_of_the_chunk_sums(rtw, cover):
    from rtw_amd.device import TorchAccumulator
    _, _, cam, scene = cover
    kw = dict(width=16, height=9)
    p = rtw.make_params(spp=45, **kw)
    zeros3, zeros2 = np.zeros((9, 16, 3)), np.zeros((9, 16, 2))
    chunks = []
    for k, n in enumerate([20, 20, 5]):  # chunk k alone: a fresh accumulator started at sample 20 k
        ta = TorchAccumulator(scene, p)
        ta.acc.load(zeros3, zeros2, 20 * k)
        run_pass(ta, cam, n)
        c, _ = ta.acc.read()
        chunks.append(c)
        ta.close()
    ta = TorchAccumulator(scene, p)
    for n in [20, 20, 5]:
        got = run_pass(ta, cam, n)
    s, st = ta.acc.read()
    ta.close()
    fold = np.zeros((9, 16, 3))
    y1, y2 = np.zeros((9, 16)), np.zeros((9, 16))
    for k, c in enumerate(chunks):
        fold = fold + c
        if k < 2:  # the 5-sample chunk is in the sum only
            y = luminance(c)
            y1 = y1 + y
            y2 = y2 + y * y
    assert np.array_equal(s, fold)
    assert np.array_equal(st[..., 0], y1) and np.array_equal(st[..., 1], y2)
    assert (y1 > 0).all()
    rgb, mean = one_shot(rtw, cover, 45, **kw)
    assert np.array_equal(np.float32(s * (1.0 / 45)).view(np.uint32), mean.view(np.uint32))
    assert same_image(got, (rgb, mean))


def test_saved_state_resumes(rtw, cover):
    from rtw_amd.device import TorchAccumulator
    _, _, cam, scene = cover
    p = rtw.make_params(spp=50, **BASE)
    a = TorchAccumulator(scene, p)
    run_pass(a, cam, 20)
    run_pass(a, cam, 20)
    s, st = a.acc.read()
    b = TorchAccumulator(scene, p)
    b.acc.load(s, st, 40)
    assert b.samples() == 40
    resumed = run_pass(b, cam, 10)
    straight = run_pass(a, cam, 10)
    assert same_image(resumed, straight)
    assert same_image(resumed, one_shot(rtw, cover, 50, **BASE))
    sa, sta = a.acc.read()
    sb, stb = b.acc.read()
    assert np.array_equal(sa, sb) and np.array_equal(sta, stb)
    a.close()
    b.close()


def test_noise_is_the_formula_and_deterministic(rtw, cover):
    from rtw_amd.device import TorchAccumulator
    _, _, cam, scene = cover
    ta = TorchAccumulator(scene, rtw.make_params(32, 18, 80))
    run_pass(ta, cam, 20)
    with pytest.raises(rtw.RtwError) as e:  # one full chunk: no spread to estimate from
        ta.noise()
    assert e.value.status == rtw.RTW_EINVAL
    for _ in range(3):
        run_pass(ta, cam, 20)
    _, st = ta.acc.read()
    m, nc, npix = 4, 20, 32 * 18
    y1, y2 = st[..., 0].ravel(), st[..., 1].ravel()
    se2 = np.maximum(0.0, y2 - y1 * y1 / m) / (m * (m - 1) * nc * nc)
    want = np.sqrt(se2.sum() / npix)
    a, b = ta.noise(), ta.noise()
    print("noise", a, "numpy", want, "rel", abs(a - want) / want)
    assert want > 0
    assert abs(a - want) <= (npix + 8) * 2.0 ** -52 * want
    assert np.float64(a).view(np.uint64) == np.float64(b).view(np.uint64)
    ta.close()


def test_refused_calls_leave_the_accumulator_unchanged(rtw, cover):
    from rtw_amd.device import TorchAccumulator
    _, _, cam, scene = cover
    ta = TorchAccumulator(scene, rtw.make_params(spp=50, **BASE))
    run_pass(ta, cam, 20)
    before = ta.acc.read()

    def refused(f, *a):
        with pytest.raises(rtw.RtwError) as e:
            f(*a)
        assert e.value.status == rtw.RTW_EINVAL
        assert rtw.lib().rtw_last_error()
        after = ta.acc.read()
        assert ta.samples() == 20 and np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1])

    refused(run_pass, ta, cam, 13)   # off the chunk grid and not the frame's end
    refused(run_pass, ta, cam, 40)   # beyond spp
    refused(run_pass, ta, cam, 0)
    refused(ta.acc.load, before[0], before[1], 13)
    refused(ta.acc.load, before[0], before[1], 60)
    run_pass(ta, cam, 20)
    got = run_pass(ta, cam, 10)
    assert same_image(got, one_shot(rtw, cover, 50, **BASE))
    with pytest.raises(rtw.RtwError):  # the frame is complete
        run_pass(ta, cam, 20)
    ta.close()


def _read_ppm(path):
    data = open(path, "rb").read()
    parts = data.split(b"\n", 3)
    w, h = map(int, parts[1].split())
    return np.frombuffer(parts[3], np.uint8).reshape(h, w, 3)


def test_cli_pass_spp_writes_the_same_image(rtw, tmp_path):
    """bin/rtw_render --pass-spp: the same --out bytes as the one-shot run, a
    preview per pass, the last preview = --out."""
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(rtw.__file__), "..", "bin", "rtw_render")
    one, prog, prev = tmp_path / "one.ppm", tmp_path / "prog.ppm", tmp_path / "previews"
    base = [exe, "--scene", "1", "--width", "64", "--spp", "40"]
    for args in (base + ["--out", str(one)],
                 base + ["--out", str(prog), "--pass-spp", "20", "--preview-dir", str(prev)]):
        r = subprocess.run(args, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
    assert one.read_bytes() == prog.read_bytes()
    assert sorted(os.listdir(prev)) == ["pass_0001.ppm", "pass_0002.ppm"]
    assert (prev / "pass_0002.ppm").read_bytes() == prog.read_bytes()
    assert (prev / "pass_0001.ppm").read_bytes() != prog.read_bytes()
    assert _read_ppm(str(prog)).shape[1] == 64
    # a noise budget every frame meets: the 80-sample frame stops as soon as there is an estimate
    # (two full chunks), with the 40-sample frame's bytes
    early = tmp_path / "early.ppm"
    r = subprocess.run([exe, "--scene", "1", "--width", "64", "--spp", "80", "--out", str(early), "--pass-spp", "20",
                        "--max-noise", "1000"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "40 of 80 samples used" in r.stderr, r.stderr
    assert early.read_bytes() == one.read_bytes()
    # a general world (the Cornell box) through the same options
    cone, cprog = tmp_path / "cornell_one.ppm", tmp_path / "cornell_prog.ppm"
    cbase = [exe, "--scene", "6", "--width", "40", "--spp", "40"]
    for args in (cbase + ["--out", str(cone)], cbase + ["--out", str(cprog), "--pass-spp", "20"]):
        r = subprocess.run(args, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
    assert cone.read_bytes() == cprog.read_bytes()


# ------------------------------------------------- quantisation edges ----
QW, QH = 31, 29  # 899 pixels: room for the ~2,600 values of one n, and no multiple of the 8x8 tile


def _quantize_values(q, n):
    """Sums whose quantisation sits on an edge, for a frame of n samples.  For
    every k in 1..255: n (k/256)^2 and its two neighbours on each side; and,
    found by bisection with the oracle's ro_quantize, the SMALLEST double that
    quantises to k with its two neighbours on each side — that group holds both
    outputs k - 1 and k by construction (the first group alone does so for
    most (n, k) only: 1/n is inexact, and t (1/n) can land a few ulps off).
    Then 0, -0.0, a subnormal, a negative sum, the neighbours of n 0.999^2,
    1e300, +inf and NaN.  Returns (values, number of first groups that straddle)."""
    scale = 1.0 / n
    vals, straddle = [], 0

    def around(t):
        g, lo, hi = [t], t, t
        for _ in range(2):
            lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
            g = [lo] + g + [hi]
        return [float(x) for x in g]

    for k in range(1, 256):
        t = float(np.float64(n) * (np.float64(k) / 256) ** 2)
        g = around(t)
        straddle += {k - 1, k} <= {q(x, scale) for x in g}
        lo, hi = np.float64(t * (1 - 1e-9)).view(np.int64), np.float64(t * (1 + 1e-9)).view(np.int64)
        assert q(float(lo.view(np.float64)), scale) == k - 1 and q(float(hi.view(np.float64)), scale) == k
        while hi - lo > 1:  # monotone in the bit pattern
            mid = np.int64((int(lo) + int(hi)) // 2)
            if q(float(mid.view(np.float64)), scale) >= k:
                hi = mid
            else:
                lo = mid
        edge = around(float(hi.view(np.float64)))
        assert [q(x, scale) for x in edge] == [k - 1, k - 1, k, k, k], (n, k)
        vals += g + edge
    top = float(np.float64(n) * np.float64(0.999) ** 2)
    vals += around(top) + [0.0, -0.0, 5e-324, 1e-310, -1e-310, -0.25 * n, -1e300, 1e300, float("inf"), float("nan"),
                           0.25 * n, float(n), 2.0 * n]
    return vals, straddle


@pytest.mark.parametrize("n", [1, 3, 7, 45, 500])
def test_resolve_quantisation_edges(rtw, oracle, cover, n):
    """accum_resolve_kernel's sqrt, clamp to 0.999, (uint8_t)(256 cl) and NaN ->
    255 on sums a test chooses (rtw_accum_load, then the resolve), value by
    value against ro_quantize(t, 1.0 / n), and the f32 mean against
    np.float32(t * (1.0 / n)) bit for bit (two NaNs are equal).  rtw_accum_load
    takes non-finite sums as they are: a saved state may hold them."""
    import torch
    from rtw_amd.device import TorchAccumulator
    _, _, _, scene = cover
    q = oracle.lib().ro_quantize
    vals, straddle = _quantize_values(q, n)
    print("n", n, "values", len(vals), "first groups holding both k - 1 and k:", straddle, "of 255")
    flat = np.full(QW * QH * 3, 0.5 * n)
    assert len(vals) <= flat.size
    flat[:len(vals)] = vals
    ta = TorchAccumulator(scene, rtw.make_params(QW, QH, n))
    try:
        ta.acc.load(flat.reshape(QH, QW, 3), np.zeros((QH, QW, 2)), n)
        assert ta.samples() == n
        ta.acc.resolve(ta.rgb.data_ptr(), ta.mean.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        rgb, mean = ta.rgb.cpu().numpy().ravel(), ta.mean.cpu().numpy().ravel()
        back, _ = ta.acc.read()
    finally:
        ta.close()
    assert np.array_equal(back.ravel().view(np.uint64), flat.view(np.uint64))  # loaded as given, NaN and -0.0 included
    scale = 1.0 / n
    want = np.array([q(float(t), scale) for t in flat], np.uint8)
    wrong = np.flatnonzero(rgb != want)
    assert wrong.size == 0, [(float.hex(float(flat[i])), int(rgb[i]), int(want[i])) for i in wrong[:8]]
    with np.errstate(over="ignore", invalid="ignore"):
        wmean = (flat * scale).astype(np.float32)
    same = (mean.view(np.uint32) == wmean.view(np.uint32)) | (np.isnan(mean) & np.isnan(wmean))
    assert same.all(), [(float.hex(float(flat[i])), float(mean[i]), float(wmean[i])) for i in np.flatnonzero(~same)[:8]]
    # what the rules give at the ends (oracle/rtw_oracle.c ro_quantize, tests/test_oracle_kat.py)
    at = {float.hex(v) if v == v else "nan": int(rgb[i]) for i, v in enumerate(vals)}
    assert at[float.hex(0.0)] == 0 and at[float.hex(-0.0)] == 0 and at[float.hex(5e-324)] == 0
    assert at["nan"] == 255 and at[float.hex(float("inf"))] == 255 and at[float.hex(1e300)] == 255
    assert at[float.hex(-0.25 * n)] == 255  # sqrt of a negative sum is NaN, and @min(NaN, 0.999) = 0.999
    assert at[float.hex(0.25 * n)] == 128 and at[float.hex(float(n))] == 255
