"""The denoiser on the GPU: rtw_denoise_device gives
rtw_denoise_host's bytes — the mean's u32 words and the rgb bytes — at every
size at which the kernels take another path, and the accumulator entry is
resolve + variance + filter without touching the accumulator."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def synthetic(rtw, w, h, seed):
    """An image with every kind of pixel: smooth regions with noise, zero, unknown
    and known variance, pixels without a sample, and guides with several
    primitives, slowly turning normals, depth steps, albedo steps and misses."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = 0.5 + 0.4 * np.sin(x / 7.0)[..., None] * np.cos(y / 5.0)[..., None] * np.array([1.0, 0.8, 0.6])
    mean = (base + rng.normal(0.0, 0.05, (h, w, 3))).clip(0.0, 4.0).astype(np.float32)
    var = rng.uniform(1e-4, 4e-3, (h, w)).astype(np.float32)
    kind = rng.integers(0, 10, (h, w))
    var[kind == 0] = 0.0
    var[kind == 1] = rtw.VAR_UNKNOWN
    empty = kind == 2
    var[empty] = rtw.VAR_EMPTY
    mean[empty] = 0.0
    g = np.zeros((h, w), rtw.GUIDE_DTYPE)
    prim = 1 + (x // 9 + 3 * (y // 7)) % 5
    miss = (x + 2 * y) % 23 < 4
    prim[miss] = 0
    ang = 0.02 * x + 0.03 * y + 0.7 * prim
    n = np.stack([np.cos(ang), np.sin(ang) * 0.6, np.sin(ang) * 0.8], axis=-1)
    g["normal"] = n
    g["depth"] = 2.0 + 0.01 * x + 0.5 * (prim % 3) + rng.uniform(0.0, 0.02, (h, w))
    g["albedo"] = (0.3 + 0.1 * (prim[..., None] % 4) + rng.uniform(0.0, 0.03, (h, w, 3)))
    g["prim"] = prim
    g["normal"][miss] = 0.0
    g["depth"][miss] = 0.0
    g["albedo"][miss] = (0.7, 0.8, 1.0)
    return mean, var, g


def run_device(rtw, mean, var, guides, opts):
    import torch
    h, w = mean.shape[:2]
    dev = "cuda:0"
    t_mean = torch.from_numpy(mean).to(dev)
    t_var = torch.from_numpy(var).to(dev) if var is not None else None
    t_g = torch.from_numpy(guides.view(np.uint8).reshape(h, w, 32)).to(dev) if guides is not None else None
    need = rtw.denoise_workspace_bytes(w, h, opts)
    ws = torch.full((need + 256,), 0xFF, dtype=torch.uint8, device=dev)
    ptr = (ws.data_ptr() + 255) & ~255
    rgb = torch.full((h, w, 3), 7, dtype=torch.uint8, device=dev)
    out = torch.full((h, w, 3), float("nan"), dtype=torch.float32, device=dev)
    rtw.denoise_device(t_mean.data_ptr(), t_var.data_ptr() if t_var is not None else None,
                       t_g.data_ptr() if t_g is not None else None, w, h, opts, ptr, need, rgb.data_ptr(),
                       out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(t_mean.cpu().numpy(), mean)  # the input is not modified
    return rgb.cpu().numpy(), out.cpu().numpy()


@pytest.mark.parametrize("levels", [1, 5, 6])
@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (60, 33), (150, 100)])
def test_device_equals_host_bit_for_bit(rtw, w, h, levels):
    mean, var, guides = synthetic(rtw, w, h, 1000 * w + levels)
    if w * h > 100:  # the generator made every kind of pixel
        assert (var == 0).any() and (var == rtw.VAR_UNKNOWN).any() and (var == rtw.VAR_EMPTY).any()
        assert (guides["prim"] == 0).any() and len(np.unique(guides["prim"])) >= 4
    for v, g in ((var, guides), (None, guides), (var, None), (None, None)):
        opts = rtw.denoise_opts(levels=levels)
        want = rtw.denoise_host(mean, v, g, opts)
        got = run_device(rtw, mean, v, g, opts)
        what = (w, h, levels, v is not None, g is not None)
        assert np.array_equal(u32(got[1]), u32(want[1])), (what, int((u32(got[1]) != u32(want[1])).sum()))
        assert np.array_equal(got[0], want[0]), what
        again = run_device(rtw, mean, v, g, opts)  # no state: the same bytes
        assert got[0].tobytes() == again[0].tobytes() and got[1].tobytes() == again[1].tobytes(), what
        # every level in the direct form (no LDS tiles): the same bytes
        direct = run_device(rtw, mean, v, g, rtw.denoise_opts(levels=levels, flags=rtw.DENOISE_DIRECT))
        assert direct[0].tobytes() == got[0].tobytes() and direct[1].tobytes() == got[1].tobytes(), what
    if w * h > 100:
        assert not np.array_equal(want[1], mean)  # (the filter did something)
        emp = var == rtw.VAR_EMPTY
        full = rtw.denoise_host(mean, var, guides, rtw.denoise_opts(levels=levels))[1]
        assert not full[emp].any() and full[~emp].all()  # empty pixels stay 0 and darken nobody to 0


# ------------------------------------------------------- accumulator path ----
def luminance_se2(stat, cnt, chunk):
    """rtw_adaptive.hpp pixel_se2 per pixel in numpy f64, the header's operation order."""
    m = (cnt // chunk).astype(np.float64)
    ms = np.where(m >= 2, m, 2.0)
    sy, sy2 = stat[..., 0], stat[..., 1]
    var = np.maximum(0.0, sy2 - sy * sy / ms)
    return var / (ms * (ms - 1.0) * np.float64(chunk) * np.float64(chunk))


def accumulator_case(rtw, target, cam, mk, one_shot, mask=None):
    import torch
    dev = "cuda:0"
    p = mk(60)
    h, w = p.row_count, p.width
    stream = torch.cuda.current_stream().cuda_stream
    acc = rtw.Accumulator(target, p)
    need = acc.workspace_bytes(20)
    ws = torch.empty(need + 256, dtype=torch.uint8, device=dev)
    ptr = (ws.data_ptr() + 255) & ~255
    if mask is not None:
        acc.set_mask(mask)
    for _ in range(2):
        acc.render_pass(cam, 20, ptr, need, stream)
    guides = torch.empty((h, w, 32), dtype=torch.uint8, device=dev)
    target.guides(cam, p, guides.data_ptr(), stream)
    rgb0 = torch.empty((h, w, 3), dtype=torch.uint8, device=dev)
    mean0 = torch.empty((h, w, 3), dtype=torch.float32, device=dev)
    acc.resolve(rgb0.data_ptr(), mean0.data_ptr(), stream)
    var = torch.empty((h, w), dtype=torch.float32, device=dev)
    acc.variance(var.data_ptr(), stream)
    torch.cuda.synchronize()
    before = acc.read()
    cnt = acc.counts() if mask is not None else np.full((h, w), 40, np.uint32)
    # the variance is pixel_se2 of the accumulator's statistic
    var_h = var.cpu().numpy()
    want_var = luminance_se2(before[1], cnt, 20).astype(np.float32)
    want_var[cnt // 20 < 2] = rtw.VAR_UNKNOWN
    want_var[cnt == 0] = rtw.VAR_EMPTY
    assert np.array_equal(u32(var_h), u32(want_var))
    assert (var_h > 0).any()
    if mask is not None:
        assert (cnt == 0).any() and (cnt == 40).any() and (var_h[cnt == 0] == rtw.VAR_EMPTY).all()
    # the entry = the host filter on the resolved mean, that variance and the guides
    dn_need = acc.denoise_workspace_bytes()
    dws = torch.full((dn_need + 256,), 0xFF, dtype=torch.uint8, device=dev)
    dptr = (dws.data_ptr() + 255) & ~255
    rgb = torch.zeros((h, w, 3), dtype=torch.uint8, device=dev)
    mean = torch.zeros((h, w, 3), dtype=torch.float32, device=dev)
    acc.denoise(guides.data_ptr(), dptr, dn_need, rgb.data_ptr(), mean.data_ptr(), None, stream)
    torch.cuda.synchronize()
    g_h = guides.cpu().numpy().view(rtw.GUIDE_DTYPE)[..., 0]
    want = rtw.denoise_host(mean0.cpu().numpy(), var_h, g_h)
    assert np.array_equal(u32(mean.cpu().numpy()), u32(want[1])) and np.array_equal(rgb.cpu().numpy(), want[0])
    assert not np.array_equal(want[1], mean0.cpu().numpy())
    if mask is not None:
        assert not mean.cpu().numpy()[cnt == 0].any()
    # the accumulator was not modified ...
    after = acc.read()
    assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()
    assert acc.samples() == 40
    # ... and one further pass still ends at the one-shot render's bytes
    acc.render_pass(cam, 20, ptr, need, stream)
    acc.resolve(rgb0.data_ptr(), mean0.data_ptr(), stream)
    torch.cuda.synchronize()
    ref = one_shot(mk(60))
    sel = np.ones((h, w), bool) if mask is None else acc.counts() == 60
    assert sel.any()
    assert np.array_equal(rgb0.cpu().numpy()[sel], ref[0][sel])
    assert np.array_equal(u32(mean0.cpu().numpy())[sel], u32(ref[1])[sel])
    acc.close()


@pytest.fixture(scope="module")
def cover(rtw):
    sph, mats, _ = rtw.cover_scene(42)
    return sph, mats, rtw.cover_camera(60 / 33), rtw.DeviceScene(sph, mats)


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_accumulator_denoise_cover(rtw, cover, precision):
    sph, mats, cam, scene = cover
    mk = lambda n: rtw.make_params(60, 33, n, precision=precision)
    accumulator_case(rtw, scene, cam, mk, lambda p: rtw.render(cam, sph, mats, p, want_mean=True))


def test_accumulator_denoise_masked(rtw, cover):
    sph, mats, cam, scene = cover
    mk = lambda n: rtw.make_params(60, 33, n)
    y, x = np.mgrid[0:33, 0:60]
    mask = ~(((x // 5 + y // 4) % 3 == 0) | ((x > 40) & (y < 9)))  # scattered blocks and a whole tile without samples
    accumulator_case(rtw, scene, cam, mk, lambda p: rtw.render(cam, sph, mats, p, want_mean=True), mask=mask)


def test_accumulator_denoise_world(rtw):
    from rtw_amd import world as Wd
    b = Wd.BuiltScene(6, 42)
    cam = b.camera()
    dw = Wd.DeviceWorld(b.desc)
    mk = lambda n: rtw.make_params(40, 40, n, background=b.background)
    accumulator_case(rtw, dw, cam, mk, lambda p: Wd.render_world(cam, b.desc, p, want_mean=True))
    dw.close()


def test_torch_accumulator_denoised(rtw, cover):
    """TorchAccumulator.guides() / .denoised(): the same bytes as the host filter, with and without guides."""
    import torch
    from rtw_amd.device import TorchAccumulator
    sph, mats, cam, scene = cover
    ta = TorchAccumulator(scene, rtw.make_params(60, 33, 40, chunk=10))
    ta.render_pass(cam, 20)
    g = ta.guides(cam)
    var = torch.empty((33, 60), dtype=torch.float32, device="cuda:0")
    ta.acc.variance(var.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert (var.cpu().numpy() >= 0).all()  # two chunks of 10: every variance is known
    g_h = g.cpu().numpy().view(rtw.GUIDE_DTYPE)[..., 0]
    for guides, guides_h in ((g, g_h), (None, None)):
        rgb, mean = ta.denoised(guides)
        torch.cuda.synchronize()
        want = rtw.denoise_host(ta.mean.cpu().numpy(), var.cpu().numpy(), guides_h)
        assert np.array_equal(u32(mean.cpu().numpy()), u32(want[1])) and np.array_equal(rgb.cpu().numpy(), want[0])
    assert ta.samples() == 20
    ta.close()


def test_cli_denoise_writes_the_accumulator_entrys_image(rtw, tmp_path):
    """bin/rtw_render --denoise: --out and every preview are rtw_accum_denoise_device's image of the
    samples so far, with the guides of the frame; without the flag the bytes are the plain run's."""
    import os
    import subprocess
    import torch
    from rtw_amd.device import TorchAccumulator
    from test_gpu_accum import _read_ppm
    exe = os.path.join(os.path.dirname(rtw.__file__), "..", "bin", "rtw_render")
    plain, dn, prev = tmp_path / "plain.ppm", tmp_path / "dn.ppm", tmp_path / "previews"
    base = [exe, "--scene", "1", "--width", "64", "--spp", "40", "--chunk", "10", "--pass-spp", "20"]
    for args in (base + ["--out", str(plain)],
                 base + ["--out", str(dn), "--denoise", "--denoise-levels", "4", "--preview-dir", str(prev)]):
        r = subprocess.run(args, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
    assert "note:" not in r.stderr  # (two chunks in every pass: nothing to warn about)
    got, first = _read_ppm(str(dn)), _read_ppm(str(prev / "pass_0001.ppm"))
    assert (prev / "pass_0002.ppm").read_bytes() == dn.read_bytes() and dn.read_bytes() != plain.read_bytes()
    h, w = got.shape[:2]
    assert (w, h) == (64, 42)
    sph, mats, _ = rtw.cover_scene(42)
    cam = rtw.cover_camera(3 / 2)  # the scene's own aspect (main.zig:304)
    scene = rtw.DeviceScene(sph, mats)
    ta = TorchAccumulator(scene, rtw.make_params(w, h, 40, chunk=10))
    g = ta.guides(cam)
    opts = rtw.denoise_opts(levels=4)
    for want in (first, got):
        ta.render_pass(cam, 20)
        rgb, _ = ta.denoised(g, opts)
        torch.cuda.synchronize()
        assert np.array_equal(rgb.cpu().numpy(), want)
    assert np.array_equal(ta.rgb.cpu().numpy(), _read_ppm(str(plain)))
    ta.close()
    scene.close()
    r = subprocess.run([exe, "--scene", "1", "--width", "64", "--spp", "20", "--denoise", "--out", str(dn)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "note:" in r.stderr and "--chunk 10" in r.stderr, r.stderr


def test_row_stride_is_refused(rtw, cover):
    import torch
    sph, mats, cam, scene = cover
    p = rtw.make_params(60, 33, 40, row_begin=1, row_stride=2)
    acc = rtw.Accumulator(scene, p)
    need = acc.workspace_bytes(20)
    ws = torch.empty(need + 256, dtype=torch.uint8, device="cuda:0")
    acc.render_pass(cam, 20, (ws.data_ptr() + 255) & ~255, need, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    buf = torch.empty(1 << 20, dtype=torch.uint8, device="cuda:0")
    st = rtw.lib().rtw_accum_denoise_device(acc.h, None, None, C.c_void_p((buf.data_ptr() + 255) & ~255), 1 << 19,
                                            C.c_void_p(buf.data_ptr()), None, None)
    assert st == rtw.RTW_UNSUPPORTED and b"row_stride" in rtw.lib().rtw_last_error()
    acc.close()
