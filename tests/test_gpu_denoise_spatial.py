"""The spatial variance estimate on the GPU:
rtw_denoise_spatial_variance_device gives rtw_denoise_spatial_variance_host's
bytes (compared as u32 words) in both of its forms, at every size at which the
kernel's tiles and halos take another path; the flagged filter entry gives the
flagged host filter's bytes; the flagged accumulator entry is resolve +
variance + estimate + filter without touching the accumulator; and the CLI's
--denoise-spatial writes that entry's image."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def synthetic(rtw, w, h, seed):
    """A noisy image, a mixed known / unknown / empty variance map, and guides that hold a block
    of misses, a normal discontinuity, a depth step and slowly varying albedo."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = 0.5 + 0.4 * np.sin(x / 7.0)[..., None] * np.cos(y / 5.0)[..., None] * np.array([1.0, 0.8, 0.6])
    mean = (base + rng.normal(0.0, 0.05, (h, w, 3))).clip(0.0, 4.0).astype(np.float32)
    var = rng.uniform(1e-4, 4e-3, (h, w)).astype(np.float32)
    kind = rng.integers(0, 8, (h, w))
    var[kind <= 3] = rtw.VAR_UNKNOWN
    var[kind == 4] = 0.0
    empty = kind == 5
    var[empty] = rtw.VAR_EMPTY
    mean[empty] = 0.0
    g = np.zeros((h, w), rtw.GUIDE_DTYPE)
    miss = (x >= w // 3) & (x < w // 3 + max(1, w // 5)) & (y >= h // 4) & (y < h // 4 + max(1, h // 3))  # a block
    turn = x >= (2 * w) // 3   # the normal turns by ~37 degrees there
    far = y >= (3 * h) // 5    # the depth steps there
    ang = 0.01 * x + 0.015 * y + 0.65 * turn
    g["normal"] = np.stack([np.sin(ang), np.zeros_like(ang), np.cos(ang)], axis=-1)
    g["depth"] = 2.0 + 0.01 * x + 1.5 * far + rng.uniform(0.0, 0.02, (h, w))
    g["albedo"] = 0.4 + 0.05 * np.sin(x / 11.0)[..., None] + rng.uniform(0.0, 0.03, (h, w, 3))
    g["prim"] = 1 + turn + 2 * far
    g["prim"][miss] = 0
    g["normal"][miss] = 0.0
    g["depth"][miss] = 0.0
    g["albedo"][miss] = (0.7, 0.8, 1.0)
    return mean, var, g


def to_dev(rtw, mean, var, guides):
    import torch
    h, w = mean.shape[:2]
    dev = "cuda:0"
    t_mean = torch.from_numpy(mean).to(dev)
    t_var = torch.from_numpy(var).to(dev) if var is not None else None
    t_g = torch.from_numpy(guides.view(np.uint8).reshape(h, w, 32)).to(dev) if guides is not None else None
    return t_mean, t_var, t_g


def estimate_device(rtw, mean, var, guides, opts):
    import torch
    h, w = mean.shape[:2]
    t_mean, t_var, t_g = to_dev(rtw, mean, var, guides)
    out = torch.full((h * w + 64,), float("nan"), dtype=torch.float32, device="cuda:0")  # (with a guard band)
    rtw.spatial_variance_device(t_mean.data_ptr(), t_var.data_ptr() if t_var is not None else None,
                                t_g.data_ptr() if t_g is not None else None, w, h, opts, out.data_ptr(),
                                torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert np.isnan(o[h * w:]).all()  # nothing written past the image
    assert np.array_equal(t_mean.cpu().numpy(), mean)  # the inputs are not modified
    if var is not None:
        assert np.array_equal(u32(t_var.cpu().numpy()), u32(var))
    return o[:h * w].reshape(h, w)


# 70x5: an x halo across two tiles and more rows than a tile; 65x9: a one-pixel second tile column and three tile rows
@pytest.mark.parametrize("w,h", [(1, 1), (3, 2), (5, 3), (70, 5), (65, 9), (150, 100)])
def test_estimate_device_equals_host_bit_for_bit(rtw, w, h):
    mean, var, guides = synthetic(rtw, w, h, 77 * w + h)
    if w * h > 300:  # the generator made every kind of pixel and guide
        assert (var == 0).any() and (var == rtw.VAR_UNKNOWN).any() and (var == rtw.VAR_EMPTY).any() and (var > 0).any()
        assert (guides["prim"] == 0).any() and len(np.unique(guides["prim"])) >= 4
    sig = dict(sigma_normal=0.3, sigma_depth=0.5, sigma_albedo=0.2)  # (wide enough that taps across the steps count)
    for v, g in ((var, guides), (None, guides), (var, None), (None, None)):
        what = (w, h, v is not None, g is not None)
        want = rtw.spatial_variance_host(mean, v, g, rtw.denoise_opts(**sig))
        got = estimate_device(rtw, mean, v, g, rtw.denoise_opts(**sig))
        assert np.array_equal(u32(got), u32(want)), (what, int((u32(got) != u32(want)).sum()))
        again = estimate_device(rtw, mean, v, g, rtw.denoise_opts(**sig))  # no state: the same bytes
        assert got.tobytes() == again.tobytes(), what
        direct = estimate_device(rtw, mean, v, g, rtw.denoise_opts(flags=rtw.DENOISE_DIRECT, **sig))
        assert direct.tobytes() == got.tobytes(), what
        if w * h > 300:
            unk = (v == rtw.VAR_UNKNOWN) if v is not None else np.ones((h, w), bool)
            assert (got[unk] > 0).mean() > 0.9  # (the kernel estimated)
            if v is not None:
                assert np.array_equal(u32(got)[~unk], u32(v)[~unk])  # known and empty: bit for bit
    if w * h > 300:  # the guides matter: their estimate differs from the unguided one
        assert not np.array_equal(rtw.spatial_variance_host(mean, None, guides, rtw.denoise_opts(**sig)),
                                  rtw.spatial_variance_host(mean, None, None))


def filter_device(rtw, mean, var, guides, opts):
    import torch
    h, w = mean.shape[:2]
    t_mean, t_var, t_g = to_dev(rtw, mean, var, guides)
    need = rtw.denoise_workspace_bytes(w, h, opts)
    ws = torch.full((need + 512,), 0xFF, dtype=torch.uint8, device="cuda:0")
    ptr = (ws.data_ptr() + 255) & ~255
    rgb = torch.full((h, w, 3), 7, dtype=torch.uint8, device="cuda:0")
    out = torch.full((h, w, 3), float("nan"), dtype=torch.float32, device="cuda:0")
    rtw.denoise_device(t_mean.data_ptr(), t_var.data_ptr() if t_var is not None else None,
                       t_g.data_ptr() if t_g is not None else None, w, h, opts, ptr, need, rgb.data_ptr(),
                       out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    tail = ws.cpu().numpy()[(ptr - ws.data_ptr()) + need:]
    assert (tail == 0xFF).all()  # the workspace's declared size is all the call writes
    return rgb.cpu().numpy(), out.cpu().numpy()


@pytest.mark.parametrize("levels", [1, 2, 5])  # (1 and 2: where the estimate's place in the ping-pong images matters)
@pytest.mark.parametrize("w,h", [(5, 3), (60, 33)])
def test_flagged_filter_device_equals_host(rtw, w, h, levels):
    mean, var, guides = synthetic(rtw, w, h, 13 * w + levels)
    for v, g in ((var, guides), (None, guides), (None, None)):
        for extra in (0, rtw.DENOISE_DIRECT):
            opts = rtw.denoise_opts(levels=levels, flags=rtw.DENOISE_SPATIAL_VAR | extra)
            want = rtw.denoise_host(mean, v, g, opts)
            got = filter_device(rtw, mean, v, g, opts)
            what = (w, h, levels, v is not None, g is not None, extra)
            assert np.array_equal(u32(got[1]), u32(want[1])), (what, int((u32(got[1]) != u32(want[1])).sum()))
            assert np.array_equal(got[0], want[0]), what
        if w * h > 300:  # (the flag did something)
            assert not np.array_equal(want[1], rtw.denoise_host(mean, v, g, rtw.denoise_opts(levels=levels))[1]), what


# ------------------------------------------------------- accumulator path ----
def accumulator_case(rtw, mask=None):
    """One default-chunk 20-sample pass of the cover scene at 64x36: no pixel has two chunks."""
    import torch
    dev = "cuda:0"
    w, h = 64, 36
    sph, mats, _ = rtw.cover_scene(42)
    cam = rtw.cover_camera(w / h)
    scene = rtw.DeviceScene(sph, mats)
    p = rtw.make_params(w, h, 40)
    assert rtw.effective_chunk(p) == 20
    stream = torch.cuda.current_stream().cuda_stream
    acc = rtw.Accumulator(scene, p)
    need = acc.workspace_bytes(20)
    ws = torch.empty(need + 256, dtype=torch.uint8, device=dev)
    ptr = (ws.data_ptr() + 255) & ~255
    if mask is not None:
        acc.set_mask(mask)
    acc.render_pass(cam, 20, ptr, need, stream)
    guides = torch.empty((h, w, 32), dtype=torch.uint8, device=dev)
    scene.guides(cam, p, guides.data_ptr(), stream)
    rgb0 = torch.empty((h, w, 3), dtype=torch.uint8, device=dev)
    mean0 = torch.empty((h, w, 3), dtype=torch.float32, device=dev)
    acc.resolve(rgb0.data_ptr(), mean0.data_ptr(), stream)
    var = torch.empty((h, w), dtype=torch.float32, device=dev)
    acc.variance(var.data_ptr(), stream)
    torch.cuda.synchronize()
    before = acc.read()
    var_h = var.cpu().numpy()
    cnt = acc.counts() if mask is not None else np.full((h, w), 20, np.uint32)
    assert (var_h[cnt > 0] == rtw.VAR_UNKNOWN).all() and (var_h[cnt == 0] == rtw.VAR_EMPTY).all()
    opts = rtw.denoise_opts(flags=rtw.DENOISE_SPATIAL_VAR)
    dn_need = acc.denoise_workspace_bytes(opts)
    assert dn_need == acc.denoise_workspace_bytes()
    dws = torch.full((dn_need + 256,), 0xFF, dtype=torch.uint8, device=dev)
    dptr = (dws.data_ptr() + 255) & ~255
    rgb = torch.zeros((h, w, 3), dtype=torch.uint8, device=dev)
    mean = torch.full((h, w, 3), float("nan"), dtype=torch.float32, device=dev)
    acc.denoise(guides.data_ptr(), dptr, dn_need, rgb.data_ptr(), mean.data_ptr(), opts, stream)
    torch.cuda.synchronize()
    g_h = guides.cpu().numpy().view(rtw.GUIDE_DTYPE)[..., 0]
    want = rtw.denoise_host(mean0.cpu().numpy(), var_h, g_h, opts)
    plain = rtw.denoise_host(mean0.cpu().numpy(), var_h, g_h)
    got_mean, got_rgb = mean.cpu().numpy(), rgb.cpu().numpy()
    assert np.array_equal(u32(got_mean), u32(want[1])) and np.array_equal(got_rgb, want[0])
    assert not np.array_equal(want[1], plain[1])  # (the estimate switched the colour term on)
    after = acc.read()  # the accumulator is only read
    assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()
    assert acc.samples() == 20
    acc.close()
    scene.close()
    return cnt, got_mean, got_rgb


def test_accumulator_single_chunk_pass(rtw):
    accumulator_case(rtw)


def test_accumulator_masked_keeps_unsampled_pixels_zero(rtw):
    y, x = np.mgrid[0:36, 0:64]
    mask = ~((x >= 20) & (x < 31) & (y >= 9) & (y < 17))  # a block that is never sampled
    cnt, mean, rgb = accumulator_case(rtw, mask=mask)
    assert (cnt[~mask] == 0).all() and (cnt[mask] == 20).all()
    assert not mean[~mask].any() and not rgb[~mask].any()
    assert mean[mask].any(axis=-1).all()  # and darken nobody to 0


def test_cli_denoise_spatial_writes_the_flagged_entrys_image(rtw, tmp_path):
    """bin/rtw_render --denoise --denoise-spatial on a single default chunk: --out is the flagged accumulator
    entry's image and the note says the variance is estimated; without the option the bytes and the note's
    advice are the unflagged run's; the option alone is refused."""
    import os
    import subprocess
    import torch
    from rtw_amd.device import TorchAccumulator
    from test_gpu_accum import _read_ppm
    exe = os.path.join(os.path.dirname(rtw.__file__), "..", "bin", "rtw_render")
    plain, flagged = tmp_path / "plain.ppm", tmp_path / "flagged.ppm"
    base = [exe, "--scene", "1", "--width", "64", "--spp", "20", "--denoise"]
    r0 = subprocess.run(base + ["--out", str(plain)], capture_output=True, text=True, timeout=120)
    r1 = subprocess.run(base + ["--denoise-spatial", "--out", str(flagged)], capture_output=True, text=True, timeout=120)
    assert r0.returncode == 0 and r1.returncode == 0, r0.stderr + r1.stderr
    assert "note:" in r0.stderr and "--chunk 10" in r0.stderr and "--denoise-spatial" in r0.stderr
    assert "note:" in r1.stderr and "estimated from the image" in r1.stderr and "--chunk" not in r1.stderr
    got = _read_ppm(str(flagged))
    h, w = got.shape[:2]
    assert (w, h) == (64, 42) and flagged.read_bytes() != plain.read_bytes()
    sph, mats, _ = rtw.cover_scene(42)
    cam = rtw.cover_camera(3 / 2)  # the scene's own aspect
    scene = rtw.DeviceScene(sph, mats)
    ta = TorchAccumulator(scene, rtw.make_params(w, h, 20))
    g = ta.guides(cam)
    ta.render_pass(cam, 20)
    for path, opts in ((plain, None), (flagged, rtw.denoise_opts(flags=rtw.DENOISE_SPATIAL_VAR))):
        rgb, _ = ta.denoised(g, opts)
        torch.cuda.synchronize()
        assert np.array_equal(rgb.cpu().numpy(), _read_ppm(str(path)))
    ta.close()
    scene.close()
    r = subprocess.run([exe, "--scene", "1", "--width", "64", "--spp", "20", "--denoise-spatial"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "need --denoise" in r.stderr
