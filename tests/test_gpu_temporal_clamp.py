"""The clamped temporal accumulation on the GPU:
rtw_temporal_clamped_device gives rtw_temporal_clamped_host's bytes — history,
mean and variance compared as u32 words — with radius 1, 2 and 3 at 2x2, 5x3,
64x4 (exactly one tile), 65x5 (one pixel into the next tile both ways: the halo
crosses tile edges and the lanes outside the image must still reach the
barrier), 67x9 and 130x5, on the fuzz of tests/test_gpu_temporal.py with a few
non-finite pixels in the current mean: the first frame, a static step, the
fuzzed step under a still and a moved camera, a second step fed from the
device's own output, the optional outputs left out, clamp NULL against
rtw_temporal_device, two calls giving the same bytes, the refused arguments,
and two frames of the Cornell box through TemporalAccumulator(clamp=...)."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_temporal import make_case, u32

pytestmark = pytest.mark.gpu

SIZES = [(2, 2), (5, 3), (64, 4), (65, 5), (67, 9), (130, 5)]
RADII = [1, 2, 3]
GAMMA = 1.0


def device_step(rtw, c, mean, hist_in, prev_p, cam_prev, opts=None, clamp=None, outputs=True, entry="clamped"):
    """rtw_temporal_clamped_device (entry "plain": rtw_temporal_device) on fresh buffers with guard bands:
    (hist, mean_out, var_out) as numpy."""
    import torch
    w, h = c["w"], c["h"]
    dev = "cuda:0"
    t_mean = torch.from_numpy(np.ascontiguousarray(mean)).to(dev)
    t_g = torch.from_numpy(c["g"].view(np.uint8).reshape(h, w, 32)).to(dev)
    t_hi = torch.from_numpy(np.ascontiguousarray(hist_in).view(np.uint8).reshape(h, w, 32)).to(dev) if hist_in is not None else None
    t_pp = torch.from_numpy(prev_p).to(dev) if prev_p is not None else None
    guard = 64
    t_ho = torch.full((h * w * 32 + guard,), 0xA5, dtype=torch.uint8, device=dev)
    t_mo = torch.full((h * w * 3 + guard,), float("nan"), dtype=torch.float32, device=dev)
    t_vo = torch.full((h * w + guard,), float("nan"), dtype=torch.float32, device=dev)
    args = (t_mean.data_ptr(), t_g.data_ptr(), t_pp.data_ptr() if t_pp is not None else None, cam_prev, c["cam"],
            t_hi.data_ptr() if t_hi is not None else None, w, h, t_ho.data_ptr(), t_mo.data_ptr() if outputs else None,
            t_vo.data_ptr() if outputs else None, opts)
    stream = torch.cuda.current_stream().cuda_stream
    if entry == "plain":
        rtw.temporal_device(*args, stream)
    else:
        rtw.temporal_clamped_device(*args, clamp, stream)
    torch.cuda.synchronize()
    ho, mo, vo = t_ho.cpu().numpy(), t_mo.cpu().numpy(), t_vo.cpu().numpy()
    assert (ho[h * w * 32:] == 0xA5).all() and np.isnan(mo[h * w * 3:]).all() and np.isnan(vo[h * w:]).all()
    if not outputs:
        assert np.isnan(mo).all() and np.isnan(vo).all()
    assert np.array_equal(u32(t_mean.cpu().numpy()), u32(mean))  # the inputs are not modified
    assert np.array_equal(t_g.cpu().numpy().reshape(-1), c["g"].view(np.uint8).reshape(-1))
    if t_hi is not None:
        assert np.array_equal(u32(t_hi.cpu().numpy()), u32(hist_in))
    return ho[:h * w * 32].view(rtw.HISTORY_DTYPE).reshape(h, w), mo[:h * w * 3].reshape(h, w, 3), vo[:h * w].reshape(h, w)


def same(got, want, where):
    for a, b, what in zip(got, want, ("history", "mean", "variance")):
        bad = np.nonzero(u32(a) != u32(b))[0]
        assert bad.size == 0, (where, what, bad[:8])


@pytest.fixture(scope="module", params=SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def case(request, rtw):
    """make_case's two frames with non-finite pixels in both means (one in 16, at least one; none at 2x2, where
    every window is the four pixels and one bad pixel would leave n = 3 and nothing clamped), the first frame's
    history from the host, and the clamp of each radius.  Shared, read-only."""
    w, h = request.param
    c = make_case(rtw, w, h, 200 * w + h)
    rng = np.random.default_rng(7 * w + h)
    for k in range(2):
        for j in range(max(1, w * h // 16) if w * h > 4 else 0):
            c["means"][k, rng.integers(h), rng.integers(w), rng.integers(3)] = (np.nan, np.inf, -np.inf)[j % 3]
    c["first"] = rtw.temporal_host(c["means"][0], c["g"], c["cam"], c["cam"])
    c["clamps"] = {r: rtw.temporal_clamp(GAMMA, r) for r in RADII}
    return c


@pytest.mark.parametrize("r", RADII)
def test_first_frame(rtw, case, r):
    got = device_step(rtw, case, case["means"][0], None, None, case["cam"], clamp=case["clamps"][r])
    same(got, rtw.temporal_clamped_host(case["means"][0], case["g"], case["cam"], case["cam"], clamp=case["clamps"][r]), "first frame")
    ok = np.isfinite(case["means"][0]).all(axis=-1)  # no history, nothing to clamp: the unclamped first frame
    for a, b in zip(got, case["first"]):
        assert np.array_equal(u32(a[ok]), u32(b[ok]))
    assert (got[0]["len"] == 1).all()


@pytest.mark.parametrize("r", RADII)
def test_static_step(rtw, case, r):
    opts, k = rtw.temporal_opts(min_len_var=2), case["clamps"][r]
    want = rtw.temporal_clamped_host(case["means"][1], case["g"], case["cam"], case["cam"], hist_in=case["first"][0], opts=opts, clamp=k)
    got = device_step(rtw, case, case["means"][1], case["first"][0], None, case["cam"], opts, k)
    same(got, want, "static step")
    assert (got[0]["len"] == 2).all()
    plain = rtw.temporal_host(case["means"][1], case["g"], case["cam"], case["cam"], hist_in=case["first"][0], opts=opts)
    assert not np.array_equal(u32(got[1]), u32(plain[1]))  # the clamp did something


@pytest.mark.parametrize("moved_camera", [False, True])
@pytest.mark.parametrize("r", RADII)
def test_fuzzed_previous_points(rtw, case, r, moved_camera):
    opts, k = rtw.temporal_opts(min_len_var=2), case["clamps"][r]
    cam_prev = case["cam_moved"] if moved_camera else case["cam"]
    want = rtw.temporal_clamped_host(case["means"][1], case["g"], cam_prev, case["cam"], hist_in=case["first"][0],
                                     prev_p=case["pp"], opts=opts, clamp=k)
    got = device_step(rtw, case, case["means"][1], case["first"][0], case["pp"], cam_prev, opts, k)
    same(got, want, "fuzzed previous points")
    if case["w"] * case["h"] > 100:  # both branches ran, and the clamp bit on pixels with history
        hit = case["g"]["prim"] > 0
        assert (got[0]["len"][hit] > 1).sum() > 20 and (got[0]["len"][hit] == 1).sum() > 20
        plain = rtw.temporal_host(case["means"][1], case["g"], cam_prev, case["cam"], hist_in=case["first"][0],
                                  prev_p=case["pp"], opts=opts)
        differs = (got[1] != plain[1]).any(axis=-1) & np.isfinite(plain[1]).all(axis=-1)
        assert differs.sum() > 20 and (got[0]["len"][differs] > 1).all()
        assert np.array_equal(u32(got[0]["len"]), u32(plain[0]["len"]))  # len is untouched


@pytest.mark.parametrize("r", RADII)
def test_second_step_from_the_devices_own_output(rtw, case, r):
    opts, k = rtw.temporal_opts(min_len_var=2, max_history=1), case["clamps"][r]
    first = device_step(rtw, case, case["means"][0], None, None, case["cam"], opts, k)
    second = device_step(rtw, case, case["means"][1], first[0], case["pp"], case["cam"], opts, k)
    third = device_step(rtw, case, case["means"][0], second[0], None, case["cam"], opts, k)
    h1 = rtw.temporal_clamped_host(case["means"][0], case["g"], case["cam"], case["cam"], opts=opts, clamp=k)
    h2 = rtw.temporal_clamped_host(case["means"][1], case["g"], case["cam"], case["cam"], hist_in=h1[0], prev_p=case["pp"], opts=opts, clamp=k)
    h3 = rtw.temporal_clamped_host(case["means"][0], case["g"], case["cam"], case["cam"], hist_in=h2[0], opts=opts, clamp=k)
    same(second, h2, "second step")
    same(third, h3, "third step")
    assert (third[0]["len"] == 2).all()  # max_history 1: N = 1 for good


def test_optional_outputs_no_clamp_and_repeatability(rtw, case):
    k = rtw.temporal_clamp(0.5, 2)
    a = device_step(rtw, case, case["means"][1], case["first"][0], case["pp"], case["cam"], clamp=k)
    b = device_step(rtw, case, case["means"][1], case["first"][0], case["pp"], case["cam"], clamp=k)
    same(a, b, "two calls")
    c = device_step(rtw, case, case["means"][1], case["first"][0], case["pp"], case["cam"], clamp=k, outputs=False)
    assert np.array_equal(u32(c[0]), u32(a[0]))
    none = device_step(rtw, case, case["means"][1], case["first"][0], case["pp"], case["cam"], clamp=None)
    plain = device_step(rtw, case, case["means"][1], case["first"][0], case["pp"], case["cam"], entry="plain")
    same(none, plain, "clamp NULL against rtw_temporal_device")
    default = device_step(rtw, case, case["means"][1], case["first"][0], case["pp"], case["cam"], clamp=rtw.temporal_clamp())
    same(default, rtw.temporal_clamped_host(case["means"][1], case["g"], case["cam"], case["cam"], hist_in=case["first"][0],
                                            prev_p=case["pp"], clamp=rtw.temporal_clamp()), "the default clamp")


def test_refused_arguments(rtw):
    import torch
    w, h = 5, 3
    L = rtw.lib()
    cam = rtw.camera_init((13, 2, 3), (0, 0, 0), (0, 1, 0), 20.0, w / h, 0.0, 10.0)
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    base = (buf.data_ptr() + 255) & ~255
    mean, guides, hist_in, hist_out, mean_out, var_out, pp = (base + 512 * k for k in range(7))
    ok_clamp = rtw.temporal_clamp(1.0, 1)

    def call(**kw):
        a = dict(mean=mean, guides=guides, prev_p=None, cam_prev=C.byref(cam), cam=C.byref(cam), hist_in=None, w=w, h=h,
                 opts=None, clamp=C.byref(ok_clamp), hist_out=hist_out, mean_out=mean_out, var_out=var_out)
        a.update(kw)
        return L.rtw_temporal_clamped_device(a["mean"], a["guides"], a["prev_p"], a["cam_prev"], a["cam"], a["hist_in"],
                                             a["w"], a["h"], a["opts"], a["clamp"], a["hist_out"], a["mean_out"],
                                             a["var_out"], None)
    assert call() == rtw.RTW_OK and call(hist_in=hist_in, prev_p=pp) == rtw.RTW_OK and call(clamp=None) == rtw.RTW_OK
    for clamp in (None, C.byref(ok_clamp)):
        for bad in (dict(mean=None), dict(guides=None), dict(cam_prev=None), dict(cam=None), dict(hist_out=None), dict(w=1),
                    dict(h=1), dict(guides=guides + 8), dict(hist_in=hist_in + 8), dict(hist_out=hist_out + 16 + 4),
                    dict(prev_p=pp + 4), dict(hist_in=hist_out), dict(mean_out=mean),
                    dict(hist_in=hist_in, hist_out=hist_in + 32), dict(mean_out=mean + 12), dict(var_out=hist_out + 64),
                    dict(opts=C.byref(rtw.temporal_opts(max_history=4097))), dict(opts=C.byref(rtw.temporal_opts(depth_tol=-1.0))),
                    dict(opts=C.byref(rtw.temporal_opts(min_len_var=1))), dict(opts=C.byref(rtw.temporal_opts(flags=1))),
                    dict(opts=C.byref(rtw.temporal_opts(flags=2)))):
            assert call(clamp=clamp, **bad) == rtw.RTW_EINVAL, bad
    for k in (rtw.TemporalClamp(-0.5, 0, 0), rtw.TemporalClamp(np.nan, 0, 0), rtw.TemporalClamp(np.inf, 0, 0),
              rtw.TemporalClamp(1e30, 0, 0), rtw.TemporalClamp(1.0, 4, 0), rtw.TemporalClamp(1.0, 1, 1)):
        assert call(clamp=C.byref(k)) == rtw.RTW_EINVAL, (k.gamma, k.radius, k.reserved)
    torch.cuda.synchronize()


def test_two_frames_of_the_cornell_box_through_the_accumulator(rtw):
    """Two renders (seeds s, s + 1) of the Cornell box through TemporalAccumulator(clamp=...): the second
    step's history, mean and variance are rtw_temporal_clamped_host's of the same frames, and the clamp bit."""
    import torch
    from rtw_amd import world as W
    from rtw_amd.device import TemporalAccumulator
    w = h = 48
    built = W.BuiltScene(6, 42, None)
    cam = built.camera(1.0)
    dw = W.DeviceWorld(built.desc)
    try:
        dev, s = "cuda:0", torch.cuda.current_stream().cuda_stream
        clamp, opts = rtw.temporal_clamp(gamma=1.0, radius=2), rtw.temporal_opts(min_len_var=2)
        ta = TemporalAccumulator(w, h, opts=opts, device=0, clamp=clamp)
        frames = []
        for k in range(2):
            p = rtw.make_params(w, h, 20, seed=7 + k, background=built.background)
            nb = dw.workspace_bytes(p)
            ws = torch.empty(nb + 256, dtype=torch.uint8, device=dev)
            rgb = torch.empty((h, w, 3), dtype=torch.uint8, device=dev)
            mean = torch.empty((h, w, 3), dtype=torch.float32, device=dev)
            dw.render_async(cam, p, (ws.data_ptr() + 255) & ~255, nb, rgb.data_ptr(), mean.data_ptr(), s)
            rays = torch.empty((w * h, 9), dtype=torch.float64, device=dev)
            hits = torch.empty((w * h, 10), dtype=torch.float64, device=dev)
            rtw.pixel_rays_device(cam, w, h, rays.data_ptr(), s)
            dw.trace(rays.data_ptr(), w * h, hits.data_ptr(), None, s)
            g = torch.empty((h, w, 32), dtype=torch.uint8, device=dev)
            dw.guides(cam, p, g.data_ptr(), s)
            pp = torch.empty((h, w, 3), dtype=torch.float64, device=dev)
            dw.prev_points_device(hits.data_ptr(), w * h, 0.5, pp.data_ptr(), None, None, s)
            mean_out, var_out = ta.step(mean, g, cam, pp)
            torch.cuda.synchronize()
            frames.append((mean.cpu().numpy(), g.cpu().numpy().reshape(-1).view(rtw.GUIDE_DTYPE).reshape(h, w), pp.cpu().numpy()))
        hist = ta.history().cpu().numpy().reshape(-1).view(rtw.HISTORY_DTYPE).reshape(h, w)
        h1 = rtw.temporal_clamped_host(frames[0][0], frames[0][1], cam, cam, prev_p=frames[0][2], opts=opts, clamp=clamp)
        h2 = rtw.temporal_clamped_host(frames[1][0], frames[1][1], cam, cam, hist_in=h1[0], prev_p=frames[1][2], opts=opts, clamp=clamp)
        same((hist, mean_out.cpu().numpy(), var_out.cpu().numpy()), h2, "Cornell box, second frame")
        assert (hist["len"] == 2).all()
        plain = rtw.temporal_host(frames[1][0], frames[1][1], cam, cam, hist_in=h1[0], prev_p=frames[1][2], opts=opts)
        assert (plain[1] != h2[1]).any(axis=-1).sum() > w * h // 20
    finally:
        dw.close()
