"""Temporal accumulation on the GPU: rtw_temporal_device gives
rtw_temporal_host's bytes — history, mean and variance compared as u32 words —
at 2x2, 5x3, 67x9 (a row longer than one wave, with a remainder) and 130x5
(three tile columns, two tile rows): the first frame, a static step, a step
with fuzzed previous points that holds every rejection case (a numpy census of
the taps shows that the primitive test and the depth test each decided pixels
on their own), a second step fed from the device's own first output, the
optional outputs left out, two calls giving the same bytes, and the refused
arguments."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [(2, 2), (5, 3), (67, 9), (130, 5)]
DEPTH_TOL = 0.02  # rtw_temporal_opts.depth_tol's default, which every step here runs with


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32).reshape(-1)


def pixel_dirs(cam, w, h, fx, fy):
    """Feature-ray directions through (fractional) pixel positions, as the guides define s and t."""
    s = (fx + 0.5) / (w - 1)
    t = ((h - 1 - fy) + 0.5) / (h - 1)
    o, hz, vt, llc = (np.array(list(getattr(cam, n))) for n in ("origin", "horizontal", "vertical", "lower_left_corner"))
    return o, llc + s[..., None] * hz + t[..., None] * vt - o


def make_case(rtw, w, h, seed):
    """Two frames over one smooth scene: guides in blocks of four primitives (the boundaries at w/2 and 2h/3)
    and a block of misses; a depth step of 1.5 at x = 3w/4, INSIDE the primitives' blocks, so that taps across
    it differ from the pixel in depth alone; and previous points half a pixel or so away — with NaN points,
    points behind the camera, the camera's own origin (determinant 0), points far outside the image, and
    points moved along their own ray to (1 +- 2 tol) times the depth (same primitive at every tap of the
    block's interior, every depth off) among them."""
    rng = np.random.default_rng(seed)
    cam = rtw.camera_init((13, 2, 3), (0, 0, 0), (0, 1, 0), 20.0, w / h, 0.0, 10.0)
    cam_moved = rtw.camera_init((13.02, 2.01, 3), (0, 0, 0), (0, 1, 0), 20.0, w / h, 0.0, 10.0)
    y, x = np.mgrid[0:h, 0:w]
    g = np.zeros((h, w), rtw.GUIDE_DTYPE)
    g["prim"] = 1 + (x >= w // 2) + 2 * (y >= (2 * h) // 3)
    g["depth"] = (2.0 + 0.004 * x + 0.003 * y + 1.5 * (x >= (3 * w) // 4)).astype(np.float32)
    g["normal"][..., 2] = 1.0
    g["albedo"] = 0.5
    miss = (x < max(1, w // 5)) & (y < max(1, h // 2))
    for f in ("prim", "depth", "normal", "albedo"):
        g[f][miss] = 0
    means = rng.uniform(0, 2, (2, h, w, 3)).astype(np.float32)
    o, d = pixel_dirs(cam, w, h, x + rng.uniform(-1.2, 1.2, (h, w)), y + rng.uniform(-1.2, 1.2, (h, w)))
    kind = rng.random((h, w))
    depth = g["depth"].astype(np.float64)
    depth[(kind >= 0.16) & (kind < 0.22)] *= 1.0 + 2 * DEPTH_TOL
    depth[(kind >= 0.22) & (kind < 0.28)] *= 1.0 - 2 * DEPTH_TOL
    pp = o + depth[..., None] * d
    pp[kind < 0.04] = np.nan
    pp[(kind >= 0.04) & (kind < 0.08)] = o
    behind = (kind >= 0.08) & (kind < 0.12)
    pp[behind] = 2 * o - pp[behind]
    far = (kind >= 0.12) & (kind < 0.16)
    pp[far] = (o + 3.0 * pixel_dirs(cam, w, h, x + 5.0 * w, y - 4.0 * h)[1])[far]
    return dict(w=w, h=h, cam=cam, cam_moved=cam_moved, g=g, means=means, pp=np.ascontiguousarray(pp))


def tap_census(c, cam_prev):
    """The taps of every hit pixel of the fuzzed step, restated in numpy: for each pixel, how many taps lie
    inside the image and carry the pixel's primitive, and how many of those pass / fail the depth test by a
    clear margin (ratio below tol / 2, above 3 tol / 2).  Pixels whose previous point does not project
    (NaN, determinant 0, behind the camera) have no taps here."""
    w, h, g = c["w"], c["h"], c["g"]
    o, hz, vt, llc = (np.array(list(getattr(cam_prev, n))) for n in ("origin", "horizontal", "vertical", "lower_left_corner"))
    same_prim, passes, fails = (np.zeros((h, w), int) for _ in range(3))
    for y in range(h):
        for x in range(w):
            q = c["pp"][y, x] - o
            if g["prim"][y, x] == 0 or not np.isfinite(q).all() or abs(np.linalg.det(np.stack([hz, vt, -q], 1))) < 1e-12:
                continue
            s, t, mu = np.linalg.solve(np.stack([hz, vt, -q], 1), o - llc)  # d0 + s h + t v = mu q
            if mu <= 0:
                continue
            fx, fy, tp = s * (w - 1) - 0.5, (h - 1) + 0.5 - t * (h - 1), 1.0 / mu
            for ty in (int(np.floor(fy)), int(np.floor(fy)) + 1):
                for tx in (int(np.floor(fx)), int(np.floor(fx)) + 1):
                    if 0 <= tx < w and 0 <= ty < h and g["prim"][ty, tx] == g["prim"][y, x]:
                        rd = float(g["depth"][ty, tx])
                        ratio = abs(rd - tp) / max(rd, tp)
                        same_prim[y, x] += 1
                        passes[y, x] += ratio < 0.5 * DEPTH_TOL
                        fails[y, x] += ratio > 1.5 * DEPTH_TOL
    return same_prim, passes, fails


def device_step(rtw, c, mean, hist_in, prev_p, cam_prev, opts=None, outputs=True):
    """rtw_temporal_device on fresh buffers with guard bands: (hist, mean_out, var_out) as numpy."""
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
    rtw.temporal_device(t_mean.data_ptr(), t_g.data_ptr(), t_pp.data_ptr() if t_pp is not None else None, cam_prev, c["cam"],
                        t_hi.data_ptr() if t_hi is not None else None, w, h, t_ho.data_ptr(),
                        t_mo.data_ptr() if outputs else None, t_vo.data_ptr() if outputs else None, opts,
                        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    ho, mo, vo = t_ho.cpu().numpy(), t_mo.cpu().numpy(), t_vo.cpu().numpy()
    assert (ho[h * w * 32:] == 0xA5).all() and np.isnan(mo[h * w * 3:]).all() and np.isnan(vo[h * w:]).all()
    if not outputs:
        assert np.isnan(mo).all() and np.isnan(vo).all()
    assert np.array_equal(u32(t_mean.cpu().numpy()), u32(mean))  # the inputs are not modified
    return ho[:h * w * 32].view(rtw.HISTORY_DTYPE).reshape(h, w), mo[:h * w * 3].reshape(h, w, 3), vo[:h * w].reshape(h, w)


def same(got, want, where):
    for a, b, what in zip(got, want, ("history", "mean", "variance")):
        bad = np.nonzero(u32(a) != u32(b))[0]
        assert bad.size == 0, (where, what, bad[:8])


@pytest.fixture(scope="module", params=SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def case(request, rtw):
    w, h = request.param
    c = make_case(rtw, w, h, 100 * w + h)
    c["first"] = rtw.temporal_host(c["means"][0], c["g"], c["cam"], c["cam"])  # shared, read-only
    return c


def test_first_frame(rtw, case):
    got = device_step(rtw, case, case["means"][0], None, None, case["cam"])
    same(got, case["first"], "first frame")
    assert (got[0]["len"] == 1).all() and u32(got[1]).tobytes() == u32(case["means"][0]).tobytes()


def test_static_step(rtw, case):
    opts = rtw.temporal_opts(min_len_var=2)
    want = rtw.temporal_host(case["means"][1], case["g"], case["cam"], case["cam"], hist_in=case["first"][0], opts=opts)
    got = device_step(rtw, case, case["means"][1], case["first"][0], None, case["cam"], opts)
    same(got, want, "static step")
    assert (got[0]["len"] == 2).all() and (got[2] >= 0).all()


@pytest.mark.parametrize("moved_camera", [False, True])
def test_fuzzed_previous_points(rtw, case, moved_camera):
    opts = rtw.temporal_opts(min_len_var=2)
    cam_prev = case["cam_moved"] if moved_camera else case["cam"]
    want = rtw.temporal_host(case["means"][1], case["g"], cam_prev, case["cam"], hist_in=case["first"][0],
                             prev_p=case["pp"], opts=opts)
    got = device_step(rtw, case, case["means"][1], case["first"][0], case["pp"], cam_prev, opts)
    same(got, want, "fuzzed previous points")
    if case["w"] * case["h"] > 100:  # both branches ran, and the rejections were there to be taken
        hit = case["g"]["prim"] > 0
        assert (got[0]["len"][hit] > 1).sum() > 20 and (got[0]["len"][hit] == 1).sum() > 20
        assert np.isnan(case["pp"]).any()
        assert ((got[0]["len"][~hit] == 1).all()) == moved_camera  # a miss keeps its history iff the camera stood still
        # the depth test decided on its own: pixels whose in-image taps of their own primitive are all off in depth
        # lost their history, and at the depth step inside a block it split the taps of one pixel
        same_prim, passes, fails = tap_census(case, cam_prev)
        depth_only = (same_prim > 0) & (fails == same_prim)
        assert depth_only.sum() > 20 and (got[0]["len"][depth_only] == 1).all()
        assert ((passes > 0) & (fails > 0)).sum() >= 3
        kept = (passes == same_prim) & (same_prim == 4)  # four taps inside, the pixel's primitive, depths agreeing
        assert kept.sum() > 20 and (got[0]["len"][kept] == 2).all()


def test_second_step_from_the_devices_own_output(rtw, case):
    opts = rtw.temporal_opts(min_len_var=2, max_history=1)
    first = device_step(rtw, case, case["means"][0], None, None, case["cam"], opts)
    second = device_step(rtw, case, case["means"][1], first[0], case["pp"], case["cam"], opts)
    third = device_step(rtw, case, case["means"][0], second[0], None, case["cam"], opts)
    h1 = rtw.temporal_host(case["means"][0], case["g"], case["cam"], case["cam"], opts=opts)
    h2 = rtw.temporal_host(case["means"][1], case["g"], case["cam"], case["cam"], hist_in=h1[0], prev_p=case["pp"], opts=opts)
    h3 = rtw.temporal_host(case["means"][0], case["g"], case["cam"], case["cam"], hist_in=h2[0], opts=opts)
    same(second, h2, "second step")
    same(third, h3, "third step")
    assert (third[0]["len"] == 2).all()  # max_history 1: N = 1 for good


def test_optional_outputs_and_repeatability(rtw, case):
    a = device_step(rtw, case, case["means"][1], case["first"][0], case["pp"], case["cam"])
    b = device_step(rtw, case, case["means"][1], case["first"][0], case["pp"], case["cam"])
    same(a, b, "two calls")
    c = device_step(rtw, case, case["means"][1], case["first"][0], case["pp"], case["cam"], outputs=False)
    assert np.array_equal(u32(c[0]), u32(a[0]))


def test_refused_arguments(rtw):
    import torch
    w, h = 5, 3
    L = rtw.lib()
    cam = rtw.camera_init((13, 2, 3), (0, 0, 0), (0, 1, 0), 20.0, w / h, 0.0, 10.0)
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    base = (buf.data_ptr() + 255) & ~255
    mean, guides, hist_in, hist_out, mean_out, var_out, pp = (base + 512 * k for k in range(7))

    def call(**kw):
        a = dict(mean=mean, guides=guides, prev_p=None, cam_prev=C.byref(cam), cam=C.byref(cam), hist_in=None, w=w, h=h,
                 opts=None, hist_out=hist_out, mean_out=mean_out, var_out=var_out)
        a.update(kw)
        return L.rtw_temporal_device(a["mean"], a["guides"], a["prev_p"], a["cam_prev"], a["cam"], a["hist_in"], a["w"],
                                     a["h"], a["opts"], a["hist_out"], a["mean_out"], a["var_out"], None)
    assert call() == rtw.RTW_OK and call(hist_in=hist_in, prev_p=pp) == rtw.RTW_OK
    for bad in (dict(mean=None), dict(guides=None), dict(cam_prev=None), dict(cam=None), dict(hist_out=None), dict(w=1),
                dict(h=1), dict(guides=guides + 8), dict(hist_in=hist_in + 8), dict(hist_out=hist_out + 16 + 4),
                dict(prev_p=pp + 4), dict(hist_in=hist_out), dict(mean_out=mean),
                dict(hist_in=hist_in, hist_out=hist_in + 32), dict(mean_out=mean + 12), dict(var_out=hist_out + 64),
                dict(opts=C.byref(rtw.temporal_opts(max_history=4097))), dict(opts=C.byref(rtw.temporal_opts(depth_tol=-1.0))),
                dict(opts=C.byref(rtw.temporal_opts(min_len_var=1))), dict(opts=C.byref(rtw.temporal_opts(flags=2)))):
        assert call(**bad) == rtw.RTW_EINVAL, bad
    torch.cuda.synchronize()
