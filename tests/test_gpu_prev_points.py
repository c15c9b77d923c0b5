"""The per-frame pieces of temporal accumulation on the GPU:
rtw_pixel_rays_device gives rtw_pixel_ray's bytes for every pixel;
rtw_world_prev_points_device gives rtw_world_prev_points_host's bytes (u64
words) on the mixed world, the Cornell box and a sphere world whose BVH has
leaves of one (its stored order differs from the list's), for the hits of a
48x27 frame, displaced previous numbers and two times; and end to end on the
Cornell box two frames of one world and camera accumulate to len 2 and to the
average of the two renders."""
import ctypes as C

import numpy as np
import pytest

from helpers import MIXED_CAMERA, MIXED_SIZES, _rot, _to_desc, mixed_bvh_world
from update_helpers import displace, numbers

pytestmark = pytest.mark.gpu

FW, FH = 48, 27
GEN_SEED = 5


def u64(a):
    return np.ascontiguousarray(a).view(np.uint64).reshape(-1)


@pytest.fixture(scope="module")
def W(rtw):
    from rtw_amd import world
    return world


def frame_hits(rtw, dw, cam, w, h):
    """(rays, hits) tensors of the frame's feature rays: rtw_pixel_rays_device, rtw_world_trace_device."""
    import torch
    n = w * h
    rays = torch.empty((n, 9), dtype=torch.float64, device="cuda:0")
    hits = torch.empty((n, 10), dtype=torch.float64, device="cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    rtw.pixel_rays_device(cam, w, h, rays.data_ptr(), s)
    dw.trace(rays.data_ptr(), n, hits.data_ptr(), None, s)
    torch.cuda.synchronize()
    return rays, hits


@pytest.mark.parametrize("w,h", [(5, 3), (67, 9)])
def test_pixel_rays_equal_the_host_helper(rtw, w, h):
    import torch
    cam = rtw.camera_init((13, 2, 3), (0.5, 0.2, 0), (0, 1, 0), 27.0, w / h, 0.1, 9.0, 0.25, 1.0)
    buf = torch.full((w * h * 9 + 16,), float("nan"), dtype=torch.float64, device="cuda:0")
    rtw.pixel_rays_device(cam, w, h, buf.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert np.isnan(got[w * h * 9:]).all()
    want = np.zeros(w * h, rtw.RAY_DTYPE)
    for y in range(h):
        for x in range(w):
            r = rtw.pixel_ray(cam, w, h, x, y)
            want[y * w + x] = (tuple(r.origin), tuple(r.dir), r.time, r.t_min, r.t_max)
    assert np.array_equal(u64(got[:w * h * 9]), u64(want))
    L = rtw.lib()
    for args in ((None, w, h, buf.data_ptr()), (C.byref(cam), w, h, None), (C.byref(cam), 1, h, buf.data_ptr()),
                 (C.byref(cam), w, 1, buf.data_ptr()), (C.byref(cam), w, h, buf.data_ptr() + 4)):
        assert L.rtw_pixel_rays_device(*args, None) == rtw.RTW_EINVAL


def _worlds(rtw, W):
    """name -> (desc, keep, camera, a_prev, xv_prev)"""
    m = MIXED_CAMERA
    cam = rtw.camera_init(m["look_from"], m["look_at"], (0, 1, 0), m["vfov"], FW / FH, m["aperture"], m["focus"], 0.0, 1.0)
    out = {}
    for name, (nb, ns, variant) in (("mixed", (*MIXED_SIZES["small"], None)), ("spheres600", (0, 600, "spheres_image"))):
        t = mixed_bvh_world(W, W.earth_map(), nb, ns, GEN_SEED, variant=variant)
        desc, keep = _to_desc(W, *t)
        a, xv = numbers(displace(t))
        out[name] = (desc, keep, cam, a, xv)
    built = W.BuiltScene(6, 42, None)
    a, xv = W.desc_numbers(built.desc)
    rng = np.random.default_rng(6)
    for i in range(built.desc.n_xforms):
        for k in range(built.desc.xforms[i].n):
            xv[i, k] = _rot(xv[i, k, 2] + rng.uniform(-0.6, 0.6)) if built.desc.xforms[i].op[k] == 1 else xv[i, k] + rng.uniform(-20, 20, 3)
    a[:, 0:5] += rng.uniform(-3, 3, (len(a), 5))  # (every rect's four bounds and its plane)
    out["cornell"] = (built.desc, built, built.camera(FW / FH), a, xv)
    return out


@pytest.fixture(scope="module")
def worlds(rtw, W):
    return _worlds(rtw, W)


@pytest.mark.parametrize("name", ["mixed", "cornell", "spheres600"])
def test_prev_points_device_equals_host(rtw, W, worlds, name):
    import torch
    desc, _, cam, a_prev, xv_prev = worlds[name]
    dw = W.DeviceWorld(desc)
    try:
        if name == "spheres600":
            info = dw.bvh_info()
            assert desc.n_prims >= 512 and info["max_leaf"] == 1, info
        rays, hits = frame_hits(rtw, dw, cam, FW, FH)
        n = FW * FH
        h_host = hits.cpu().numpy().reshape(-1).view(rtw.HIT_DTYPE)
        hit = h_host["prim"] > 0
        assert hit.sum() > n // 4
        kinds = {desc.prims[int(p) - 1].kind for p in np.unique(h_host["prim"][hit])}
        assert len(kinds) >= (1 if name != "mixed" else 3), kinds
        d_a = torch.from_numpy(a_prev).cuda()
        d_xv = torch.from_numpy(xv_prev).cuda() if xv_prev.size else None
        s = torch.cuda.current_stream().cuda_stream
        for time in (0.5, 0.0):
            for use_a, use_xv in ((True, True), (True, False), (False, True), (False, False)):
                if use_xv and d_xv is None:
                    continue
                out = torch.full((n * 3 + 8,), float("nan"), dtype=torch.float64, device="cuda:0")
                dw.prev_points_device(hits.data_ptr(), n, time, out.data_ptr(), d_a.data_ptr() if use_a else None,
                                      d_xv.data_ptr() if use_xv else None, s)
                torch.cuda.synchronize()
                got = out.cpu().numpy()
                assert np.isnan(got[n * 3:]).all()
                want = W.prev_points_host(desc, h_host, time, a_prev if use_a else None, xv_prev if use_xv else None)
                bad = np.nonzero(u64(got[:n * 3]) != u64(want))[0]
                assert bad.size == 0, (name, time, use_a, use_xv, bad[:6] // 3, h_host[bad[:2] // 3])
                if not use_a and not use_xv:
                    assert np.array_equal(u64(want.reshape(n, 3)[hit]), u64(h_host["p"][hit]))
                    assert (u64(want.reshape(n, 3)[~hit]) == 0).all()
                elif use_a and name != "cornell":
                    assert np.abs(want.reshape(n, 3)[hit] - h_host["p"][hit]).max() > 0.5  # the numbers did move
        L = rtw.lib()
        assert L.rtw_world_prev_points_device(dw.h, hits.data_ptr(), n, float("nan"), None, None, out.data_ptr(), None) == rtw.RTW_EINVAL
        assert L.rtw_world_prev_points_device(None, hits.data_ptr(), n, 0.5, None, None, out.data_ptr(), None) == rtw.RTW_EINVAL
        assert L.rtw_world_prev_points_device(dw.h, None, n, 0.5, None, None, out.data_ptr(), None) == rtw.RTW_EINVAL
        assert L.rtw_world_prev_points_device(dw.h, hits.data_ptr(), n, 0.5, None, None, out.data_ptr() + 4, None) == rtw.RTW_EINVAL
        assert L.rtw_world_prev_points_device(dw.h, None, 0, 0.5, None, None, None, None) == rtw.RTW_OK
    finally:
        dw.close()


def test_two_frames_of_the_cornell_box_end_to_end(rtw, W):
    """Two renders (seeds s, s + 1) of one world and camera, their first hits followed back with the world's own
    numbers (NULL arrays): every pixel's guide prim is equal in both frames, so every pixel has len 2, and the
    accumulated mean is the f32-rounded average of the two renders' means (two f32 roundings: rtol 1e-6)."""
    import torch
    from rtw_amd.device import TemporalAccumulator
    w = h = 48
    built = W.BuiltScene(6, 42, None)
    cam = built.camera(1.0)
    dw = W.DeviceWorld(built.desc)
    try:
        dev, s = "cuda:0", torch.cuda.current_stream().cuda_stream
        ta = TemporalAccumulator(w, h, device=0)
        means, guides = [], []
        for k in range(2):
            p = rtw.make_params(w, h, 20, seed=7 + k, background=built.background)
            nb = dw.workspace_bytes(p)
            ws = torch.empty(nb + 256, dtype=torch.uint8, device=dev)
            ptr = (ws.data_ptr() + 255) & ~255
            rgb = torch.empty((h, w, 3), dtype=torch.uint8, device=dev)
            mean = torch.empty((h, w, 3), dtype=torch.float32, device=dev)
            dw.render_async(cam, p, ptr, nb, rgb.data_ptr(), mean.data_ptr(), s)
            rays, hits = frame_hits(rtw, dw, cam, w, h)
            g = torch.empty((h, w, 32), dtype=torch.uint8, device=dev)
            dw.guides(cam, p, g.data_ptr(), s)
            pp = torch.empty((h, w, 3), dtype=torch.float64, device=dev)
            dw.prev_points_device(hits.data_ptr(), w * h, 0.5, pp.data_ptr(), None, None, s)
            mean_out, var_out = ta.step(mean, g, cam, pp)
            torch.cuda.synchronize()
            means.append(mean.cpu().numpy())
            guides.append(g.cpu().numpy().reshape(-1).view(rtw.GUIDE_DTYPE))
        assert np.array_equal(guides[0]["prim"], guides[1]["prim"]) and (guides[0]["prim"] > 0).sum() > w * h // 2
        hist = ta.history().cpu().numpy().reshape(-1).view(rtw.HISTORY_DTYPE)
        assert (hist["len"] == 2).all()
        avg = ((means[0].astype(np.float64) + means[1].astype(np.float64)) / 2).astype(np.float32)
        assert not np.array_equal(means[0], means[1])
        np.testing.assert_allclose(mean_out.cpu().numpy(), avg, rtol=1e-6, atol=0)
        assert (var_out.cpu().numpy() == rtw.VAR_UNKNOWN).all()  # len 2 < min_len_var's default
    finally:
        dw.close()
