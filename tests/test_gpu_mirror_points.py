"""rtw_world_mirror_points_device on the GPU, held as uint64
words against the pipeline a caller would run without it: mirror_rays_host,
rtw_world_trace_device on the flagged rays only (the yardstick: the existing
query tests hold it to the oracle), mirror_points_host.

Worlds: a hand-made one (a metal sphere, a moving metal sphere, a fuzzy metal
sphere, a metal rect under Translate + RotateY, a glass sphere, a Lambert
ground and a moving Lambert sphere, a light, and small Lambert spheres that
bring it past 32 primitives) created with RTW_WORLD_LINEAR and with its BVH
(the union walk); and the spheres-only world of the query tests, for which the
plan chooses the per-lane walk, with a batch one 64-ray block beyond the
device-filling grid so that lanes take further records.  Batches of 1, 63, 64,
65 and 257 records with a time per ray; pixel-ray frames of 5x3 and 67x9."""
import ctypes as C

import numpy as np
import pytest

from helpers import MIXED_CAMERA, _rot, _to_desc, mixed_bvh_world
from update_helpers import displace, numbers

pytestmark = pytest.mark.gpu

GEN_SEED = 5
LOOK_FROM, LOOK_AT, VFOV = (0.0, 3.0, 9.0), (0.0, 1.0, 0.0), 35.0


def u64(a):
    return np.ascontiguousarray(a).view(np.uint64).reshape(-1)


@pytest.fixture(scope="module")
def W(rtw):
    from rtw_amd import world
    return world


def hand_tables(W):
    tex = [dict(kind=W.TEX_SOLID, color=(0.5, 0.5, 0.5)), dict(kind=W.TEX_SOLID, color=(4.0, 4.0, 4.0))]
    mats = [dict(kind=W.WMAT_LAMBERT, tex=0), dict(kind=W.WMAT_METAL, albedo=(0.8, 0.8, 0.8), fuzz=0.0),
            dict(kind=W.WMAT_METAL, albedo=(0.8, 0.6, 0.2), fuzz=0.4), dict(kind=W.WMAT_DIELECTRIC, ir=1.5),
            dict(kind=W.WMAT_LIGHT, tex=1)]
    xf = [dict(n=2, op=[W.XF_TRANSLATE, W.XF_ROTATE_Y], v=[(0.2, 0.0, -2.5), _rot(0.25)])]

    def sph(c, r, m):
        return dict(kind=W.PRIM_SPHERE, mat=m, xform=-1, a=[*c, *c, r, 0, 0])

    def mov(c0, c1, r, m):
        return dict(kind=W.PRIM_MOVING_SPHERE, mat=m, xform=-1, a=[*c0, *c1, r, 0.0, 1.0])
    prims = [sph((0, -1000, 0), 1000.0, 0), sph((-2.2, 1.0, 0.0), 1.0, 1), mov((0.3, 0.7, 1.5), (0.3, 1.1, 1.5), 0.7, 1),
             sph((2.3, 0.8, 0.5), 0.8, 2), dict(kind=W.PRIM_XY_RECT, mat=1, xform=0, a=[-3.0, 3.0, 0.0, 2.5, 0.0]),
             sph((-0.6, 0.5, 3.0), 0.5, 3), dict(kind=W.PRIM_XZ_RECT, mat=4, xform=-1, a=[-2.0, 2.0, -2.0, 2.0, 6.0]),
             mov((1.5, 0.4, 3.0), (1.8, 0.4, 3.2), 0.4, 0)]
    rng = np.random.default_rng(21)
    for _ in range(30):  # past 32 primitives: the world gets a BVH unless RTW_WORLD_LINEAR
        prims.append(sph((float(rng.uniform(-5, 5)), 0.15, float(rng.uniform(3.5, 6.0))), 0.15, 0))
    return prims, xf, tex, mats, [], []


def hand_prev(tables):
    """Last frame's numbers of the hand-made world: the spheres a little off, the chain turned and shifted."""
    a, xv = numbers(tables)
    rng = np.random.default_rng(22)
    for i, p in enumerate(tables[0]):
        if p["kind"] <= 1 and abs(p["a"][6]) < 100:
            d = rng.uniform(-0.08, 0.08, 3) * (1, 0, 1)
            a[i, 0:3] += d
            a[i, 3:6] += d
    xv[0, 0] += (0.05, 0.0, -0.04)
    xv[0, 1] = _rot(0.25 + 0.03)
    return a, xv


def camera(rtw, look_from, w, h):
    return rtw.camera_init(look_from, LOOK_AT, (0, 1, 0), VFOV, w / h, 0.0, 9.0, 0.0, 1.0)


def pixel_rays(rtw, cam, w, h, times_seed=None):
    import torch
    rays = torch.empty((w * h, 9), dtype=torch.float64, device="cuda:0")
    rtw.pixel_rays_device(cam, w, h, rays.data_ptr(), torch.cuda.current_stream().cuda_stream)
    if times_seed is not None:
        t = np.random.default_rng(times_seed).uniform(0.0, 1.0, w * h)
        rays[:, 6] = torch.from_numpy(t).cuda()
    torch.cuda.synchronize()
    return rays


def pipeline(rtw, W, dw, desc, d_rays, cam_prev, a_prev, xv_prev, opts=None):
    """The records of d_rays, and what mirror_points_device has to give for them."""
    import torch
    n, s = d_rays.shape[0], torch.cuda.current_stream().cuda_stream
    d_hits = torch.empty((n, 10), dtype=torch.float64, device="cuda:0")
    dw.trace(d_rays.data_ptr(), n, d_hits.data_ptr(), None, s)
    torch.cuda.synchronize()
    r = d_rays.cpu().numpy().reshape(-1).view(rtw.RAY_DTYPE)
    h = d_hits.cpu().numpy().reshape(-1).view(rtw.HIT_DTYPE)
    rays2, flag = W.mirror_rays_host(desc, r, h)
    idx = np.nonzero(flag)[0]
    hits2 = np.zeros(n, rtw.HIT_DTYPE)
    if idx.size:
        d_r2 = torch.from_numpy(np.ascontiguousarray(rays2[idx]).view(np.float64).reshape(-1, 9)).cuda()
        d_h2 = torch.empty((idx.size, 10), dtype=torch.float64, device="cuda:0")
        dw.trace(d_r2.data_ptr(), idx.size, d_h2.data_ptr(), None, s)
        torch.cuda.synchronize()
        hits2[idx] = d_h2.cpu().numpy().reshape(-1).view(rtw.HIT_DTYPE)
    want = W.mirror_points_host(desc, r, h, hits2, cam_prev, a_prev, xv_prev, opts)
    return d_hits, h, flag.astype(bool), hits2, want


def device_points(dw, d_rays, d_hits, cam_prev, d_a, d_xv, opts=None, with_hits2=True):
    """(prev_p (n, 3), hits2 (n, 10) or None) of the device entry, each buffer followed by NaNs that must stay."""
    import torch
    n = d_rays.shape[0]
    out = torch.full((n * 3 + 8,), float("nan"), dtype=torch.float64, device="cuda:0")
    h2 = torch.full((n * 10 + 8,), float("nan"), dtype=torch.float64, device="cuda:0") if with_hits2 else None
    dw.mirror_points_device(d_rays.data_ptr(), d_hits.data_ptr(), n, cam_prev, out.data_ptr(),
                            d_a.data_ptr() if d_a is not None else None, d_xv.data_ptr() if d_xv is not None else None,
                            opts, h2.data_ptr() if with_hits2 else None, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.isnan(got[n * 3:]).all()
    got2 = None
    if with_hits2:
        got2 = h2.cpu().numpy()
        assert np.isnan(got2[n * 10:]).all()
        got2 = got2[:n * 10].reshape(n, 10)
    return got[:n * 3].reshape(n, 3), got2


def assert_equal(rtw, got, got2, want, hits2, where):
    bad = np.nonzero(u64(got) != u64(want))[0]
    assert bad.size == 0, (where, "prev_p", bad[:6] // 3, got.reshape(-1)[bad[:3]], want.reshape(-1)[bad[:3]])
    if got2 is not None:
        bad = np.nonzero(u64(got2) != u64(hits2))[0]
        assert bad.size == 0, (where, "hits2", bad[:6] // 10)


@pytest.fixture(scope="module")
def hand(rtw, W):
    tables = hand_tables(W)
    desc, keep = _to_desc(W, *tables)
    a_prev, xv_prev = hand_prev(tables)
    return desc, keep, a_prev, xv_prev


@pytest.mark.parametrize("linear", [True, False], ids=["linear", "union"])
def test_hand_made_world(rtw, W, hand, linear):
    import torch
    desc, _, a_prev, xv_prev = hand
    dw = W.DeviceWorld(desc, linear=linear)
    try:
        assert dw.query_info()["traversal"] == ("linear" if linear else "union")
        d_a, d_xv = torch.from_numpy(a_prev).cuda(), torch.from_numpy(xv_prev).cuda()
        s = torch.cuda.current_stream().cuda_stream
        seen = dict(hit=0, sky=0, fell_back=0, kinds=set(), fuzzy=0)
        # ---- pixel-ray frames (every ray at time 0.5), the camera moved as well; then the world standing still
        for (w, h) in ((5, 3), (67, 9)):
            cam, cam_prev = camera(rtw, LOOK_FROM, w, h), camera(rtw, (4.0, 3.4, 7.5), w, h)
            d_rays = pixel_rays(rtw, cam, w, h)
            n = w * h
            for use_a, use_xv in ((True, True), (True, False), (False, True), (False, False)):
                ap, xp = (a_prev if use_a else None), (xv_prev if use_xv else None)
                d_hits, hrec, flag, hits2, want = pipeline(rtw, W, dw, desc, d_rays, cam_prev, ap, xp)
                got, got2 = device_points(dw, d_rays, d_hits, cam_prev, d_a if use_a else None, d_xv if use_xv else None)
                assert_equal(rtw, got, got2, want, hits2, (w, h, use_a, use_xv))
                # non-mirror records and misses: rtw_world_prev_points_device's bytes
                pp = torch.empty((n, 3), dtype=torch.float64, device="cuda:0")
                dw.prev_points_device(d_hits.data_ptr(), n, 0.5, pp.data_ptr(), d_a.data_ptr() if use_a else None,
                                      d_xv.data_ptr() if use_xv else None, s)
                torch.cuda.synchronize()
                surf = pp.cpu().numpy()
                assert np.array_equal(u64(got[~flag]), u64(surf[~flag])), (w, h, use_a, use_xv)
                if not use_a and not use_xv:  # "the world stood still, the camera may not have"
                    assert np.array_equal(u64(got[~flag]), u64(np.where((hrec["prim"] > 0)[:, None], hrec["p"], 0.0)[~flag]))
                    if (w, h) == (67, 9):
                        assert np.abs(got[flag] - hrec["p"][flag]).max() > 1e-3  # the mirrors did follow the camera
                if (w, h) == (67, 9) and use_a and use_xv:
                    same = (u64(got).reshape(n, 3) == u64(surf).reshape(n, 3)).all(axis=1)
                    seen["hit"] += int((flag & (hits2["prim"] > 0)).sum())
                    seen["sky"] += int((flag & (hits2["prim"] == 0)).sum())
                    seen["fell_back"] += int((flag & same).sum())
                    seen["kinds"] |= {int(desc.prims[int(p) - 1].kind) for p in hrec["prim"][flag]}
                    seen["fuzzy"] += int((hrec["prim"][flag] == 4).sum())
                    seen["glass"] = seen.get("glass", 0) + int((hrec["prim"] == 6).sum())
                    assert not flag[hrec["prim"] == 6].any()  # glass is no mirror
                    # the predictor alone, one step, eight steps: each the host's bytes, and not all the same
                    outs = []
                    for o in (rtw.mirror_opts(flags=rtw.MIRROR_PREDICT_ONLY), rtw.mirror_opts(1), rtw.mirror_opts(8)):
                        _, _, _, _, want_o = pipeline(rtw, W, dw, desc, d_rays, cam_prev, ap, xp, o)
                        got_o, _ = device_points(dw, d_rays, d_hits, cam_prev, d_a, d_xv, o, with_hits2=False)
                        assert_equal(rtw, got_o, None, want_o, None, ("opts", o.steps, o.flags))
                        outs.append(got_o.tobytes())
                    assert len(set(outs)) == 3 and got.tobytes() not in outs[:2]
        # the batch holds what it claims to test
        print("mirror records of the 67x9 frame:", seen)
        assert seen["hit"] > 0 and seen["sky"] > 0 and seen["fell_back"] > 0, seen
        assert {0, 1, 2} <= seen["kinds"] and seen["fuzzy"] > 0 and seen["glass"] > 0, seen
        # ---- batches with a time per ray, cut from a shuffled 67x9 frame that starts with a mirror record
        cam, cam_prev = camera(rtw, LOOK_FROM, 67, 9), camera(rtw, (0.6, 3.1, 8.8), 67, 9)
        all_rays = pixel_rays(rtw, cam, 67, 9, times_seed=23)
        _, _, flag, _, _ = pipeline(rtw, W, dw, desc, all_rays, cam_prev, a_prev, xv_prev)
        order = np.random.default_rng(24).permutation(67 * 9)
        first = int(np.nonzero(flag[order])[0][0])
        order[[0, first]] = order[[first, 0]]
        shuffled = all_rays[torch.from_numpy(order).cuda()].contiguous()
        for n in (1, 63, 64, 65, 257):
            d_rays = shuffled[:n].contiguous()
            d_hits, hrec, flag, hits2, want = pipeline(rtw, W, dw, desc, d_rays, cam_prev, a_prev, xv_prev)
            assert flag[0] and (n == 1 or (~flag).any())
            got, got2 = device_points(dw, d_rays, d_hits, cam_prev, d_a, d_xv)
            assert_equal(rtw, got, got2, want, hits2, ("batch", n))
            again, _ = device_points(dw, d_rays, d_hits, cam_prev, d_a, d_xv, with_hits2=False)
            assert again.tobytes() == got.tobytes()  # the same inputs give the same bytes, with or without d_hits2
    finally:
        dw.close()


def test_per_lane_walk_with_regeneration(rtw, W):
    import torch
    tables = mixed_bvh_world(W, W.earth_map(), 0, 600, GEN_SEED, variant="spheres_image")
    desc, keep = _to_desc(W, *tables)
    a_prev, xv_prev = numbers(displace(tables, k_range=(0.05, 0.2)))
    dw = W.DeviceWorld(desc)
    try:
        info = dw.query_info()
        assert info["traversal"] == "lane", info
        n = info["grid"] * 256 + 64  # one 64-ray block beyond what fills the device: a wave takes a second block
        w = 768
        h = -(-n // w)
        m = MIXED_CAMERA
        cam = rtw.camera_init(m["look_from"], m["look_at"], (0, 1, 0), m["vfov"], w / h, 0.0, m["focus"], 0.0, 1.0)
        cam_prev = rtw.camera_init((1.0, 7.2, 18.5), m["look_at"], (0, 1, 0), m["vfov"], w / h, 0.0, m["focus"], 0.0, 1.0)
        d_rays = pixel_rays(rtw, cam, w, h)[:n].contiguous()
        d_a = torch.from_numpy(a_prev).cuda()
        for use_a in (True, False):
            d_hits, hrec, flag, hits2, want = pipeline(rtw, W, dw, desc, d_rays, cam_prev, a_prev if use_a else None, None)
            # mirrors are a minority here as in a frame: most lanes finish a record at once and take another
            assert 0 < flag.sum() < 0.5 * n
            assert (flag & (hits2["prim"] > 0)).any() and (flag & (hits2["prim"] == 0)).any()
            got, got2 = device_points(dw, d_rays, d_hits, cam_prev, d_a if use_a else None, None)
            assert_equal(rtw, got, got2, want, hits2, ("lane", use_a))
    finally:
        dw.close()
    del keep


def test_refused_arguments(rtw, W, hand):
    import torch
    desc, _, a_prev, xv_prev = hand
    dw = W.DeviceWorld(desc)
    try:
        w, h = 16, 8
        n = w * h
        cam = camera(rtw, LOOK_FROM, w, h)
        d_rays = pixel_rays(rtw, cam, w, h)
        d_hits = torch.empty((n, 10), dtype=torch.float64, device="cuda:0")
        dw.trace(d_rays.data_ptr(), n, d_hits.data_ptr(), None, torch.cuda.current_stream().cuda_stream)
        out = torch.zeros((n + 1, 3), dtype=torch.float64, device="cuda:0")
        h2 = torch.zeros((n + 1, 10), dtype=torch.float64, device="cuda:0")
        d_a, d_xv = torch.from_numpy(a_prev).cuda(), torch.from_numpy(xv_prev).cuda()
        big = torch.zeros((n * 13 + 16,), dtype=torch.float64, device="cuda:0")  # room for hits2 and prev_p side by side
        L, V = rtw.lib(), C.c_void_p
        R, H, O, H2, A, X, B = (t.data_ptr() for t in (d_rays, d_hits, out, h2, d_a, d_xv, big))

        def call(world=dw.h, r=R, hh=H, nn=n, cp=C.byref(cam), a=A, x=X, o=None, pp=O, hits2=H2):
            return L.rtw_world_mirror_points_device(world, V(r) if r else None, V(hh) if hh else None, nn, cp,
                                                    V(a) if a else None, V(x) if x else None, o, V(pp) if pp else None,
                                                    V(hits2) if hits2 else None, None)
        assert call() == rtw.RTW_OK and call(hits2=None) == rtw.RTW_OK and call(a=None, x=None) == rtw.RTW_OK
        cases = {
            "null world": dict(world=None), "null cam_prev": dict(cp=None), "null d_rays": dict(r=None),
            "null d_hits": dict(hh=None), "null d_prev_p": dict(pp=None), "n > 2^31": dict(nn=(1 << 31) + 1),
            "d_rays not aligned": dict(r=R + 4), "d_hits not aligned": dict(hh=H + 4), "d_prev_p not aligned": dict(pp=O + 4),
            "d_hits2 not aligned": dict(hits2=H2 + 4), "d_a_prev not aligned": dict(a=A + 4), "d_xv_prev not aligned": dict(x=X + 4),
            "steps 9": dict(o=C.byref(rtw.mirror_opts(9))), "unknown flag": dict(o=C.byref(rtw.mirror_opts(0, 2))),
            "d_prev_p on d_rays": dict(pp=R), "d_prev_p inside d_hits": dict(pp=H + 80 * n - 8),
            "d_hits2 on d_hits": dict(hits2=H), "d_hits2 inside d_rays": dict(hits2=R + 72 * n - 8),
            "d_prev_p on d_a_prev": dict(pp=A + 72 * desc.n_prims - 8), "d_hits2 on d_xv_prev": dict(hits2=X),
            "the outputs overlap": dict(pp=B + 80 * n - 8, hits2=B),
        }
        for what, kw in cases.items():
            assert call(**kw) == rtw.RTW_EINVAL, what
            assert L.rtw_last_error(), what
        assert call(pp=B + 80 * n, hits2=B) == rtw.RTW_OK  # adjacent is not overlapping
        assert call(r=None, hh=None, nn=0, pp=None, hits2=None) == rtw.RTW_OK  # n == 0 launches nothing
        assert call(nn=0, cp=None) == rtw.RTW_EINVAL and call(nn=0, o=C.byref(rtw.mirror_opts(9))) == rtw.RTW_EINVAL
        torch.cuda.synchronize()
        if torch.cuda.device_count() > 1:  # a world that lives on another device
            with torch.cuda.device(1):
                assert call() == rtw.RTW_EINVAL
    finally:
        dw.close()


def test_torch_tracer(rtw, W, hand):
    """TorchTracer.mirror_points gives the entry's bytes, on torch's current stream."""
    import torch
    from rtw_amd.device import TorchTracer
    desc, _, a_prev, xv_prev = hand
    dw = W.DeviceWorld(desc)
    try:
        w, h = 67, 9
        cam, cam_prev = camera(rtw, LOOK_FROM, w, h), camera(rtw, (0.6, 3.1, 8.8), w, h)
        d_rays = pixel_rays(rtw, cam, w, h)
        d_a, d_xv = torch.from_numpy(a_prev).cuda(), torch.from_numpy(xv_prev).cuda()
        d_hits, hrec, flag, hits2, want = pipeline(rtw, W, dw, desc, d_rays, cam_prev, a_prev, xv_prev)
        tr = TorchTracer(dw)
        pp, rec2 = tr.mirror_points(d_rays, d_hits, cam_prev, d_a, d_xv, hits2=True)
        torch.cuda.synchronize()
        assert_equal(rtw, pp.cpu().numpy(), rec2.cpu().numpy(), want, hits2, "torch")
        # on another stream than the default one: the launch follows torch's current stream
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            pp2 = tr.mirror_points(d_rays, d_hits, cam_prev, d_a, d_xv)
        side.synchronize()
        assert np.array_equal(u64(pp2.cpu().numpy()), u64(want))
        with pytest.raises(ValueError):
            tr.mirror_points(d_rays[:, :8], d_hits, cam_prev)
    finally:
        dw.close()
