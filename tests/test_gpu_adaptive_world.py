"""Adaptive sampling of general worlds: the world kernel's masked
passes keep the per-pixel contract — a pixel that holds n samples has
rtw_world_render's bytes with spp = n there — on the Cornell box (rects,
transform chains) and on the globe + 10k spheres under the per-lane BVH walk,
with the tail dealing's rings in the workspace and without; and a per-pixel
budget calibrated on the frame itself stops about half the pixels early."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_adaptive import luminance_se2, u32

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def Wd():
    from rtw_amd import world
    return world


class Passes:
    """rtw_amd.Accumulator over a world on torch's stream, with its own workspace (tail=False: of
    rtw_accum_workspace_bytes only, without the tail dealing's rings)."""

    def __init__(self, rtw, dw, p, pass_spp, tail=True):
        import torch
        self.torch = torch
        self.acc = rtw.Accumulator(dw, p)
        full = self.acc.workspace_bytes(pass_spp)
        self.need = full if tail else rtw.lib().rtw_accum_workspace_bytes(C.byref(p), pass_spp)
        assert tail or self.need < full
        self.ws = torch.empty(self.need + 256, dtype=torch.uint8, device="cuda:0")
        self.ptr = (self.ws.data_ptr() + 255) & ~255
        self.rgb = torch.zeros((p.row_count, p.width, 3), dtype=torch.uint8, device="cuda:0")
        self.mean = torch.zeros((p.row_count, p.width, 3), dtype=torch.float32, device="cuda:0")

    def run(self, cam, n, poison=False):
        stream = self.torch.cuda.current_stream().cuda_stream
        if poison:
            self.ws.fill_(0xFF)
        self.acc.render_pass(cam, n, self.ptr, self.need, stream)
        self.acc.resolve(self.rgb.data_ptr(), self.mean.data_ptr(), stream)
        self.torch.cuda.synchronize()
        return self.rgb.cpu().numpy(), self.mean.cpu().numpy()


def assert_pixels_equal_their_render(refs, got, counts, what):
    for n in np.unique(counts):
        sel = counts == n
        want = refs[int(n)]
        assert np.array_equal(got[0][sel], want[0][sel]), (what, int(n), int((got[0][sel] != want[0][sel]).sum()))
        assert np.array_equal(u32(got[1])[sel], u32(want[1])[sel]), (what, int(n))


def masks(w, h):
    y, x = np.mgrid[0:h, 0:w]
    checker = (x + y) % 2 == (w - 1 + h - 1) % 2  # (keeps the last pixel: inactive is sticky)
    tx, ty, ctx, cty = x // 8, y // 8, (w - 1) // 8, (h - 1) // 8
    tiles = (tx + ty) % 2 == (ctx + cty) % 2
    tiles &= ~((tx == ctx) & (ty == cty)) | ((x == w - 1) & (y == h - 1))  # the corner tile: its last pixel only
    return checker, tiles


def masked_passes(rtw, Wd, b, w, h, lane):
    cam = b.camera()
    mk = lambda n: rtw.make_params(w, h, n, 50, 42, background=b.background)
    refs = {n: Wd.render_world(cam, b.desc, mk(n), want_mean=True) for n in (20, 40, 60)}  # once, for both runs
    dw = Wd.DeviceWorld(b.desc)
    if lane:
        assert dw.launch_info(mk(20))["traversal"] == "lane"
    checker, tiles = masks(w, h)
    for tail in (True, False):
        ps = Passes(rtw, dw, mk(60), 20, tail)
        active = np.ones((h, w), bool)
        want_cnt = np.zeros((h, w), np.uint32)
        for k in range(3):
            if k:
                m = (checker, tiles)[k - 1]
                ps.acc.set_mask(m)
                active &= m
                assert ps.acc.active()[0] == active.sum()
            before = ps.acc.read()
            got = ps.run(cam, 20, poison=k > 0)
            want_cnt[active] += 20
            cnt = ps.acc.counts()
            assert np.array_equal(cnt, want_cnt), (tail, k)
            s, st = ps.acc.read()
            assert not np.isnan(s).any() and not np.isnan(st).any() and not np.isnan(got[1]).any()
            assert np.array_equal(s[~active], before[0][~active]) and np.array_equal(st[~active], before[1][~active])
            assert_pixels_equal_their_render(refs, got, cnt, (tail, k))
        assert set(np.unique(want_cnt)) == {20, 40, 60} and active[h - 1, w - 1]
        assert active[(h - 1) // 8 * 8:, (w - 1) // 8 * 8:].sum() == 1 and cnt[h - 1, w - 1] == 60  # one live pixel
        ps.acc.close()
    dw.close()


def test_cornell_masked_passes_equal_the_render_per_pixel(rtw, Wd):
    masked_passes(rtw, Wd, Wd.BuiltScene(6, 42), 40, 40, lane=False)


def test_globe_lane_walk_masked_passes_equal_the_render_per_pixel(rtw, Wd):
    masked_passes(rtw, Wd, Wd.BuiltScene(7, 42, image=Wd.synthetic_world_map()), 64, 36, lane=True)


def test_budget_calibrated_on_the_frame_stops_half_the_pixels(rtw, Wd):
    """tol = the median over pixels of the standard error after two chunks: about half the pixels stop there."""
    w, h = 48, 27
    b = Wd.BuiltScene(3, 42)
    cam = b.camera()
    mk = lambda n: rtw.make_params(w, h, n, 50, 42, background=b.background)
    dw = Wd.DeviceWorld(b.desc)
    plain = Passes(rtw, dw, mk(60), 20)
    plain.run(cam, 20)
    plain.run(cam, 20)
    _, st = plain.acc.read()
    se2, _ = luminance_se2(st, np.full((h, w), 40, np.uint32), 20)
    tol = float(np.median(np.sqrt(se2)))
    assert tol > 0
    plain.acc.close()
    ps = Passes(rtw, dw, mk(60), 20)
    ps.acc.set_adaptive(tol)
    for _ in range(3):
        got = ps.run(cam, 20)
    cnt = ps.acc.counts()
    classes = {int(n): int((cnt == n).sum()) for n in np.unique(cnt)}
    print("tol", tol, "classes", classes)
    assert set(classes) == {40, 60} and min(classes.values()) >= w * h // 4
    assert np.array_equal(cnt == 40, se2 <= np.float64(tol) * np.float64(tol))
    refs = {n: Wd.render_world(cam, b.desc, mk(n), want_mean=True) for n in (40, 60)}
    assert_pixels_equal_their_render(refs, got, cnt, "perlin adaptive")
    ps.acc.close()
    dw.close()
