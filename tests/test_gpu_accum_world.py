"""Progressive rendering of general worlds (rtw_accum_world_render_device): the
world kernel's passes fold to the one-shot frame, byte for byte — the Cornell
box (rects, transform chains, a light), the Perlin spheres (noise texture,
the unconstrained register budget) and the globe + 10k spheres under the
per-lane BVH walk — with and without the tail dealing's rings in the
workspace.  Bar against the oracle: test_gpu_parity.assert_parity."""
import pytest

from test_gpu_accum import same_image
from test_gpu_parity import assert_parity

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def Wd():
    from rtw_amd import world
    return world


def accumulate(rtw, dw, cam, p, passes, tail=True):
    """Passes through rtw_amd.Accumulator on torch's stream -> (rgb, mean) after the last.
    tail=False: a workspace of rtw_accum_workspace_bytes only, without the rings."""
    import ctypes as C
    import torch
    acc = rtw.Accumulator(dw, p)
    need = max(acc.workspace_bytes(n) if tail else rtw.lib().rtw_accum_workspace_bytes(C.byref(p), n)
               for n in passes)
    if not tail:
        assert need < max(acc.workspace_bytes(n) for n in passes)
    ws = torch.empty(need + 256, dtype=torch.uint8, device="cuda:0")
    ptr = (ws.data_ptr() + 255) & ~255
    rgb = torch.empty((p.row_count, p.width, 3), dtype=torch.uint8, device="cuda:0")
    mean = torch.empty((p.row_count, p.width, 3), dtype=torch.float32, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    for n in passes:
        acc.render_pass(cam, n, ptr, need, stream)
    assert acc.samples() == sum(passes)
    acc.resolve(rgb.data_ptr(), mean.data_ptr(), stream)
    torch.cuda.synchronize()
    acc.close()
    return rgb.cpu().numpy(), mean.cpu().numpy()


def test_cornell_passes_equal_one_shot_and_oracle(rtw, oracle, Wd):
    b = Wd.BuiltScene(6, 42)
    cam = b.camera()
    p = rtw.make_params(40, 40, 40, 50, 42, background=b.background)
    want = Wd.render_world(cam, b.desc, p, want_mean=True)
    dw = Wd.DeviceWorld(b.desc)
    got = accumulate(rtw, dw, cam, p, [20, 20])
    assert same_image(got, want)
    bare = accumulate(rtw, dw, cam, p, [20, 20], tail=False)  # no rings: no tail dealing, the same bytes
    assert same_image(bare, want)
    dw.close()
    o = oracle.OracleWorld(6, 42)
    ref, _ = o.render_tier_b(o.camera(), 40, 40, 40)
    assert_parity(got[0], ref, "accumulated Cornell box 40x40x40")


def test_perlin_passes_equal_one_shot(rtw, Wd):
    b = Wd.BuiltScene(3, 42)
    cam = b.camera()
    p = rtw.make_params(48, 27, 40, 50, 42, background=b.background)
    want = Wd.render_world(cam, b.desc, p, want_mean=True)
    dw = Wd.DeviceWorld(b.desc)
    assert same_image(accumulate(rtw, dw, cam, p, [20, 20]), want)
    dw.close()


def test_globe_lane_walk_passes_equal_one_shot(rtw, Wd):
    b = Wd.BuiltScene(7, 42, image=Wd.synthetic_world_map())
    cam = b.camera()
    p = rtw.make_params(64, 36, 40, 50, 42, background=b.background)
    want = Wd.render_world(cam, b.desc, p, want_mean=True)
    dw = Wd.DeviceWorld(b.desc)
    q = rtw.make_params(64, 36, 20, 50, 42, background=b.background)  # a pass's launch
    assert dw.launch_info(q)["traversal"] == "lane" and dw.launch_info(p)["traversal"] == "lane"
    assert same_image(accumulate(rtw, dw, cam, p, [20, 20]), want)
    assert same_image(accumulate(rtw, dw, cam, p, [20, 20], tail=False), want)
    dw.close()
    assert want[0].std() > 5
