"""The wavefront engine with three and four queue sets (params.wf_sets).  Its
host driver (csrc/rtw_wavefront_host.hip) indexes the poll words, the events,
the side streams and the workspace's regions by set number; the other GPU
tests run one or two sets.  Same bar as test_gpu_wavefront.py: every byte of
rgb and every bit of the linear mean equal the megakernel's render of the same
params, and the counting pass sees every sample.

wf_paths 64: each of four sets holds one segment of 16 paths (heavy slot
recycling); 4096: several segments per set.  96x54 at 3 spp and 40x23 at 9 spp
in chunks of 4 are the smallest frames with partial tiles and with more than
one chunk."""
import numpy as np
import pytest
import torch

from helpers import diff_stats
from test_gpu_parity import ASPECT

pytestmark = pytest.mark.gpu

FRAMES = {"96x54x3": dict(width=96, height=54, spp=3), "40x23x9c4": dict(width=40, height=23, spp=9, chunk=4)}


@pytest.fixture(scope="module")
def cover(rtw):
    sph, mats, _ = rtw.cover_scene(42)
    return sph, mats, rtw.cover_camera(ASPECT)


@pytest.fixture(scope="module")
def megakernel(rtw, cover):
    """(rgb, mean) of the megakernel per (precision, frame), rendered once."""
    sph, mats, cam = cover
    return {(prec, f): rtw.render(cam, sph, mats, rtw.make_params(precision=prec, **kw), want_mean=True)
            for prec in ("f64", "f32") for f, kw in FRAMES.items()}


def check(rtw, cover, megakernel, precision, frame, **wf):
    sph, mats, cam = cover
    p = rtw.make_params(precision=precision, engine="wavefront", **wf, **FRAMES[frame])
    rgb, mean = rtw.render(cam, sph, mats, p, want_mean=True)
    want_rgb, want_mean = megakernel[(precision, frame)]
    assert (rgb == want_rgb).all(), (wf, diff_stats(rgb, want_rgb))
    assert np.array_equal(mean.view(np.uint32), want_mean.view(np.uint32)), wf
    scene = rtw.DeviceScene(sph, mats)
    try:
        need = rtw.workspace_bytes(p)
        ws = torch.empty(need + 256, dtype=torch.uint8, device="cuda:0")
        counts = scene.counts(cam, p, (ws.data_ptr() + 255) & ~255, need)
    finally:
        scene.close()
    assert counts["samples"] == p.width * p.height * p.spp, (wf, counts)


@pytest.mark.parametrize("frame", list(FRAMES))
@pytest.mark.parametrize("paths", [64, 4096])
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("sets", [3, 4])
def test_three_and_four_sets_equal_the_megakernel(rtw, cover, megakernel, sets, precision, paths, frame):
    check(rtw, cover, megakernel, precision, frame, wf_sets=sets, wf_paths=paths)


@pytest.mark.parametrize("cfg", [dict(wf_form="split"), dict(wf_drain="none")], ids=["split", "drain_none"])
def test_four_sets_split_form_and_no_drain(rtw, cover, megakernel, cfg):
    check(rtw, cover, megakernel, "f64", "40x23x9c4", wf_sets=4, wf_paths=4096, **cfg)
