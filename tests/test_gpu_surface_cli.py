"""rtw_render --aov-dir DIR: the two images of a frame's guides.  Scene 6 at
40x40: albedo.ppm and normal.ppm are rtw_world_guides_device's buffer of that frame quantised in
numpy by the rules rtw_main.cpp states (albedo as a render quantises a linear colour, normal as
0.5 (n + 1) through the same quantiser without the gamma); --frames 3 --orbit 5 --temporal
writes one pair per frame, the first the single frame's; without the option no file appears
and the rendered bytes are what they are with it."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W_ = H_ = 40


def read_ppm(path):
    data = open(path, "rb").read()
    magic, size, maxv, body = data.split(b"\n", 3)
    w, h = (int(x) for x in size.split())
    assert magic == b"P6" and maxv == b"255" and len(body) == w * h * 3, path
    return np.frombuffer(body, np.uint8).reshape(h, w, 3)


def quantise_unit(x):
    """(uint8)(256 * max(0, min(x, 0.999))) in f64."""
    return (256.0 * np.maximum(0.0, np.minimum(x, 0.999))).astype(np.uint8)


def test_cli_aov_images(rtw, tmp_path):
    import torch
    from rtw_amd import world as W
    exe = os.path.join(os.path.dirname(rtw.__file__), "..", "bin", "rtw_render")
    base = [exe, "--scene", "6", "--width", str(W_), "--spp", "20", "--seed", "11"]
    orbit = ["--frames", "3", "--orbit", "5", "--temporal"]
    runs = {"plain": [], "aov": ["--aov-dir", "AOV"], "frames": orbit, "frames_aov": orbit + ["--aov-dir", "AOV"]}
    dirs = {}
    for n, extra in runs.items():
        dirs[n] = tmp_path / n
        dirs[n].mkdir()
        extra = [str(dirs[n] / "aov") if x == "AOV" else x for x in extra]
        r = subprocess.run(base + ["--out", str(dirs[n] / "out.ppm")] + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (n, r.stderr)
    frames = [f"frame_{k:04d}.ppm" for k in range(3)]
    # without the option: no file appears; with it: the same rendered bytes, and the pairs
    assert sorted(os.listdir(dirs["plain"])) == ["out.ppm"]
    assert sorted(os.listdir(dirs["frames"])) == frames + ["out.ppm"]
    assert sorted(os.listdir(dirs["aov"])) == ["aov", "out.ppm"]
    assert sorted(os.listdir(dirs["aov"] / "aov")) == ["albedo.ppm", "normal.ppm"]
    assert sorted(os.listdir(dirs["frames_aov"])) == ["aov"] + frames + ["out.ppm"]
    assert sorted(os.listdir(dirs["frames_aov"] / "aov")) == [f"{a}_{k:04d}.ppm" for a in ("albedo", "normal") for k in range(3)]
    assert (dirs["aov"] / "out.ppm").read_bytes() == (dirs["plain"] / "out.ppm").read_bytes()
    for f in frames + ["out.ppm"]:
        assert (dirs["frames_aov"] / f).read_bytes() == (dirs["frames"] / f).read_bytes(), f
    # the two images: the frame's guides, quantised by the stated rules
    built = W.BuiltScene(6, 42, None)
    assert (built.settings.width, built.settings.height) == (600, 600)  # aspect 1: --width 40 is a 40x40 frame
    cam = built.camera(1.0)
    dw = W.DeviceWorld(built.desc)
    try:
        g = torch.empty((H_, W_, 32), dtype=torch.uint8, device="cuda:0")
        dw.guides(cam, rtw.make_params(W_, H_, 1, background=built.background), g.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    finally:
        dw.close()
    guides = g.cpu().numpy().view(rtw.GUIDE_DTYPE)[..., 0]
    assert (guides["prim"] > 0).sum() > W_ * H_ // 2 and (guides["prim"] == 0).any()
    albedo = quantise_unit(np.sqrt(guides["albedo"].astype(np.float64)))
    normal = quantise_unit(0.5 * (guides["normal"].astype(np.float64) + 1.0))
    assert len(np.unique(albedo.reshape(-1, 3), axis=0)) >= 4 and len(np.unique(normal.reshape(-1, 3), axis=0)) >= 5
    assert (albedo == 255).any()  # the light: a linear value above 1 ends at the quantiser's top
    assert (normal[guides["prim"] == 0] == 128).all()  # a miss: 0.5 (0 + 1)
    for d, suffix in ((dirs["aov"] / "aov", ""), (dirs["frames_aov"] / "aov", "_0000")):
        assert np.array_equal(read_ppm(d / f"albedo{suffix}.ppm"), albedo), suffix
        assert np.array_equal(read_ppm(d / f"normal{suffix}.ppm"), normal), suffix
    pairs = [(read_ppm(dirs["frames_aov"] / "aov" / f"albedo_{k:04d}.ppm"), read_ppm(dirs["frames_aov"] / "aov" / f"normal_{k:04d}.ppm"))
             for k in range(3)]
    assert not np.array_equal(pairs[0][1], pairs[1][1]) and not np.array_equal(pairs[1][1], pairs[2][1])  # the boxes turn
