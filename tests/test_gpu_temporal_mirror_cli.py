"""rtw_render --frames N --orbit DEG --temporal --temporal-mirror
[--temporal-mirror-steps K]: three accumulated frames at 96x54,
4 spp.  On a scene without metal (scene 2) the option changes no byte; on
scene 1, whose metal spheres it follows, the second frame differs; the option
is deterministic; and without --temporal it is refused."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

FRAMES = ["frame_0000.ppm", "frame_0001.ppm", "frame_0002.ppm"]


def test_cli_temporal_mirror_frames(rtw, tmp_path):
    exe = os.path.join(os.path.dirname(rtw.__file__), "..", "bin", "rtw_render")
    temporal = ["--frames", "3", "--orbit", "2", "--temporal"]
    runs = {"s2": ("2", temporal), "s2_mirror": ("2", temporal + ["--temporal-mirror"]),
            "s1": ("1", temporal), "s1_mirror": ("1", temporal + ["--temporal-mirror"]),
            "s1_mirror_again": ("1", temporal + ["--temporal-mirror"]),
            "s1_steps2": ("1", temporal + ["--temporal-mirror", "--temporal-mirror-steps", "2"]),
            "s1_steps1": ("1", temporal + ["--temporal-mirror", "--temporal-mirror-steps", "1"])}
    out = {}
    for n, (scene, extra) in runs.items():
        d = tmp_path / n
        d.mkdir()
        cmd = [exe, "--scene", scene, "--width", "96", "--spp", "4", "--seed", "11", "--out", str(d / "out.ppm")] + extra
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (n, r.stderr)
        assert sorted(os.listdir(d)) == FRAMES + ["out.ppm"], n
        out[n] = [(d / f).read_bytes() for f in FRAMES]
        assert len(out[n][0]) >= 96 * 54 * 3
    assert out["s2_mirror"] == out["s2"]                              # no metal: the same bytes
    assert out["s1_mirror"][0] == out["s1"][0]                        # frame 0 has no history
    assert out["s1_mirror"][1] != out["s1"][1]                        # the metal spheres reproject from elsewhere
    assert out["s1_mirror"] == out["s1_mirror_again"] == out["s1_steps2"]  # deterministic; 2 steps are the default
    assert out["s1_steps1"][1] != out["s1"][1]
    base = [exe, "--scene", "1", "--width", "96", "--spp", "4"]
    for extra, word in ((["--frames", "3", "--orbit", "2", "--temporal-mirror"], "--temporal-mirror"),
                        (["--frames", "3", "--temporal-mirror-steps", "2"], "--temporal-mirror"),
                        (temporal + ["--temporal-mirror-steps", "2"], "--temporal-mirror-steps needs --temporal-mirror"),
                        (temporal + ["--temporal-mirror", "--temporal-mirror-steps", "0"], "--temporal-mirror-steps"),
                        (temporal + ["--temporal-mirror", "--temporal-mirror-steps", "9"], "--temporal-mirror-steps")):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and word in r.stderr, (extra, r.stderr)
