"""rtw_render --frames N --orbit DEG --temporal --temporal-clamp G
[--temporal-clamp-radius R]: three accumulated frames of a small
Cornell box; the clamp changes frames 1 and 2 and leaves frame 0 alone (it has no
history); G = 0 is the default gamma; without the option the frames' bytes are
what the same command gives without it, twice; and the refusals."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

FRAMES = ["frame_0000.ppm", "frame_0001.ppm", "frame_0002.ppm"]


def test_cli_temporal_clamp_frames(rtw, tmp_path):
    exe = os.path.join(os.path.dirname(rtw.__file__), "..", "bin", "rtw_render")
    base = [exe, "--scene", "6", "--width", "40", "--spp", "20", "--seed", "11"]
    temporal = ["--frames", "3", "--orbit", "5", "--temporal"]
    runs = {"temporal": temporal, "again": temporal,
            "clamped": temporal + ["--temporal-clamp", "1"], "clamped_again": temporal + ["--temporal-clamp", "1"],
            "default": temporal + ["--temporal-clamp", "0"], "half": temporal + ["--temporal-clamp", "0.5"],
            "wide": temporal + ["--temporal-clamp", "0.5", "--temporal-clamp-radius", "3"],
            "denoised": temporal + ["--temporal-clamp", "1", "--denoise", "--denoise-spatial"]}
    out = {}
    for n, extra in runs.items():
        d = tmp_path / n
        d.mkdir()
        r = subprocess.run(base + ["--out", str(d / "out.ppm")] + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (n, r.stderr)
        assert sorted(os.listdir(d)) == FRAMES + ["out.ppm"], n
        out[n] = [(d / f).read_bytes() for f in FRAMES]
    t, c = out["temporal"], out["clamped"]
    assert t == out["again"]                                    # without the option: the same bytes, twice
    assert c == out["clamped_again"]                            # deterministic
    assert c[0] == t[0] and c[1] != t[1] and c[2] != t[2]       # frame 0 has no history to clamp
    assert out["default"] == out["half"] and out["default"][1] != c[1]  # G = 0: the default gamma, 0.5
    assert out["wide"][0] == t[0] and out["wide"][1] != c[1] and out["wide"][1] != t[1]
    assert len(out["denoised"][1]) == len(c[1]) and out["denoised"][1] != c[1]
    for extra, word in ((["--frames", "3", "--temporal-clamp", "1"], "--temporal-clamp"),
                        (["--frames", "3", "--temporal-clamp-radius", "2"], "--temporal-clamp"),
                        (temporal + ["--temporal-clamp-radius", "2"], "--temporal-clamp-radius needs --temporal-clamp"),
                        (temporal + ["--temporal-clamp", "-1"], "--temporal-clamp"),
                        (temporal + ["--temporal-clamp", "nan"], "--temporal-clamp"),
                        (temporal + ["--temporal-clamp", "1", "--temporal-clamp-radius", "4"], "--temporal-clamp-radius"),
                        (temporal + ["--temporal-clamp", "1", "--temporal-clamp-radius", "0"], "--temporal-clamp-radius")):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and word in r.stderr, (extra, r.stderr)
