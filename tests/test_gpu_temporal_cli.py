"""rtw_render --frames N --orbit DEG --temporal: three accumulated
frames of a small Cornell box; frame 0 is the plain one-shot frame of the seed;
the same command twice gives the same bytes; without --temporal the command
gives the bytes it gave before (frame 0 the plain frame, and --frames with
--denoise still refused); --temporal with --denoise writes its frames too."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

FRAMES = ["frame_0000.ppm", "frame_0001.ppm", "frame_0002.ppm"]


def test_cli_temporal_frames(rtw, tmp_path):
    exe = os.path.join(os.path.dirname(rtw.__file__), "..", "bin", "rtw_render")
    base = [exe, "--scene", "6", "--width", "40", "--spp", "20", "--seed", "11"]
    orbit = ["--frames", "3", "--orbit", "5"]
    runs = {"plain": [], "orbit": orbit, "temporal": orbit + ["--temporal"], "again": orbit + ["--temporal"],
            "denoised": orbit + ["--temporal", "--temporal-history", "8", "--denoise", "--denoise-spatial"]}
    dirs = {}
    for n, extra in runs.items():
        dirs[n] = tmp_path / n
        dirs[n].mkdir()
        r = subprocess.run(base + ["--out", str(dirs[n] / "out.ppm")] + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (n, r.stderr)
    plain = (dirs["plain"] / "out.ppm").read_bytes()
    for n in ("orbit", "temporal", "again", "denoised"):
        assert sorted(os.listdir(dirs[n])) == FRAMES + ["out.ppm"], n
        assert (dirs[n] / "frame_0002.ppm").read_bytes() == (dirs[n] / "out.ppm").read_bytes()
    t = [(dirs["temporal"] / f).read_bytes() for f in FRAMES]
    assert t[0] == plain                                                   # frame 0: the plain frame of the seed
    assert t == [(dirs["again"] / f).read_bytes() for f in FRAMES]         # deterministic
    o = [(dirs["orbit"] / f).read_bytes() for f in FRAMES]
    assert o[0] == plain and len(set(o)) == 3                              # without the flag: as before
    assert t[1] != o[1] and t[2] != o[2] and len(set(t)) == 3              # the accumulation did something
    dn = [(dirs["denoised"] / f).read_bytes() for f in FRAMES]
    assert len(dn[0]) == len(plain) and dn[1] != t[1]
    for extra, word in ((["--temporal"], "--temporal"), (["--frames", "3", "--denoise"], "--frames"),
                        (["--temporal-history", "4"], "--temporal-history"),
                        (orbit + ["--temporal", "--pass-spp", "10"], "--temporal")):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and word in r.stderr, (extra, r.stderr)
