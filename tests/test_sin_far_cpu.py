"""rtwl::sin_far (rtw_libm.hpp): the sin the device's kernels use for 2^20 pi/2 <= |x| < 2^32 — a noise
texture at a point a surface query's caller made up — is rounded to nearest.  A host build of the same
text is held against tests/golden/sin_far.f64 (5,009 arguments and their correctly rounded sines,
tests/native/sin_far_check.cpp says which); the gfx950 build is held against the oracle by
tests/test_gpu_surface.py::test_out_of_range_uv_and_far_points."""
import os
import re
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sin_far_is_rounded_to_nearest(tmp_path):
    exe = str(tmp_path / "sinfar")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-I",
                    os.path.join(REPO, "raytracinginoneweekend.zig_amd", "csrc"),
                    os.path.join(REPO, "tests", "native", "sin_far_check.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe, os.path.join(REPO, "tests", "golden", "sin_far.f64")], capture_output=True, text=True)
    print(p.stdout)
    assert p.returncode == 0, p.stdout + p.stderr
    m = re.search(r"cases (\d+) mismatches (\d+)", p.stdout)
    assert m and int(m.group(1)) == 5009 and int(m.group(2)) == 0, p.stdout
