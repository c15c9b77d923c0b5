"""The self-skip rule of the f64 megakernel (csrc/rtw_selfskip.hpp) on the CPU:
rtws::leaves never fires where the reference's literal f64 sphere test (oracle/tierb_core.h `test`,
restated in tests/native/selfskip_check.cpp) accepts the sphere, on more than 10^7 adversarial rays that
start on a sphere the way the kernel makes them; it does fire on the leaving rays of cover-like scenes;
and the check has teeth: with the condition's constant loosened tenfold it reports violations.  No GPU."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "raytracinginoneweekend.zig_amd", "csrc")
SRC = os.path.join(REPO, "tests", "native", "selfskip_check.cpp")
RESULT = r"selfskip_check: cases (\d+) fired (\d+) violations (\d+) cover_leaving (\d+) cover_fired (\d+)"

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


def _build(tmp_path, name, extra=()):
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", *extra, "-I", CSRC, SRC, "-o", exe], check=True)
    return exe


def _run(exe, n, seed):
    p = subprocess.run([exe, str(n), str(seed)], capture_output=True, text=True)
    m = re.search(RESULT, p.stdout)
    assert m, p.stdout + p.stderr
    print(p.stdout.strip()[-600:])
    return (p.returncode, *map(int, m.groups()))


@needs_gxx
def test_rule_never_fires_where_the_literal_test_accepts(tmp_path):
    exe = _build(tmp_path, "sschk")
    total = 0
    for seed, n in ((1, 8_000_000), (2, 4_000_000)):
        rc, cases, fired, viol, leaving, cover_fired = _run(exe, n, seed)
        assert viol == 0 and rc == 0
        assert cases >= n and fired > cases // 4  # the rule does fire on the adversarial mix as well
        # a rule that never fired would pass the line above it: >= 80 % of the cover-like leaving rays
        assert leaving > cases // 8 and cover_fired >= 0.8 * leaving
        total += cases
    assert total >= 10_000_000


@needs_gxx
def test_check_detects_a_tenfold_looser_constant(tmp_path):
    """cc > -10 tmin hb lets the exact second root reach 2.3 tmin (hb = a tmin): the literal test accepts."""
    exe = _build(tmp_path, "sschk10", extra=["-DRTW_SELFSKIP_CC_SCALE=10.0"])
    rc, cases, fired, viol, _, _ = _run(exe, 3_000_000, 1)
    assert viol > 0 and rc == 1


@needs_gxx
def test_check_clean_under_host_sanitizers(tmp_path):
    try:
        exe = _build(tmp_path, "sschk_san", extra=["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    except subprocess.CalledProcessError:
        pytest.skip("sanitizer runtime not installed")
    rc, cases, fired, viol, _, _ = _run(exe, 300_000, 3)
    assert rc == 0 and viol == 0
