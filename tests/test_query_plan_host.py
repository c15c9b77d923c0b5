"""The host side of a ray query (csrc/rtw_query_plan.cpp): argument checks,
the traversal after AUTO and the world's limits, the launch geometry
(n = 0, 1, 63, 64, 65, n no multiple of the workgroup, the n limit).  A
stand-alone program under tests/native/, built with g++ and no HIP
(query_plan_check.cpp has the list); run once more against a copy of the plan
with one line broken, which it must report."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import PKG_ROOT, REPO

CSRC = os.path.join(PKG_ROOT, "csrc")
NATIVE = os.path.join(REPO, "tests", "native")
FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off"]

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


def _build(out_dir, plan_src=None):
    exe = os.path.join(str(out_dir), "query_plan_check")
    cmd = ["g++", *FLAGS, "-I", os.path.join(REPO, "include"), "-I", CSRC,
           os.path.join(NATIVE, "query_plan_check.cpp"), plan_src or os.path.join(CSRC, "rtw_query_plan.cpp"), "-o", exe]
    return exe, subprocess.run(cmd, capture_output=True, text=True)


def _run(exe):
    p = subprocess.run([exe], capture_output=True, text=True)
    m = re.search(r"checks (\d+) violations (\d+)", p.stdout)
    assert m, p.stdout + p.stderr
    return p.returncode, int(m.group(1)), int(m.group(2)), p.stderr


def test_query_plan(tmp_path):
    exe, r = _build(tmp_path)
    assert r.returncode == 0, r.stderr
    rc, checks, viol, err = _run(exe)
    assert rc == 0 and viol == 0, err
    assert checks >= 200  # the checks did run


BROKEN = [
    ("n_limit", "  if (n > RTW_QUERY_MAX_RAYS) {", "  if (n > RTW_QUERY_MAX_RAYS + 1) {"),
    ("grid_rounds_down", "  const uint64_t want = (n + kBlock - 1) / kBlock;", "  const uint64_t want = n / kBlock;"),
    ("lane_where_not_allowed", "  const bool lane = lane_ok && (asked", "  const bool lane = (asked"),
]


@pytest.mark.parametrize("name,line,broken", BROKEN, ids=[b[0] for b in BROKEN])
def test_query_plan_checks_have_teeth(tmp_path, name, line, broken):
    src = open(os.path.join(CSRC, "rtw_query_plan.cpp")).read()
    assert src.count(line) == 1, line
    copy = tmp_path / "rtw_query_plan.cpp"
    copy.write_text(src.replace(line, broken))
    exe, r = _build(tmp_path, plan_src=str(copy))
    assert r.returncode == 0, r.stderr
    rc, _, viol, err = _run(exe)
    assert rc == 1 and viol > 0, (name, err)
