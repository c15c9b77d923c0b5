"""The render plan (csrc/rtw_plan.cpp): validation of rtw_params, the unit
arithmetic and the layout of every device allocation the C ABI carves up.  A
stand-alone program under tests/native/, built with g++ and no HIP, checks the
layouts against their descriptions over a grid of params (plan_check.cpp has
the list).  It is run once more against two copies of the plan with one line
broken each, and must report violations, and once built with the address and
undefined-behaviour sanitizers."""
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


def _build(out_dir, plan_src=None, extra=()):
    """The check program, built with the plan (or the copy `plan_src`)."""
    exe = os.path.join(str(out_dir), "plan_check")
    cmd = ["g++", *FLAGS, *extra, "-I", os.path.join(REPO, "include"), "-I", CSRC,
           os.path.join(NATIVE, "plan_check.cpp"), plan_src or os.path.join(CSRC, "rtw_plan.cpp"), "-o", exe]
    return exe, subprocess.run(cmd, capture_output=True, text=True)


def _run(exe):
    p = subprocess.run([exe], capture_output=True, text=True)
    m = re.search(r"plans 7500 checks (\d+) violations (\d+)", p.stdout)
    assert m, p.stdout + p.stderr
    print(p.stdout.strip())
    return p.returncode, int(m.group(1)), int(m.group(2)), p.stderr


def test_layouts_match_their_descriptions(tmp_path):
    exe, r = _build(tmp_path)
    assert r.returncode == 0, r.stderr
    rc, checks, viol, err = _run(exe)
    assert rc == 0 and viol == 0, err
    assert checks >= 850000  # (942,520 when written) the checks did run: every plan, region and rejection


# One line of the plan broken per copy: (name, the line, its replacement).
BROKEN = [
    # region 31 of a queue set (seg_a, the first whose size is no multiple of 256) loses its al256
    ("region_alignment", "  bytes += al256(elems * elem_size);",
     "  bytes += n == 31 ? elems * elem_size : al256(elems * elem_size);"),
    # a queue without its hk array: 13 regions for PathBuf's 14 members
    ("queue_without_hk", "    g.put(n, 4);  // hk\n", ""),
]


@pytest.mark.parametrize("name,line,broken", BROKEN, ids=[b[0] for b in BROKEN])
def test_checks_have_teeth(tmp_path, name, line, broken):
    src = open(os.path.join(CSRC, "rtw_plan.cpp")).read()
    assert src.count(line) == 1, line
    copy = tmp_path / "rtw_plan.cpp"
    copy.write_text(src.replace(line, broken))
    exe, r = _build(tmp_path, plan_src=str(copy))
    assert r.returncode == 0, r.stderr
    rc, _, viol, err = _run(exe)
    assert rc == 1 and viol > 0, (name, err)


def test_plan_clean_under_host_sanitizers(tmp_path):
    """The same program (a stand-alone executable), plan and checks built with
    ASan and UBSan: no report, no violation."""
    exe, r = _build(tmp_path, extra=["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    if r.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|libasan|libubsan", r.stderr):
        pytest.skip("sanitizer runtime not installed")
    assert r.returncode == 0, r.stderr
    rc, _, viol, err = _run(exe)
    assert rc == 0 and viol == 0 and "ERROR: AddressSanitizer" not in err and "runtime error" not in err, err
