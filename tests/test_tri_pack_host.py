"""Triangles through the host packer, the refit and the rebuild's host twin (tests/native/tri_pack_check.cpp has
the list): built with g++ and no HIP, run clean, run once more against a packer with one line broken (the
triangle's padded box, the feature bit), and once under the address and undefined-behaviour sanitizers.
Worlds without triangles keep their tables: tests/test_pack_host.py's digests, unchanged."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import PKG_ROOT, REPO

CSRC = os.path.join(PKG_ROOT, "csrc")
SRC = os.path.join(REPO, "tests", "native", "tri_pack_check.cpp")
FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off"]
RESULT = r"tri_pack_check: checks (\d+) violations (\d+)"
UNITS = ("rtw_world_pack.cpp", "rtw_world_refit.cpp", "rtw_world_build.cpp")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


def _build(out_dir, src_dir=None, extra=()):
    exe = os.path.join(str(out_dir), "tri_pack_check")
    inc = (["-I", str(src_dir)] if src_dir else []) + ["-I", os.path.join(REPO, "include"), "-I", CSRC]
    units = [os.path.join(str(src_dir) if src_dir else CSRC, u) for u in UNITS]
    return exe, subprocess.run(["g++", *FLAGS, *extra, *inc, SRC, *units, "-o", exe], capture_output=True, text=True)


def _run(exe):
    p = subprocess.run([exe], capture_output=True, text=True)
    m = re.search(RESULT, p.stdout)
    assert m, p.stdout + p.stderr
    print(p.stdout.strip())
    return p.returncode, int(m.group(1)), int(m.group(2)), p.stderr


def test_packed_triangles_match_the_descriptor(tmp_path):
    exe, r = _build(tmp_path)
    assert r.returncode == 0, r.stderr
    rc, checks, viol, err = _run(exe)
    assert rc == 0 and viol == 0, err
    assert checks >= 20000  # the checks did run: every record, every vertex against its leaf box


@pytest.mark.parametrize("name,old,new", [
    ("rtw_world_box.hpp", "b.hi[k] = std::max(std::max(p.a[k], p.a[3 + k]), p.a[6 + k]) + 0.0001;",
     "b.hi[k] = std::max(p.a[k], p.a[3 + k]) + 0.0001;"),
    ("rtw_world_pack.cpp", "      wp.feat |= 64u;\n", ""),
    ("rtw_world_refit.hpp", "  r[9] = n[0], r[10] = n[1], r[12] = n[2], r[13] = h;", "  r[9] = n[0], r[10] = n[1], r[12] = h, r[13] = n[2];")])
def test_tri_pack_check_has_teeth(tmp_path, name, old, new):
    d = tmp_path / "broken"
    d.mkdir()
    for u in os.listdir(CSRC):  # (the headers include each other by name: a copy of every one beside the units)
        if u.endswith(".hpp") or u in UNITS:
            shutil.copy(os.path.join(CSRC, u), d / u)
    src = open(os.path.join(CSRC, name)).read()
    assert src.count(old) == 1
    (d / name).write_text(src.replace(old, new))
    exe, r = _build(d, src_dir=d)
    assert r.returncode == 0, r.stderr
    rc, _, viol, err = _run(exe)
    assert rc == 1 and viol > 0, err


def test_tri_pack_check_clean_under_host_sanitizers(tmp_path):
    exe, r = _build(tmp_path, extra=["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    if r.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|libasan|libubsan", r.stderr):
        pytest.skip("sanitizer runtime not installed")
    assert r.returncode == 0, r.stderr
    rc, _, viol, err = _run(exe)
    assert rc == 0 and viol == 0 and "ERROR: AddressSanitizer" not in err and "runtime error" not in err, err
