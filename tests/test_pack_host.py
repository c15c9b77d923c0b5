"""The host packers (csrc/rtw_scene_pack.cpp, csrc/rtw_world_pack.cpp) build
the device tables every kernel reads.  Stand-alone programs under
tests/native/, built with g++ and no HIP, check those tables against the
inputs they were made from (scene_pack_check.cpp, world_pack_check.cpp have
the lists); the BVH-free blobs must also be, byte for byte, the ones the parent
commit uploaded (tests/golden/pack_digests.json).  Each program is run once
more against a copy of its packer with one line broken, and must report
violations, and once built with the address and undefined-behaviour
sanitizers."""
import hashlib
import json
import os
import re
import shutil
import subprocess

import pytest

from conftest import GOLDEN, PKG_ROOT, REPO

CSRC = os.path.join(PKG_ROOT, "csrc")
NATIVE = os.path.join(REPO, "tests", "native")
FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off"]
PROGRAMS = {"scene": ("scene_pack_check.cpp", "rtw_scene_pack.cpp", r"scenes 7 checks (\d+) violations (\d+)"),
            "world": ("world_pack_check.cpp", "rtw_world_pack.cpp", r"worlds 5 checks (\d+) violations (\d+)")}

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


@pytest.fixture(scope="module")
def host_objs(tmp_path_factory):
    """The library's HIP-free host sources (rtw_cover_scene, rtw_build_scene), compiled once."""
    d = tmp_path_factory.mktemp("host")
    objs = []
    for name in ("rtw_host", "rtw_world_host"):
        objs.append(str(d / (name + ".o")))
        subprocess.run(["g++", *FLAGS, "-I", os.path.join(REPO, "include"), "-I", CSRC, "-c",
                        os.path.join(CSRC, name + ".cpp"), "-o", objs[-1]], check=True)
    return objs


def _build(which, out_dir, host_objs, pack_src=None, extra=()):
    """The check program of `which`, built with the packer (or the copy `pack_src`)."""
    check, pack, _ = PROGRAMS[which]
    exe = os.path.join(str(out_dir), which + "_pack_check")
    cmd = ["g++", *FLAGS, *extra, "-I", os.path.join(REPO, "include"), "-I", CSRC, "-I", NATIVE,
           os.path.join(NATIVE, check), pack_src or os.path.join(CSRC, pack), *host_objs, "-o", exe]
    return exe, subprocess.run(cmd, capture_output=True, text=True)


def _run(which, exe, *args):
    p = subprocess.run([exe, *args], capture_output=True, text=True)
    m = re.search(PROGRAMS[which][2], p.stdout)
    assert m, p.stdout + p.stderr
    print(p.stdout.strip())
    return p.returncode, int(m.group(1)), int(m.group(2)), p.stderr


@pytest.fixture(scope="module")
def programs(tmp_path_factory, host_objs):
    d = tmp_path_factory.mktemp("pack")
    out = {}
    for which in PROGRAMS:
        exe, r = _build(which, d, host_objs)
        assert r.returncode == 0, r.stderr
        out[which] = exe
    return out


@pytest.mark.parametrize("which,min_checks", [("scene", 5000), ("world", 100000)])
def test_tables_match_their_inputs(programs, tmp_path, which, min_checks):
    rc, checks, viol, err = _run(which, programs[which], str(tmp_path))
    assert rc == 0 and viol == 0, err
    assert checks >= min_checks  # the checks did run: every sphere, slot, node and leaf
    # the BVH-free blobs are the parent commit's, byte for byte
    want = json.load(open(os.path.join(GOLDEN, "pack_digests.json")))["sha256"]
    names = ("cover42", "gen101") if which == "scene" else ("world6", "world1_linear")
    for name in names:
        blob = open(os.path.join(str(tmp_path), name + ".blob"), "rb").read()
        assert hashlib.sha256(blob).hexdigest() == want[name], name


# One line of the packer broken per copy: (program, name, the line, its replacement).
BROKEN = [
    # cvalid: bit 31 - r of a word is slot r; broken: bit r
    ("scene", "cvalid_shift", "|= 0x80000000u >> (sl & 31u);", "|= 1u << (sl & 31u);"),
    # the static half of a mixed pair takes its partner's time group; broken: keeps group 0
    ("scene", "mixed_pair_group", "if (!m0 && m1) cull_tg[j / 2] = (cull_tg[j / 2] & 0xFF00u) | (cull_tg[j / 2] >> 8);",
     "if (false) cull_tg[j / 2] = 0;"),
    # pack_refs moves a lower bound DOWN to the float with the payload byte; broken: to the nearest above as well
    ("world", "lower_bound_rounding", "    if (c > b) c -= 256u;", "    if (false) c -= 256u;"),
]


@pytest.mark.parametrize("which,name,line,broken", BROKEN, ids=[b[1] for b in BROKEN])
def test_checks_have_teeth(tmp_path, host_objs, which, name, line, broken):
    src = open(os.path.join(CSRC, PROGRAMS[which][1])).read()
    assert src.count(line) == 1, line
    copy = tmp_path / PROGRAMS[which][1]
    copy.write_text(src.replace(line, broken))
    exe, r = _build(which, tmp_path, host_objs, pack_src=str(copy))
    assert r.returncode == 0, r.stderr
    rc, _, viol, err = _run(which, exe)
    assert rc == 1 and viol > 0, (name, err)


@pytest.mark.parametrize("which", ["scene", "world"])
def test_packers_clean_under_host_sanitizers(tmp_path, host_objs, which):
    """The same programs (stand-alone executables), packer and checks built
    with ASan and UBSan: no report, no violation."""
    exe, r = _build(which, tmp_path, host_objs,
                    extra=["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    if r.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|libasan|libubsan", r.stderr):
        pytest.skip("sanitizer runtime not installed")
    assert r.returncode == 0, r.stderr
    rc, _, viol, err = _run(which, exe)
    assert rc == 0 and viol == 0 and "ERROR: AddressSanitizer" not in err and "runtime error" not in err, err
