"""The host rebuild of a dynamic world's tree (csrc/rtw_world_build.cpp and the
per-item functions of csrc/rtw_world_build.hpp, which the rebuild kernels run
too) defines what rtw_world_rebuild leaves in the device tables.
tests/native/rebuild_check.cpp, built with g++ and no HIP, checks it (its header
has the list) on helpers.mixed_bvh_world "large" and "spheres_image", on the
same worlds after update_helpers.displace, and on the three degenerate worlds of
rebuild_helpers (every centre equal; every centre on one line; 300 coincident
pairs).  The program is run once more against a copy of the header whose split
search starts one key too late, and must report violations, and once built with
the address and undefined-behaviour sanitizers, as a plain executable."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import PKG_ROOT, REPO
from helpers import MIXED_SIZES, _to_desc, mixed_bvh_world
from rebuild_helpers import DEGENERATE, degenerate_world
from update_helpers import displace, dump_desc, numbers

CSRC = os.path.join(PKG_ROOT, "csrc")
NATIVE = os.path.join(REPO, "tests", "native")
FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off"]
GEN_SEED = 5
RESULT = r"worlds 5 checks (\d+) violations (\d+)"
SOURCES = ("rtw_world_pack.cpp", "rtw_world_refit.cpp", "rtw_world_build.cpp")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


@pytest.fixture(scope="module")
def W(rtw):
    from rtw_amd import world
    return world


@pytest.fixture(scope="module")
def earth(W):
    return W.earth_map()


@pytest.fixture(scope="module")
def dumps(W, earth, tmp_path_factory):
    """WORLD.bin:MOVED.bin arguments of rebuild_check: the world and the same world with other numbers."""
    d = tmp_path_factory.mktemp("rebuild_worlds")
    args = []

    def dump(name, t0, t1):
        paths = []
        for tag, t in (("", t0), ("_moved", t1)):
            desc, keep = _to_desc(W, *t)
            paths.append(str(d / (name + tag + ".bin")))
            dump_desc(desc, 0, paths[-1])
        args.append(":".join(paths))
    for name, (nb, ns, variant) in (("large", (*MIXED_SIZES["large"], None)), ("spheres_image", (0, 520, "spheres_image"))):
        t0 = mixed_bvh_world(W, earth, nb, ns, GEN_SEED, variant=variant)
        dump(name, t0, displace(t0))
    for kind in DEGENERATE:
        dump(kind, degenerate_world(W, kind), degenerate_world(W, kind, moved=True))
    return args


def _build(out_dir, header_dir=None, extra=()):
    exe = os.path.join(str(out_dir), "rebuild_check")
    inc = (["-I", str(header_dir)] if header_dir else []) + ["-I", os.path.join(REPO, "include"), "-I", CSRC]
    src = str(header_dir) if header_dir else CSRC
    cmd = ["g++", *FLAGS, *extra, *inc, os.path.join(NATIVE, "rebuild_check.cpp"), *(os.path.join(src, s) for s in SOURCES),
           "-o", exe]
    return exe, subprocess.run(cmd, capture_output=True, text=True)


def _run(exe, dumps):
    p = subprocess.run([exe, *dumps], capture_output=True, text=True)
    m = re.search(RESULT, p.stdout)
    assert m, p.stdout + p.stderr
    print(p.stdout.strip())
    return p.returncode, int(m.group(1)), int(m.group(2)), p.stderr


def test_rebuilt_trees_match_the_definition_and_the_descriptor(tmp_path, dumps):
    exe, r = _build(tmp_path)
    assert r.returncode == 0, r.stderr
    rc, checks, viol, err = _run(exe, dumps)
    assert rc == 0 and viol == 0, err
    assert checks >= 100000  # the checks did run: every primitive, node, child and axis


def test_rebuild_check_has_teeth(tmp_path, dumps):
    """A split search that cannot return the first key after b: wrong wherever the bit flips there."""
    src = open(os.path.join(CSRC, "rtw_world_build.hpp")).read()
    line = "  uint32_t lo = b, hi = e - 1u;"
    assert src.count(line) == 1
    d = tmp_path / "broken"
    d.mkdir()
    (d / "rtw_world_build.hpp").write_text(src.replace(line, "  uint32_t lo = b + 1u, hi = e - 1u;"))
    for name in ("rtw_world_pack.hpp", *SOURCES):  # (they include the header by its name)
        shutil.copy(os.path.join(CSRC, name), d / name)
    exe, r = _build(d, header_dir=d)
    assert r.returncode == 0, r.stderr
    p = subprocess.run([exe, *dumps], capture_output=True, text=True)
    m = re.search(RESULT, p.stdout)
    # (the host build asserts its own invariants, so the broken header may stop it before the report)
    assert p.returncode != 0 and (m is None or int(m.group(2)) > 0), p.stdout + p.stderr


def test_rebuild_clean_under_host_sanitizers(tmp_path, dumps):
    exe, r = _build(tmp_path, extra=["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    if r.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|libasan|libubsan", r.stderr):
        pytest.skip("sanitizer runtime not installed")
    assert r.returncode == 0, r.stderr
    rc, _, viol, err = _run(exe, dumps)
    assert rc == 0 and viol == 0 and "ERROR: AddressSanitizer" not in err and "runtime error" not in err, err


def test_c_abi_of_rebuilds(rtw, W):
    syms = rtw.header_symbols()
    for s in ("rtw_world_rebuild", "rtw_world_rebuild_device", "rtw_world_bvh_cost", "rtw_world_rebuild_tables_host",
              "rtw_world_rebuild_refit_tables_host"):
        assert s in syms and hasattr(rtw.lib(), s) and getattr(rtw.lib(), s).argtypes, s
    assert rtw.abi_version() == 4
    for m in ("rebuild", "rebuild_device", "bvh_cost"):
        assert callable(getattr(W.DeviceWorld, m)), m
    from rtw_amd import device
    assert callable(device.rebuild_world) and callable(W.rebuild_tables_host)


def test_rebuild_tables_host_through_python(W, earth):
    """rtw_world_rebuild_tables_host needs no device: a permutation in the order table, the same node count,
    a depth within the per-lane stack, other bytes than the created tables, the same bytes on a second
    call; a world with leaves of two and a non-finite number are refused."""
    flags = W.WORLD_DYNAMIC
    t0 = mixed_bvh_world(W, earth, 0, 520, GEN_SEED, variant="spheres_image")
    desc, keep = _to_desc(W, *t0)
    a1, xv1 = numbers(displace(t0))
    created = W.refit_tables_host(desc, flags, _table_bytes(W, desc, flags))
    n = created["blob"].size
    got = W.rebuild_tables_host(desc, flags, n, a1)
    again = W.rebuild_tables_host(desc, flags, n, a1)
    assert got["info"]["nodes"] == desc.n_prims - 1 and got["info"]["max_leaf"] == 1 and got["info"]["max_depth"] <= 16
    assert (got["blob"] == again["blob"]).all() and (got["blob"] != created["blob"]).sum() > 1000
    then = W.rebuild_tables_host(desc, flags, n, numbers(t0)[0], then_a=a1)
    assert np.array_equal(then["bounds"], got["bounds"]) and np.array_equal(then["cull"], got["cull"])
    bad = a1.copy()
    bad[7, 0] = np.inf
    with pytest.raises(W.RtwError) as e:
        W.rebuild_tables_host(desc, flags, n, bad)
    assert e.value.status == -1  # RTW_EINVAL
    ts = mixed_bvh_world(W, earth, *MIXED_SIZES["small"], GEN_SEED)
    ds, keep_s = _to_desc(W, *ts)
    with pytest.raises(W.RtwError) as e:
        W.rebuild_tables_host(ds, flags, _table_bytes(W, ds, flags), numbers(ts)[0], numbers(ts)[1])
    assert e.value.status == -2  # RTW_UNSUPPORTED


def _table_bytes(W, desc, flags):
    """The size of a world's tables without a device: rtw_world_refit_tables_host names it when asked for the wrong one."""
    try:
        W.refit_tables_host(desc, flags, 1)
    except W.RtwError as e:
        return int(re.search(r"the tables have (\d+)", str(e)).group(1))
    raise AssertionError("a one-byte table")
