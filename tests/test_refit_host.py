"""The host refit of a dynamic world (csrc/rtw_world_refit.cpp and the per-item
steps of csrc/rtw_world_refit.hpp, which the update kernels run too) defines
what rtw_world_update leaves in the device tables.  tests/native/refit_check.cpp,
built with g++ and no HIP, checks it against the packer and the descriptor (its
header has the list) on the mixed worlds of helpers.mixed_bvh_world — "small":
leaves of <= 2, "large": leaves of 1, packed refs, the depth-capped rebuild,
more than 256 nodes — and on scene 7 cut to 600 spheres.  The program is run
once more against a copy of the header whose unions read the PACKED bounds, and
must report violations, and once built with the address and undefined-behaviour
sanitizers.  On the oracle alone: the updated mixed worlds the GPU tests render
(update_helpers.displace) keep the camera outside every sphere and still show
every class of helpers.MIXED_CLASSES."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import PKG_ROOT, REPO
from helpers import MIXED_CAMERA, MIXED_CLASSES, MIXED_SIZES, _to_desc, mixed_bvh_world
from update_helpers import camera_outside_spheres, displace, dump_desc, numbers, truncated

CSRC = os.path.join(PKG_ROOT, "csrc")
NATIVE = os.path.join(REPO, "tests", "native")
FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off"]
GEN_SEED = 5  # mixed_bvh_world's seed (as tests/test_world_cpu.py)
RESULT = r"worlds 3 checks (\d+) violations (\d+)"

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
    d = tmp_path_factory.mktemp("refit_worlds")
    paths = []
    for size in ("small", "large"):
        desc, keep = _to_desc(W, *mixed_bvh_world(W, earth, *MIXED_SIZES[size], GEN_SEED))
        paths.append(str(d / (size + ".bin")))
        dump_desc(desc, 0, paths[-1])
    b = W.BuiltScene(7, 42, image=earth)
    paths.append(str(d / "globe600.bin"))
    dump_desc(truncated(W, b.desc, 600), 0, paths[-1])
    return paths


def _build(out_dir, header_dir=None, extra=()):
    exe = os.path.join(str(out_dir), "refit_check")
    inc = (["-I", str(header_dir)] if header_dir else []) + ["-I", os.path.join(REPO, "include"), "-I", CSRC]
    src = str(header_dir) if header_dir else CSRC
    cmd = ["g++", *FLAGS, *extra, *inc, os.path.join(NATIVE, "refit_check.cpp"), os.path.join(src, "rtw_world_pack.cpp"),
           os.path.join(src, "rtw_world_refit.cpp"), "-o", exe]
    return exe, subprocess.run(cmd, capture_output=True, text=True)


def _run(exe, dumps):
    p = subprocess.run([exe, *dumps], capture_output=True, text=True)
    m = re.search(RESULT, p.stdout)
    assert m, p.stdout + p.stderr
    print(p.stdout.strip())
    return p.returncode, int(m.group(1)), int(m.group(2)), p.stderr


def test_refit_tables_match_the_packer_and_the_descriptor(tmp_path, dumps):
    exe, r = _build(tmp_path)
    assert r.returncode == 0, r.stderr
    rc, checks, viol, err = _run(exe, dumps)
    assert rc == 0 and viol == 0, err
    assert checks >= 100000  # the checks did run: every primitive, node, child and axis


def test_refit_check_has_teeth(tmp_path, dumps):
    """Unions taken from the packed bounds, whose <= 512-ulp downward shifts would compound level by level."""
    src = open(os.path.join(CSRC, "rtw_world_refit.hpp")).read()
    line = "      const float* q = V.plain + (size_t)12 * ref;"
    assert src.count(line) == 1
    d = tmp_path / "broken"
    d.mkdir()
    (d / "rtw_world_refit.hpp").write_text(src.replace(line, "      const float* q = V.node + (size_t)rtwk::kNodeWords * ref;"))
    for name in ("rtw_world_pack.hpp", "rtw_world_pack.cpp", "rtw_world_refit.cpp"):  # (they include the header by its name)
        shutil.copy(os.path.join(CSRC, name), d / name)
    exe, r = _build(d, header_dir=d)
    assert r.returncode == 0, r.stderr
    rc, _, viol, err = _run(exe, dumps)
    assert rc == 1 and viol > 0, err


def test_refit_clean_under_host_sanitizers(tmp_path, dumps):
    exe, r = _build(tmp_path, extra=["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    if r.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|libasan|libubsan", r.stderr):
        pytest.skip("sanitizer runtime not installed")
    assert r.returncode == 0, r.stderr
    rc, _, viol, err = _run(exe, dumps)
    assert rc == 0 and viol == 0 and "ERROR: AddressSanitizer" not in err and "runtime error" not in err, err


def test_c_abi_of_dynamic_worlds(rtw, W):
    syms = rtw.header_symbols()
    for s in ("rtw_world_update", "rtw_world_update_device", "rtw_world_table_bytes", "rtw_world_read_tables",
              "rtw_world_refit_tables_host"):
        assert s in syms and hasattr(rtw.lib(), s) and getattr(rtw.lib(), s).argtypes, s
    assert "#define RTW_WORLD_DYNAMIC 4u" in open(os.path.join(REPO, "include", "rtw_hip.h")).read()
    assert W.WORLD_DYNAMIC == 4 and rtw.abi_version() == 4
    for m in ("update", "update_device", "read_tables", "table_bytes"):
        assert callable(getattr(W.DeviceWorld, m)), m
    from rtw_amd import device
    assert callable(device.update_world) and callable(W.refit_tables_host)


# ---- the inputs of tests/test_gpu_world_update.py, on the oracle alone ----
MIXED_BG = (0.7, 0.8, 1.0)


@pytest.mark.parametrize("size", ["small", "large"])
def test_updated_mixed_worlds_stay_in_the_input_domain_and_show_every_class(W, oracle, earth, size):
    """The displaced worlds: the camera outside every sphere; the numbers did move (every sphere by
    >= 3 radii); and, as test_world_cpu.py shows for the originals, removing any one class changes
    >= 2 % of the oracle's 96x54x4 frame."""
    import numpy as np

    from test_world_cpu import _mixed_oracle_camera
    t0 = mixed_bvh_world(W, earth, *MIXED_SIZES[size], GEN_SEED)
    t1 = displace(t0)
    assert camera_outside_spheres(t1, MIXED_CAMERA["look_from"])
    a0, xv0 = numbers(t0)
    a1, xv1 = numbers(t1)
    sph = np.array([p["kind"] <= 1 for p in t0[0]])
    move = np.linalg.norm(a1[sph, 0:3] - a0[sph, 0:3], axis=1) / np.abs(a0[sph, 6])
    assert move.min() >= 3.0 - 1e-9 and move.max() <= 10.0 + 1e-9, (move.min(), move.max())
    assert (xv1 != xv0).any(axis=(1, 2)).all()
    assert [(p["kind"], p["mat"], p["xform"]) for p in t0[0]] == [(p["kind"], p["mat"], p["xform"]) for p in t1[0]]
    cam = _mixed_oracle_camera(oracle)

    def render(drop=()):
        t = ([p for p in t1[0] if p["cls"] not in drop],) + tuple(t1[1:])
        return oracle.TableWorld(*t, background=MIXED_BG).render_tier_b(cam, 96, 54, 4, bg=MIXED_BG, threads=8)[0], len(t[0])
    full, n = render()
    for cls in MIXED_CLASSES:
        img, nd = render((cls,))
        assert nd < n
        frac = float((img != full).any(axis=2).mean())
        print(size, cls, "changed pixels", frac)
        assert frac >= 0.02, (size, cls, frac)
