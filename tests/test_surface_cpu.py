"""Surface queries without a GPU (rtw_hip.h "surface queries"): the layout of
rtw_surface as a C compiler sees it against the ctypes struct and SURFACE_DTYPE; the three
entries declared, exported and bound with the declared number of arguments; null arguments
refused before anything touches a device; the argument check of csrc/rtw_surface.hpp as a plain
program (tests/native/surface_check.cpp), once more under the host sanitizers; and, on the oracle
alone, that the frames of tests/test_gpu_surface.py hold every class of record they are there
for, so the GPU tests cannot pass vacuously."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import PKG_ROOT, REPO

CSRC = os.path.join(PKG_ROOT, "csrc")
INCLUDE = os.path.join(REPO, "include")
SYMBOLS = {"rtw_world_surface_device": 7, "rtw_scene_surface_device": 7, "rtw_world_surface": 4}
FIELDS = ["value", "fuzz", "ir", "kind", "mat", "tex", "tex_kind", "reserved"]

needs_cc = pytest.mark.skipif(shutil.which("cc") is None, reason="cc not available")
needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


@needs_cc
def test_layout_of_rtw_surface(rtw, tmp_path):
    src = tmp_path / "layout.c"
    lines = "\n".join(f'  printf("{f} %zu %zu\\n", offsetof(rtw_surface, {f}), sizeof(((rtw_surface*)0)->{f}));' for f in FIELDS)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "rtw_hip.h"\nint main(void) {\n'
                   '  printf("sizeof %zu %zu\\n", sizeof(rtw_surface), _Alignof(rtw_surface));\n' + lines +
                   '\n  printf("abi %d\\n", RTW_ABI_VERSION);\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c11", "-Wall", "-Werror", "-I", INCLUDE, str(src), "-o", str(exe)], check=True)
    out = dict((ln.split()[0], [int(x) for x in ln.split()[1:]]) for ln in subprocess.run([str(exe)], capture_output=True, text=True,
                                                                                         check=True).stdout.splitlines())
    assert out["sizeof"] == [64, 8] and out["abi"] == [4]
    assert C.sizeof(rtw.Surface) == 64 and C.alignment(rtw.Surface) == 8 and rtw.SURFACE_DTYPE.itemsize == 64
    assert [f for f, _ in rtw.Surface._fields_] == FIELDS and list(rtw.SURFACE_DTYPE.names) == FIELDS
    for f in FIELDS:
        off, size = out[f]
        cf = getattr(rtw.Surface, f)
        assert (cf.offset, cf.size) == (off, size), f
        dt, doff = rtw.SURFACE_DTYPE.fields[f][:2]
        assert (doff, dt.itemsize) == (off, size), f
    assert out["value"] == [0, 24] and out["kind"] == [40, 4] and out["reserved"] == [56, 8]


def test_symbols_declared_exported_and_bound(rtw):
    txt = re.sub(r"/\*.*?\*/", "", open(rtw.HEADER_PATH).read(), flags=re.S)
    L = rtw.lib()
    for name, n_args in SYMBOLS.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
        assert m, f"{name} is not declared in rtw_hip.h"
        assert len(m.group(1).split(",")) == n_args, (name, m.group(1))
        assert name in rtw.header_symbols() and hasattr(L, name), name
        assert len(getattr(L, name).argtypes) == n_args, name
    decl = re.search(r"int\s+rtw_world_surface_device\s*\(([^)]*)\)", txt).group(1)
    assert [a.split()[-1].lstrip("*").split("[")[0] for a in decl.split(",")] == ["w", "d_hits", "n", "background", "d_surf",
                                                                              "d_guides", "stream"]
    assert "typedef struct" in txt and re.search(r"}\s*rtw_surface\s*;", txt)
    assert L.rtw_abi_version() == 4  # new symbols only
    from rtw_amd import world
    from rtw_amd.device import TorchTracer
    assert callable(world.DeviceWorld.surface) and callable(world.DeviceWorld.surface_host) and callable(rtw.DeviceScene.surface)
    assert callable(TorchTracer.surface) and callable(TorchTracer.guides)


def test_null_arguments_are_refused_without_a_device(rtw):
    L = rtw.lib()
    hits = np.zeros(4, rtw.HIT_DTYPE)
    surf = np.full(4, 7, np.uint8).repeat(64).view(rtw.SURFACE_DTYPE)
    before = surf.tobytes()
    assert L.rtw_world_surface(None, hits.ctypes.data, 4, surf.ctypes.data) == rtw.RTW_EINVAL
    assert b"rtw_world_surface" in L.rtw_last_error()
    assert L.rtw_world_surface(None, None, 0, None) == rtw.RTW_EINVAL
    bg = (C.c_double * 3)(0.1, 0.2, 0.3)
    assert L.rtw_world_surface_device(None, hits.ctypes.data, 4, bg, surf.ctypes.data, None, None) == rtw.RTW_EINVAL
    assert L.rtw_scene_surface_device(None, hits.ctypes.data, 4, bg, surf.ctypes.data, None, None) == rtw.RTW_EINVAL
    assert surf.tobytes() == before


def _build_check(out_dir, extra=()):
    exe = os.path.join(str(out_dir), "surface_check")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", *extra, "-I", CSRC, "-I", INCLUDE,
                        os.path.join(REPO, "tests", "native", "surface_check.cpp"), "-o", exe], capture_output=True, text=True)
    return exe, r


def _run_check(exe):
    p = subprocess.run([exe], capture_output=True, text=True)
    m = re.search(r"surface_check: bad (\d+)/(\d+)", p.stdout)
    assert m, p.stdout + p.stderr
    return p.returncode, int(m.group(1)), int(m.group(2)), p.stdout + p.stderr


@needs_gxx
def test_argument_check_as_a_plain_program(tmp_path):
    exe, r = _build_check(tmp_path)
    assert r.returncode == 0, r.stderr
    rc, bad, checks, out = _run_check(exe)
    assert rc == 0 and bad == 0, out
    assert checks >= 4000  # the refusals and the overlap sweep did run


@needs_gxx
def test_argument_check_clean_under_host_sanitizers(tmp_path):
    exe, r = _build_check(tmp_path, extra=["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    if r.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|libasan|libubsan", r.stderr):
        pytest.skip("sanitizer runtime not installed")
    assert r.returncode == 0, r.stderr
    rc, bad, _, out = _run_check(exe)
    assert rc == 0 and bad == 0 and "runtime error" not in out and "AddressSanitizer" not in out, out


def test_frames_hold_every_class_of_record(rtw, oracle):
    """The census of tests/test_gpu_surface.py's frames and of its bounce, on the oracle alone."""
    from rtw_amd import world as W
    from query_helpers import oracle_hits
    from surface_helpers import FRAMES, bounce_rays, check_census, get_case, guides_of, oracle_surface
    for name in FRAMES:
        case = get_case(rtw, oracle, W, name)
        c = check_census(oracle, W, case)
        hit = case.ref_surf["kind"] > 0
        assert (hit == (case.ref_hits["prim"] > 0)).all() and c["miss"] == (~hit).sum()
        g = guides_of(rtw, case.ref_hits, case.ref_surf, case.background)
        assert (g["prim"] == case.ref_hits["prim"]).all() and (g["depth"][hit] > 0).all() and (g["depth"][~hit] == 0).all()
    want = {"scene1": {"solid": 30, "solid_moving": 64, "checker": 802, "metal": 287, "glass": 74, "miss": 279},
            "scene3": {"noise": 1119}, "scene4": {"image": 394}, "scene5": {"light_rect": 14}, "scene6": {"light": 7},
            "scene7": {"image": 374, "solid_moving": 344, "metal": 47, "glass": 11, "checker": 250}}
    for name, counts in want.items():  # what the frames were counted to hold
        case = get_case(rtw, oracle, W, name)
        c = check_census(oracle, W, case)
        assert {k: c[k] for k in counts} == counts, (name, c)
    for name, need in (("scene1", ("inside", "metal", "glass", "checker", "miss")), ("scene6", ("back", "xy_back", "xz_back", "yz_back", "xform")),
                       ("scene7", ("inside", "image", "metal", "glass", "checker", "miss"))):
        case = get_case(rtw, oracle, W, name)
        rays = bounce_rays(rtw, case.rays, case.ref_hits)
        hits = oracle_hits(rtw, case.oracle, rays)
        check_census(oracle, W, case, hits, oracle_surface(rtw, oracle, case.oracle, hits, case.desc), need)
