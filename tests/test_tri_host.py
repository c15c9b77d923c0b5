"""The triangle primitive on the CPU (csrc/rtw_tri.hpp).

tests/native/tri_check.cpp, built with g++ and no HIP, holds the header to its contract: axis-aligned triangles
give the rect's bits, closed meshes are closed (edges and vertices, aimed exactly and a few ulps beside), the
barycentric point stays within the derived bound, the two prim_box statements agree for kind 5, degenerate
triangles are reported.  The program runs once more against the header with one line broken (twice: the inside
test's >= made >, and the + 0.0 dropped) and must report violations, and once under the address and
undefined-behaviour sanitizers.  Then the Python layer: load_obj / mesh_prims, and rtw_world_trace_tri_host
against hand-computed records.  (On the parent every world with kind 5 is RTW_EINVAL and rtw_tri.hpp does not exist.)"""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, PKG_ROOT, REPO
from helpers import _to_desc
import tri_helpers as T

CSRC = os.path.join(PKG_ROOT, "csrc")
SRC = os.path.join(REPO, "tests", "native", "tri_check.cpp")
FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off"]
RESULT = r"tri_check: checks (\d+) violations (\d+) bary_ratio (\S+)"
needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


def _build(out_dir, inc=None, extra=()):
    exe = os.path.join(str(out_dir), "tri_check")
    incs = (["-I", str(inc)] if inc else []) + ["-I", os.path.join(REPO, "include"), "-I", CSRC]
    return exe, subprocess.run(["g++", *FLAGS, *extra, *incs, SRC, "-o", exe], capture_output=True, text=True)


def _run(exe):
    p = subprocess.run([exe], capture_output=True, text=True)
    m = re.search(RESULT, p.stdout)
    assert m, p.stdout + p.stderr
    print(p.stdout.strip())
    return p.returncode, int(m.group(1)), int(m.group(2)), float(m.group(3)), p.stderr


@needs_gxx
def test_header_meets_its_contract(tmp_path):
    exe, r = _build(tmp_path)
    assert r.returncode == 0, r.stderr
    rc, checks, viol, ratio, err = _run(exe)
    assert rc == 0 and viol == 0, err
    assert checks >= 1000000  # the checks did run: >= 1e5 rays against the rect formula, every edge and vertex
    assert ratio <= 1.0  # the barycentric point against DESIGN.md §22's bound (observed: 0.004)


@needs_gxx
@pytest.mark.parametrize("old,new", [("(w0 >= -t0 && w1 >= -t1 && w2 >= -t2)", "(w0 > -t0 && w1 > -t1 && w2 > -t2)"),
                                     ("n[0] = Nx / s + 0.0, n[1] = Ny / s + 0.0, n[2] = Nz / s + 0.0;",
                                      "n[0] = Nx / s, n[1] = Ny / s, n[2] = Nz / s;")])
def test_tri_check_has_teeth(tmp_path, old, new):
    """An exclusive inside test opens the mesh along edges whose function is exactly 0; without the + 0.0 an
    axis-aligned triangle's normal carries -0 components."""
    src = open(os.path.join(CSRC, "rtw_tri.hpp")).read()
    assert src.count(old) == 1
    d = tmp_path / "broken"
    d.mkdir()
    (d / "rtw_tri.hpp").write_text(src.replace(old, new))
    exe, r = _build(d, inc=d)
    assert r.returncode == 0, r.stderr
    rc, _, viol, _, err = _run(exe)
    assert rc == 1 and viol > 0, err


@needs_gxx
def test_tri_check_clean_under_host_sanitizers(tmp_path):
    exe, r = _build(tmp_path, extra=["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    if r.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|libasan|libubsan", r.stderr):
        pytest.skip("sanitizer runtime not installed")
    assert r.returncode == 0, r.stderr
    rc, _, viol, _, err = _run(exe)
    assert rc == 0 and viol == 0 and "ERROR: AddressSanitizer" not in err and "runtime error" not in err, err


# ------------------------------------------------------------------ the Python layer ----
@pytest.fixture(scope="module")
def W(rtw):
    from rtw_amd import world
    return world


def test_load_obj_and_mesh_prims(W, tmp_path):
    v, f = W.load_obj(os.path.join(GOLDEN, "tri_fixture.obj"))
    assert v.shape == (11, 3) and f.shape == (13, 3) and v.dtype == np.float64 and f.dtype == np.int64
    assert f[0].tolist() == [3, 2, 1] and f[1].tolist() == [3, 1, 0]            # a quad, fanned from its first vertex
    assert f[4].tolist() == [0, 1, 5] and f[6].tolist() == [1, 2, 6]            # a/b/c and a//c indices
    assert f[12].tolist() == [8, 9, 10] and v[9].tolist() == [3.5, 0.0, 0.25]   # negative indices
    p = tmp_path / "own.obj"
    p.write_text("# own\nv 0 0 0\nv 2 0 0\nv 2 2 0\nv 0 2 0\nv 1 3 0\nvn 0 0 1\nf 1 2 3 4 5\n\nf -5/1 -4/1 -1/1\n")
    v2, f2 = W.load_obj(str(p))
    assert f2.tolist() == [[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 1, 4]] and v2.shape == (5, 3)
    prims = W.mesh_prims(v2, f2, mat=3, xform=-1)
    assert len(prims) == 4 and all(q.kind == W.PRIM_TRIANGLE == 5 and q.mat == 3 and q.xform == -1 for q in prims)
    assert list(prims[2].a) == [0, 0, 0, 0, 2, 0, 1, 3, 0]
    for bad in ("v 0 0 0\nf 1 2 3\n", "v 0 0 0\nv 1 0 0\nf 1 2\n", "v 0 0\n", "v 0 0 0\nf 0 1 1\n"):
        p.write_text(bad)
        with pytest.raises(ValueError):
            W.load_obj(str(p))
    with pytest.raises(ValueError):
        W.mesh_prims(v2, [[0, 1, 7]], 0)


def _world(W, prims, xf=()):
    tex = [dict(kind=W.TEX_SOLID, color=(0.5, 0.5, 0.5))]
    mats = [dict(kind=W.WMAT_LAMBERT, tex=0)]
    return _to_desc(W, prims, list(xf), tex, mats, [], [])


def test_trace_tri_host_records(rtw, W):
    """Hand-computed records: u, v are the weights of v1 and v2; the normal faces the ray; spheres are skipped;
    the later of two coincident triangles wins; a chain moves the triangle."""
    tri = [0, 0, 0, 4, 0, 0, 0, 4, 0]  # n = +z
    sph = dict(kind=W.PRIM_SPHERE, mat=0, xform=-1, a=[1, 1, 5, 1, 1, 5, 1.0, 0, 0])
    xf = [dict(n=1, op=[W.XF_TRANSLATE], v=[(10.0, 0.0, 0.0)])]
    prims = [sph, dict(kind=W.PRIM_TRIANGLE, mat=0, xform=-1, a=tri), dict(kind=W.PRIM_TRIANGLE, mat=0, xform=-1, a=tri),
             dict(kind=W.PRIM_TRIANGLE, mat=0, xform=0, a=tri)]
    desc, keep = _world(W, prims, xf)
    rays = np.zeros(5, rtw.RAY_DTYPE)
    rays["t_max"] = np.inf
    rays[0]["origin"], rays[0]["dir"] = (1, 2, 8), (0, 0, -2)       # front, through the sphere's place
    rays[1]["origin"], rays[1]["dir"] = (1, 2, -3), (0, 0, 1)       # from behind
    rays[2]["origin"], rays[2]["dir"] = (11, 1, 2), (0, 0, -1)      # the translated copy
    rays[3]["origin"], rays[3]["dir"] = (3, 3, 2), (0, 0, -1)       # outside (u + v > 1)
    rays[4]["origin"], rays[4]["dir"] = (1, 2, 8), (0, 0, -2)       # t_max short of the plane
    rays[4]["t_max"] = 3.5
    h = W.trace_tri_host(desc, rays)
    assert h["prim"].tolist() == [3, 3, 4, 0, 0] and h["front"].tolist() == [1, 0, 1, 0, 0]
    assert h["t"].tolist() == [4.0, 3.0, 2.0, 0.0, 0.0]
    assert h["p"][0].tolist() == [1, 2, 0] and h["p"][2].tolist() == [11, 1, 0]
    assert h["normal"][0].tolist() == [0, 0, 1] and h["normal"][1].tolist() == [0, 0, -1]
    assert (h["u"][0], h["v"][0]) == (0.25, 0.5) and (h["u"][2], h["v"][2]) == (0.25, 0.25)
    assert not h[3:].view(np.uint8).any()  # a miss is all zero
    # the library refuses what the kernels would
    for bad in ([0, 0, 0, 1, 1, 1, 2, 2, 2], [0, 0, 0, np.nan, 0, 0, 0, 1, 0]):
        d2, k2 = _world(W, [dict(kind=W.PRIM_TRIANGLE, mat=0, xform=-1, a=bad)])
        with pytest.raises(rtw.RtwError) as e:
            W.trace_tri_host(d2, rays)
        assert e.value.status == rtw.RTW_EINVAL and "zero area" in str(e.value)


def test_creation_and_host_twins_refuse_bad_triangles(rtw, W):
    """rtw_world_create's packer (which runs before any device call), rtw_world_refit_tables_host and the
    rebuild's host twin: RTW_EINVAL with the triangle's message; the prev-point and mirror-point host twins:
    RTW_UNSUPPORTED for a description that holds a triangle."""
    v, f = T.icosphere(3)
    good = T.mesh_dicts(W, v * 3.0, f, 0)
    assert len(good) == 1280
    desc, keep = _world(W, good)
    a, _ = W.desc_numbers(desc)
    # the size of the tables, from the refusal of a wrong size (no device on this machine)
    with pytest.raises(rtw.RtwError) as e:
        W.refit_tables_host(desc, W.WORLD_DYNAMIC, 8)
    nbytes = int(re.search(r"the tables have (\d+)", str(e.value)).group(1))
    ok = W.refit_tables_host(desc, W.WORLD_DYNAMIC, nbytes, a)
    assert ok["blob"].any()
    for row, bad in ((7, [1, 2, 3, 1, 2, 3, 4, 5, 6]), (700, [0, 0, 0, 1, 0, np.inf, 0, 1, 0])):
        a2 = a.copy()
        a2[row] = bad
        for call in (lambda: W.refit_tables_host(desc, W.WORLD_DYNAMIC, nbytes, a2),
                     lambda: W.rebuild_tables_host(desc, W.WORLD_DYNAMIC, nbytes, a2)):
            with pytest.raises(rtw.RtwError) as e:
                call()
            assert e.value.status == rtw.RTW_EINVAL and str(row) in str(e.value), str(e.value)
        prims = [dict(p) for p in good]
        prims[row] = dict(prims[row], a=bad)
        d2, k2 = _world(W, prims)
        with pytest.raises(rtw.RtwError) as e:
            W.DeviceWorld(d2)
        assert e.value.status == rtw.RTW_EINVAL and f"prim {row}: triangle" in str(e.value), str(e.value)
    # a rebuild of the good numbers moves the records and keeps them whole
    rb = W.rebuild_tables_host(desc, W.WORLD_DYNAMIC, nbytes, a)
    assert rb["info"]["max_leaf"] == 1 and rb["blob"].any()
    hits = np.zeros(2, rtw.HIT_DTYPE)
    hits["prim"] = 1
    with pytest.raises(rtw.RtwError) as e:
        W.prev_points_host(desc, hits, 0.5)
    assert e.value.status == rtw.RTW_UNSUPPORTED and "triangle" in str(e.value)
    rays = np.zeros(2, rtw.RAY_DTYPE)
    with pytest.raises(rtw.RtwError) as e:
        W.mirror_rays_host(desc, rays, hits)
    assert e.value.status == rtw.RTW_UNSUPPORTED and "triangle" in str(e.value)


def test_c_abi_of_triangles(rtw, W):
    syms = rtw.header_symbols()
    assert "rtw_world_trace_tri_host" in syms and rtw.lib().rtw_world_trace_tri_host.argtypes
    assert rtw.abi_version() == 4 and W.PRIM_TRIANGLE == 5
    src = open(os.path.join(REPO, "include", "rtw_hip.h")).read()
    assert re.search(r"RTW_PRIM_TRIANGLE = 5\b", src)


@needs_gxx
def test_cpp_mirror_flattens_a_triangle(tmp_path):
    """Hittable::makeTriangle through flattenWorld (tests/native/tri_flatten_check.cpp): kind 5, the vertices, the
    material, the wrappers as a chain."""
    exe = str(tmp_path / "tri_flatten_check")
    src = [os.path.join(REPO, "tests", "native", "tri_flatten_check.cpp"), os.path.join(CSRC, "rtw_host.cpp"),
           os.path.join(CSRC, "rtw_world_host.cpp")]
    r = subprocess.run(["g++", *FLAGS, "-I", os.path.join(REPO, "include"), "-I", CSRC, *src, "-lz", "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    p = subprocess.run([exe], capture_output=True, text=True)
    m = re.search(r"tri_flatten_check: checks (\d+) violations (\d+)", p.stdout)
    assert m and p.returncode == 0 and int(m.group(2)) == 0 and int(m.group(1)) >= 20, p.stdout + p.stderr
