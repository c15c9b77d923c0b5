"""Mirror points on the CPU: csrc/rtw_specular.hpp held against
its properties and an independent solve (tests/native/specular_check.cpp, built
with g++ and no HIP; once more with the address and undefined-behaviour
sanitizers as a plain executable; and once with RTW_SPECULAR_NO_GUARD, the
header without its acceptance guard, which the 5-degree census must catch); the
new entry points declared, exported and bound; the two host forms through
Python on a hand-made world.  No GPU.

The census (2,000 cases per set-up, uniform over the sphere's image: a pixel is
a case), as the check printed it when this test was written, pixels at 1200x675:

    set-up            point      mean      p50       p95       p99       max    within 0.1 px
    r = 1,   1 deg    surface    2.11      0.934     8.74      14.8      19.2   0.0250
                      predictor  0.609     0.217     2.53      5.17      8.54   0.3255
                      newton 2   0.000987  7.8e-11   4.1e-05   0.00661   1.03   0.9990
    r = 0.2, 1 deg    surface    1.6       0.249     7.54      13.1      20.8   0.2912
                      predictor  0.587     0.0757    2.95      7         20.8   0.5397
                      newton 2   0.112     1.9e-11   0.00764   4.37      20.8   0.9714
    r = 1,   5 deg    surface    11        4.65      44.9      71.6      116    0.0005
                      predictor  4.14      1.15      16.9      47        116    0.0882
                      newton 2   0.934     1.3e-10   0.0741    44        116    0.9539
"""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import PKG_ROOT, REPO
from helpers import _rot, _to_desc

CSRC = os.path.join(PKG_ROOT, "csrc")
SRC = os.path.join(REPO, "tests", "native", "specular_check.cpp")
FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off"]
RESULT = r"specular_check: bad (\d+)/(\d+)"
SYMBOLS = ["rtw_world_mirror_points_device", "rtw_world_mirror_points_host", "rtw_world_mirror_rays_host"]

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


def _build(out_dir, extra=()):
    exe = os.path.join(str(out_dir), "specular_check")
    return exe, subprocess.run(["g++", *FLAGS, *extra, "-I", CSRC, SRC, "-o", exe], capture_output=True, text=True)


def _run(exe):
    p = subprocess.run([exe], capture_output=True, text=True)
    m = re.search(RESULT, p.stdout)
    assert m, p.stdout + p.stderr
    print(p.stdout.strip()[-4000:])
    return p.returncode, int(m.group(1)), int(m.group(2)), p.stdout + p.stderr


@needs_gxx
def test_header_properties_and_the_census(tmp_path):
    exe, r = _build(tmp_path)
    assert r.returncode == 0, r.stderr
    rc, bad, checks, out = _run(exe)
    assert rc == 0 and bad == 0, out
    assert checks >= 20000 and out.count("census") >= 3  # the checks did run


@needs_gxx
def test_specular_check_has_teeth(tmp_path):
    """Without the acceptance guard a Newton step may leave with a larger residual than it came with, or on the far
    side of the sphere: the 5-degree census must say so (and nothing else may)."""
    exe, r = _build(tmp_path, extra=["-DRTW_SPECULAR_NO_GUARD"])
    assert r.returncode == 0, r.stderr
    rc, bad, _, out = _run(exe)
    assert rc != 0 and bad > 0, out
    assert "an accepted iteration broke the guard's promises" in out
    m = re.search(r"guard promises broken: (\d+)", out)
    assert m and int(m.group(1)) > 0, out


@needs_gxx
def test_specular_check_clean_under_host_sanitizers(tmp_path):
    exe, r = _build(tmp_path, extra=["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    if r.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|libasan|libubsan", r.stderr):
        pytest.skip("sanitizer runtime not installed")
    assert r.returncode == 0, r.stderr
    rc, bad, _, out = _run(exe)
    assert rc == 0 and bad == 0 and "ERROR: AddressSanitizer" not in out and "runtime error" not in out, out


def test_c_abi_of_the_mirror_points(rtw):
    from rtw_amd import device, world
    syms = rtw.header_symbols()
    for s in SYMBOLS:
        assert s in syms and hasattr(rtw.lib(), s) and getattr(rtw.lib(), s).argtypes, s
    assert rtw.abi_version() == 4
    assert C.sizeof(rtw.MirrorOpts) == 8 and rtw.MIRROR_PREDICT_ONLY == 1
    o = rtw.mirror_opts(3, 1)
    assert (o.steps, o.flags) == (3, 1)
    for f in (world.mirror_rays_host, world.mirror_points_host, world.DeviceWorld.mirror_points_device,
              device.TorchTracer.mirror_points):
        assert callable(f), f


# ---- the host forms on a world small enough to trace here: spheres and one rect, by hand ----
def _world(W):
    tex = [dict(kind=W.TEX_SOLID, color=(0.5, 0.5, 0.5))]
    mats = [dict(kind=W.WMAT_LAMBERT, tex=0), dict(kind=W.WMAT_METAL, albedo=(0.8, 0.8, 0.8), fuzz=0.0),
            dict(kind=W.WMAT_DIELECTRIC, ir=1.5)]
    xf = [dict(n=2, op=[W.XF_TRANSLATE, W.XF_ROTATE_Y], v=[(0.5, 0.0, -3.0), _rot(0.3)])]

    def sph(c, r, m):
        return dict(kind=W.PRIM_SPHERE, mat=m, xform=-1, a=[*c, *c, r, 0, 0])
    prims = [sph((0, -1000, 0), 1000.0, 0), sph((0, 1, 0), 1.0, 1), sph((2.5, 0.7, 1.0), 0.7, 2),
             dict(kind=W.PRIM_MOVING_SPHERE, mat=1, xform=-1, a=[-2.5, 0.8, 0.5, -2.5, 1.2, 0.5, 0.8, 0.0, 1.0]),
             dict(kind=W.PRIM_XY_RECT, mat=1, xform=0, a=[-3.0, 3.0, 0.0, 3.0, 0.0])]
    return _to_desc(W, prims, xf, tex, mats, [], [])


def _hit_sphere(o, d, c, r, tmin=0.001):
    oc = o - c
    a, hb, cc = d @ d, oc @ d, oc @ oc - r * r
    disc = hb * hb - a * cc
    if disc < 0:
        return None
    for t in ((-hb - np.sqrt(disc)) / a, (-hb + np.sqrt(disc)) / a):
        if t >= tmin:
            return t
    return None


def _records(rtw, W):
    """Hand-made rays and records: a front hit of the metal sphere (its reflected ray goes to the ground), one whose
    reflected ray leaves for the sky, a hit of the glass sphere, a hit of the Lambert ground, a miss, a back-face
    record of the metal sphere, a record of a prim beyond the list."""
    o = np.array([0.0, 3.0, 8.0])
    rays, hits = np.zeros(7, rtw.RAY_DTYPE), np.zeros(7, rtw.HIT_DTYPE)

    def fill(i, d, c, r, prim, front=1):
        t = _hit_sphere(o, d, c, r)
        p = o + t * d
        n = (p - c) / r
        rays[i] = (tuple(o), tuple(d), 0.25 + 0.1 * i, 0.001, np.inf)
        hits[i] = (t, tuple(p), tuple(n if front else -n), 0.0, 0.0, prim, front)
    c = np.array([0.0, 1.0, 0.0])
    fill(0, np.array([0.1, -2.6, -8.0]), c, 1.0, 2)     # lower half: reflects the ground
    fill(1, np.array([0.05, -1.3, -8.0]), c, 1.0, 2)    # upper half: reflects the sky
    fill(2, np.array([2.5, -2.3, -7.0]), np.array([2.5, 0.7, 1.0]), 0.7, 3)
    fill(3, np.array([6.0, -3.0, -4.0]), np.array([0.0, -1000.0, 0.0]), 1000.0, 1)
    rays[4] = (tuple(o), (0.0, 1.0, -1.0), 0.5, 0.001, np.inf)
    fill(5, np.array([0.1, -2.0, -8.0]), c, 1.0, 2, front=0)
    fill(6, np.array([0.1, -2.0, -8.0]), c, 1.0, 99)
    return rays, hits


def test_host_forms_through_python(rtw):
    from rtw_amd import world as W
    desc, keep = _world(W)
    rays, hits = _records(rtw, W)
    rays2, flag = W.mirror_rays_host(desc, rays, hits)
    assert flag.tolist() == [1, 1, 0, 0, 0, 0, 0]
    assert (rays2[flag == 0].view(np.uint64) == 0).all()
    for i in (0, 1):
        d, n = rays[i]["dir"], hits[i]["normal"]
        np.testing.assert_allclose(rays2[i]["dir"], d - 2 * (d @ n) * n, rtol=1e-14, atol=1e-15)
        assert rays2[i]["origin"].tobytes() == hits[i]["p"].tobytes() and rays2[i]["time"] == rays[i]["time"]
        assert rays2[i]["t_min"] == 0.001 and rays2[i]["t_max"] == np.inf
    assert rays2[0]["dir"][1] < 0 < rays2[1]["dir"][1]
    # the reflected rays' records, traced here: ray 0 meets the ground sphere, ray 1 nothing
    hits2 = np.zeros(7, rtw.HIT_DTYPE)
    o2, d2, gc = rays2[0]["origin"], rays2[0]["dir"], np.array([0.0, -1000.0, 0.0])
    t = _hit_sphere(o2, d2, gc, 1000.0)
    p2 = o2 + t * d2
    hits2[0] = (t, tuple(p2), tuple((p2 - gc) / 1000.0), 0.0, 0.0, 1, 1)
    cam = rtw.camera_init((0, 3, 8), (0, 1, 0), (0, 1, 0), 30.0, 1.5, 0.0, 8.0)
    # nothing moved, the same camera: every hit keeps its point (mirrors to 1e-9), misses get zeros
    same = W.mirror_points_host(desc, rays, hits, hits2, cam)
    assert same[[2, 3, 5]].tobytes() == hits["p"][[2, 3, 5]].tobytes() and (same[[4, 6]] == 0).all()
    assert np.abs(same[:2] - hits["p"][:2]).max() <= 1e-9
    # the metal sphere one degree further back on its orbit: non-mirror records equal prev_points_host at each ray's
    # time; the mirror records land on the previous sphere, off its surface point, and obey the law of reflection
    a, xv = W.desc_numbers(desc)
    a_prev = a.copy()
    th = np.deg2rad(-1.0)
    for e in (0, 3):
        x, z = a[1, e], a[1, e + 2] + 4.0
        a_prev[1, e], a_prev[1, e + 2] = np.cos(th) * x + np.sin(th) * z, -np.sin(th) * x + np.cos(th) * z - 4.0
    got = W.mirror_points_host(desc, rays, hits, hits2, cam, a_prev, xv)
    for i in (2, 3, 4, 5, 6):
        assert got[i].tobytes() == W.prev_points_host(desc, hits[i:i + 1], float(rays[i]["time"]), a_prev, xv)[0].tobytes()
    surf = np.stack([W.prev_points_host(desc, hits[i:i + 1], float(rays[i]["time"]), a_prev, xv)[0] for i in (0, 1)])
    cprev, O = a_prev[1, 0:3], np.array([0.0, 3.0, 8.0])
    def residual(m, i):  # the tangential part of unit(m - O) + unit(m - target) on the previous sphere
        n = m - cprev
        va = (m - O) / np.linalg.norm(m - O)
        vb = (m - p2) / np.linalg.norm(m - p2) if i == 0 else -rays2[1]["dir"] / np.linalg.norm(rays2[1]["dir"])
        w = va + vb
        return np.linalg.norm(w - (w @ n) * n)
    for i in (0, 1):
        assert abs(np.linalg.norm(got[i] - cprev) - 1.0) <= 1e-12 and np.linalg.norm(got[i] - surf[i]) > 1e-3
        # (Newton squares a relative error; from a start some 0.1 radii off, two steps leave far less than 1 %)
        assert residual(got[i], i) <= 1e-2 * residual(surf[i], i), (i, residual(got[i], i), residual(surf[i], i))
    # the predictor alone lies between; an unknown flag, too many steps, NULLs and overlaps are refused
    pred = W.mirror_points_host(desc, rays, hits, hits2, cam, a_prev, xv, rtw.mirror_opts(flags=rtw.MIRROR_PREDICT_ONLY))
    assert np.linalg.norm(pred[0] - got[0]) < np.linalg.norm(surf[0] - got[0])
    assert W.mirror_points_host(desc, rays, hits, hits2, cam, a_prev, xv, rtw.mirror_opts(8)).tobytes() != pred.tobytes()
    L, out = rtw.lib(), np.zeros((7, 3))
    big = np.zeros(7 * 10 + 7 * 3)

    def call(d=C.byref(desc), r=rays.ctypes.data, h=hits.ctypes.data, h2=hits2.ctypes.data, n=7, cp=C.byref(cam),
             ap=a_prev.ctypes.data, o=None, pp=out.ctypes.data):
        return L.rtw_world_mirror_points_host(d, r, h, h2, n, cp, ap, None, o, pp)
    assert call() == rtw.RTW_OK
    for bad in (dict(d=None), dict(r=None), dict(h=None), dict(h2=None), dict(cp=None), dict(pp=None),
                dict(r=rays.ctypes.data + 4), dict(pp=out.ctypes.data + 4), dict(n=(1 << 31) + 1),
                dict(o=C.byref(rtw.mirror_opts(9))), dict(o=C.byref(rtw.mirror_opts(0, 2))),
                dict(pp=hits.ctypes.data), dict(pp=rays.ctypes.data + 72 * 7 - 8), dict(pp=hits2.ctypes.data + 8),
                dict(pp=a_prev.ctypes.data)):
        assert call(**bad) == rtw.RTW_EINVAL, bad
        assert L.rtw_last_error()
    assert call(h=big.ctypes.data, pp=big.ctypes.data + 80 * 7) == rtw.RTW_OK  # adjacent is not overlapping
    assert call(r=None, h=None, h2=None, n=0, pp=None) == rtw.RTW_OK
    r2, fl = np.zeros(7, rtw.RAY_DTYPE), np.zeros(7, np.uint8)
    assert L.rtw_world_mirror_rays_host(None, rays.ctypes.data, hits.ctypes.data, 7, r2.ctypes.data, fl.ctypes.data) == rtw.RTW_EINVAL
    assert L.rtw_world_mirror_rays_host(C.byref(desc), None, hits.ctypes.data, 7, r2.ctypes.data, fl.ctypes.data) == rtw.RTW_EINVAL
    assert L.rtw_world_mirror_rays_host(C.byref(desc), rays.ctypes.data, hits.ctypes.data, 7, r2.ctypes.data + 4, fl.ctypes.data) == rtw.RTW_EINVAL
    assert L.rtw_world_mirror_rays_host(C.byref(desc), None, None, 0, None, None) == rtw.RTW_OK
    del keep
