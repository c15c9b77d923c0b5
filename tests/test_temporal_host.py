"""Temporal accumulation on the CPU: csrc/rtw_temporal.hpp held
against the definition stated a second time, bit for bit, and its properties
(tests/native/temporal_check.cpp, built with g++ and no HIP, once more with the
address and undefined-behaviour sanitizers as a plain executable, and once
against a copy of the header without the snap, which must be caught); the new
entry points declared, exported and bound; rtw_temporal_host through Python: the
first frame, a static camera's running mean, refused arguments.  No GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import PKG_ROOT, REPO

CSRC = os.path.join(PKG_ROOT, "csrc")
SRC = os.path.join(REPO, "tests", "native", "temporal_check.cpp")
FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off"]
RESULT = r"temporal_check: bad (\d+)/(\d+)"
SYMBOLS = ["rtw_temporal_device", "rtw_temporal_host", "rtw_pixel_rays_device", "rtw_world_prev_points_device",
           "rtw_world_prev_points_host"]

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


def _build(out_dir, inc=CSRC, extra=()):
    exe = os.path.join(str(out_dir), "temporal_check")
    return exe, subprocess.run(["g++", *FLAGS, *extra, "-I", str(inc), SRC, "-o", exe], capture_output=True, text=True)


def _run(exe):
    p = subprocess.run([exe], capture_output=True, text=True)
    m = re.search(RESULT, p.stdout)
    assert m, p.stdout + p.stderr
    print(p.stdout.strip()[-2000:])
    return p.returncode, int(m.group(1)), int(m.group(2)), p.stdout + p.stderr


@needs_gxx
def test_header_matches_the_definition_and_its_properties(tmp_path):
    exe, r = _build(tmp_path)
    assert r.returncode == 0, r.stderr
    rc, bad, checks, out = _run(exe)
    assert rc == 0 and bad == 0, out
    assert checks >= 20000  # the checks did run: every pixel of every fuzzed frame


@needs_gxx
def test_temporal_check_has_teeth(tmp_path):
    """Without the snap a static scene no longer reads exactly its own pixel: the round trip must say so."""
    d = tmp_path / "broken"
    d.mkdir()
    src = open(os.path.join(CSRC, "rtw_temporal.hpp")).read()
    line = "constexpr double kSnap = 0x1p-10,"
    assert src.count(line) == 1
    (d / "rtw_temporal.hpp").write_text(src.replace(line, "constexpr double kSnap = 0.0,"))
    for name in ("rtw_denoise.hpp", "rtw_world_refit.hpp", "rtw_layout.hpp"):
        shutil.copy(os.path.join(CSRC, name), d / name)
    exe, r = _build(d, inc=d)
    assert r.returncode == 0, r.stderr
    rc, bad, _, out = _run(exe)
    assert rc != 0 and bad > 0, out


@needs_gxx
def test_temporal_check_clean_under_host_sanitizers(tmp_path):
    exe, r = _build(tmp_path, extra=["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    if r.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|libasan|libubsan", r.stderr):
        pytest.skip("sanitizer runtime not installed")
    assert r.returncode == 0, r.stderr
    rc, bad, _, out = _run(exe)
    assert rc == 0 and bad == 0 and "ERROR: AddressSanitizer" not in out and "runtime error" not in out, out


def test_c_abi_of_temporal_accumulation(rtw):
    from rtw_amd import device, world
    syms = rtw.header_symbols()
    for s in SYMBOLS:
        assert s in syms and hasattr(rtw.lib(), s) and getattr(rtw.lib(), s).argtypes, s
    assert rtw.abi_version() == 4
    assert C.sizeof(rtw.History) == 32 and rtw.HISTORY_DTYPE.itemsize == 32 and C.sizeof(rtw.TemporalOpts) == 24
    for f in (rtw.temporal_host, rtw.temporal_device, rtw.pixel_rays_device, world.prev_points_host,
              world.DeviceWorld.prev_points_device, device.TemporalAccumulator.step, device.TemporalAccumulator.reset):
        assert callable(f), f


@pytest.fixture(scope="module")
def frames(rtw):
    """K = 8 frames of 9 x 6 means over constant guides (hits of three primitives and misses)."""
    rng = np.random.default_rng(18)
    W, H, K = 9, 6, 8
    g = np.zeros((H, W), rtw.GUIDE_DTYPE)
    g["prim"] = rng.integers(0, 4, (H, W))
    g["depth"] = np.where(g["prim"] > 0, rng.uniform(1, 3, (H, W)), 0).astype(np.float32)
    g["normal"][..., 2] = g["prim"] > 0
    means = rng.uniform(0, 2, (K, H, W, 3)).astype(np.float32)
    cam = rtw.camera_init((13, 2, 3), (0, 0, 0), (0, 1, 0), 20.0, W / H, 0.0, 10.0)
    return W, H, K, g, means, cam


def test_first_frame_through_python(rtw, frames):
    W, H, K, g, means, cam = frames
    ho, mo, vo = rtw.temporal_host(means[0], g, cam, cam)
    assert mo.tobytes() == means[0].tobytes() and ho["mean"].tobytes() == means[0].tobytes()
    assert (ho["len"] == 1).all() and (vo == rtw.VAR_UNKNOWN).all()
    assert (ho["prim"] == g["prim"]).all() and ho["depth"].tobytes() == g["depth"].tobytes()
    m = means[0].astype(np.float64)
    y = (0.2126 * m[..., 0] + 0.7152 * m[..., 1]) + 0.0722 * m[..., 2]
    assert (ho["m1"] == y.astype(np.float32)).all() and (ho["m2"] == (y * y).astype(np.float32)).all()


@pytest.mark.parametrize("max_history", [0, 3])
def test_static_camera_running_mean(rtw, frames, max_history):
    """prev_p None over constant guides: the f64 running mean of the inputs, rounded each frame (8 frames of
    f32 rounding at 6e-8 each: rtol 1e-6); len counts 1..8, and stops at max_history + 1."""
    W, H, K, g, means, cam = frames
    opts = rtw.temporal_opts(max_history=max_history)
    hist, rm = None, np.zeros((H, W, 3))
    for k in range(K):
        hist, mo, vo = rtw.temporal_host(means[k], g, cam, cam, hist_in=hist, opts=opts)
        rm += (means[k].astype(np.float64) - rm) / (k + 1)
        if max_history == 0:
            assert (hist["len"] == k + 1).all()
            np.testing.assert_allclose(mo, rm, rtol=1e-6, atol=0)
            assert ((vo >= 0) == (k + 1 >= 4)).all()  # min_len_var's default
        else:
            assert (hist["len"] == min(k + 1, max_history + 1)).all()


def test_refused_arguments(rtw, frames):
    W, H, K, g, means, cam = frames
    L = rtw.lib()
    m = np.ascontiguousarray(means[0])
    ho = np.zeros((H, W), rtw.HISTORY_DTYPE)
    mo, vo = np.zeros((H, W, 3), np.float32), np.zeros((H, W), np.float32)
    big = np.zeros((2 * H, W), rtw.HISTORY_DTYPE)  # room for two history images side by side
    assert big.ctypes.data % 16 == 0

    def call(mean=m.ctypes.data, guides=g.ctypes.data, prev_p=None, cam_prev=C.byref(cam), cam_now=C.byref(cam), hist_in=None,
             w=W, h=H, opts=None, hist_out=ho.ctypes.data, mean_out=mo.ctypes.data, var_out=vo.ctypes.data):
        return L.rtw_temporal_host(mean, guides, prev_p, cam_prev, cam_now, hist_in, w, h, opts, hist_out, mean_out,
                                   var_out, None)
    assert call() == rtw.RTW_OK
    assert call(mean_out=None, var_out=None) == rtw.RTW_OK  # the optional outputs
    for bad in (dict(mean=None), dict(guides=None), dict(cam_prev=None), dict(cam_now=None), dict(hist_out=None),
                dict(w=1), dict(h=1), dict(guides=g.ctypes.data + 8), dict(hist_out=ho.ctypes.data + 4),
                dict(hist_in=ho.ctypes.data + 8), dict(prev_p=mo.ctypes.data + 4), dict(hist_in=ho.ctypes.data),
                dict(mean_out=m.ctypes.data),
                # overlaps that share no pointer: an output inside an input, an input's tail, two outputs
                dict(mean_out=m.ctypes.data + 12), dict(var_out=g.ctypes.data + 32 * (W * H - 1)),
                dict(hist_out=big.ctypes.data, hist_in=big.ctypes.data + 32),
                dict(hist_out=big.ctypes.data, var_out=big.ctypes.data + 32 * W * H - 4),
                # the image's size: a side above 65,536, more than 2^28 pixels
                dict(w=65537), dict(h=65537), dict(w=65536, h=4097)):
        assert call(**bad) == rtw.RTW_EINVAL, bad
        assert rtw.lib().rtw_last_error()
    assert call(hist_out=big.ctypes.data, var_out=big.ctypes.data + 32 * W * H) == rtw.RTW_OK  # adjacent is not overlapping
    for o in (rtw.temporal_opts(max_history=4097), rtw.temporal_opts(depth_tol=-0.1), rtw.temporal_opts(depth_tol=np.nan),
              rtw.temporal_opts(depth_tol=np.inf), rtw.temporal_opts(min_len_var=1), rtw.temporal_opts(flags=1)):
        assert call(opts=C.byref(o)) == rtw.RTW_EINVAL
    assert call(opts=C.byref(rtw.temporal_opts(4096, 1.0, 2, 0))) == rtw.RTW_OK
