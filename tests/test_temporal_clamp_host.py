"""The clamped temporal accumulation on the CPU:
csrc/rtw_temporal_clamp.hpp held against the definition stated a second time,
bit for bit, and its properties (tests/native/temporal_clamp_check.cpp, built
with g++ and no HIP, once more with the address and undefined-behaviour
sanitizers as a plain executable, and once against a copy of the header whose
clamp is inverted, which must be caught); the new entry points declared,
exported and bound; rtw_temporal_clamped_host through Python: clamp None and a
clamp too wide to bite give rtw_temporal_host's bytes, a step change is followed
at once, and the refused arguments.  No GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import PKG_ROOT, REPO

CSRC = os.path.join(PKG_ROOT, "csrc")
SRC = os.path.join(REPO, "tests", "native", "temporal_clamp_check.cpp")
FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off"]
RESULT = r"temporal_clamp_check: bad (\d+)/(\d+)"
SYMBOLS = ["rtw_temporal_clamped_device", "rtw_temporal_clamped_host"]

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


def _build(out_dir, inc=CSRC, extra=()):
    exe = os.path.join(str(out_dir), "temporal_clamp_check")
    return exe, subprocess.run(["g++", *FLAGS, *extra, "-I", str(inc), SRC, "-o", exe], capture_output=True, text=True)


def _run(exe):
    p = subprocess.run([exe], capture_output=True, text=True)
    m = re.search(RESULT, p.stdout)
    assert m, p.stdout + p.stderr
    print(p.stdout.strip()[-2000:])
    return p.returncode, int(m.group(1)), int(m.group(2)), p.stdout + p.stderr


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32).reshape(-1)


@needs_gxx
def test_header_matches_the_definition_and_its_properties(tmp_path):
    exe, r = _build(tmp_path)
    assert r.returncode == 0, r.stderr
    rc, bad, checks, out = _run(exe)
    assert rc == 0 and bad == 0, out
    assert checks >= 200000  # the checks did run: every pixel of every fuzzed frame, radius and gamma


@needs_gxx
def test_clamp_check_has_teeth(tmp_path):
    """With min and max exchanged in the clamp the history is thrown to the far bound: the check must say so."""
    d = tmp_path / "broken"
    d.mkdir()
    src = open(os.path.join(CSRC, "rtw_temporal_clamp.hpp")).read()
    line = "const double k0 = fmin(fmax(h0, mu0 - g0), mu0 + g0);"
    assert src.count(line) == 1
    (d / "rtw_temporal_clamp.hpp").write_text(src.replace(line, "const double k0 = fmax(fmin(h0, mu0 - g0), mu0 + g0);"))
    for name in ("rtw_temporal.hpp", "rtw_denoise.hpp", "rtw_world_refit.hpp", "rtw_layout.hpp"):
        shutil.copy(os.path.join(CSRC, name), d / name)
    exe, r = _build(d, inc=d)
    assert r.returncode == 0, r.stderr
    rc, bad, _, out = _run(exe)
    assert rc != 0 and bad > 0, out


@needs_gxx
def test_clamp_check_clean_under_host_sanitizers(tmp_path):
    exe, r = _build(tmp_path, extra=["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    if r.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|libasan|libubsan", r.stderr):
        pytest.skip("sanitizer runtime not installed")
    assert r.returncode == 0, r.stderr
    rc, bad, _, out = _run(exe)
    assert rc == 0 and bad == 0 and "ERROR: AddressSanitizer" not in out and "runtime error" not in out, out


def test_c_abi_of_the_clamp(rtw):
    from rtw_amd import device
    syms = rtw.header_symbols()
    for s in SYMBOLS:
        assert s in syms and hasattr(rtw.lib(), s) and getattr(rtw.lib(), s).argtypes, s
    assert rtw.abi_version() == 4
    assert C.sizeof(rtw.TemporalClamp) == 16 and C.sizeof(rtw.TemporalOpts) == 24
    k = rtw.temporal_clamp()
    assert (k.gamma, k.radius, k.reserved) == (0.0, 0, 0)
    k = rtw.temporal_clamp(gamma=1.5, radius=2)
    assert (k.gamma, k.radius, k.reserved) == (1.5, 2, 0)
    for f in (rtw.temporal_clamped_host, rtw.temporal_clamped_device, device.TemporalAccumulator.step):
        assert callable(f), f
    import inspect
    assert "clamp" in inspect.signature(device.TemporalAccumulator.__init__).parameters
    for f in (rtw.temporal_clamped_host, rtw.temporal_clamped_device):  # `clamp` comes right after `opts`
        names = list(inspect.signature(f).parameters)
        assert names.index("clamp") == names.index("opts") + 1, names


@pytest.fixture(scope="module")
def frames(rtw):
    """Two frames of 9 x 6 finite means over constant guides (hits of three primitives and misses) and the
    first frame's history."""
    rng = np.random.default_rng(20)
    W, H = 9, 6
    g = np.zeros((H, W), rtw.GUIDE_DTYPE)
    g["prim"] = rng.integers(0, 4, (H, W))
    g["depth"] = np.where(g["prim"] > 0, rng.uniform(1, 3, (H, W)), 0).astype(np.float32)
    g["normal"][..., 2] = g["prim"] > 0
    means = rng.uniform(0, 2, (2, H, W, 3)).astype(np.float32)
    cam = rtw.camera_init((13, 2, 3), (0, 0, 0), (0, 1, 0), 20.0, W / H, 0.0, 10.0)
    first = rtw.temporal_host(means[0], g, cam, cam)
    return W, H, g, means, cam, first


def test_no_clamp_and_a_clamp_that_does_not_bite_are_the_unclamped_call(rtw, frames):
    W, H, g, means, cam, first = frames
    opts = rtw.temporal_opts(min_len_var=2)
    want = rtw.temporal_host(means[1], g, cam, cam, hist_in=first[0], opts=opts)
    for clamp in (None, rtw.temporal_clamp(gamma=9e29), rtw.temporal_clamp(gamma=9e29, radius=3)):
        got = rtw.temporal_clamped_host(means[1], g, cam, cam, hist_in=first[0], opts=opts, clamp=clamp)
        for a, b in zip(got, want):
            assert np.array_equal(u32(a), u32(b))
    got = rtw.temporal_clamped_host(means[0], g, cam, cam, clamp=rtw.temporal_clamp())  # the first frame
    for a, b in zip(got, first):
        assert np.array_equal(u32(a), u32(b))
    bites = rtw.temporal_clamped_host(means[1], g, cam, cam, hist_in=first[0], opts=opts, clamp=rtw.temporal_clamp(gamma=0.5))
    assert not np.array_equal(u32(bites[1]), u32(want[1]))  # (uniform noise against uniform noise: a narrow clamp bites)
    assert (bites[0]["len"] == 2).all()  # len is untouched


def test_step_change_through_python(rtw, frames):
    """History of a constant image A with len 8, the frame a constant image B: sigma 0 in every window, so the
    clamped mean is B's bytes; the unclamped call lags at A + (B - A) / 9."""
    W, H, g, means, cam, first = frames
    A, B = np.float32([0.8, 0.3, 1.7]), np.float32([0.1, 1.3, 0.45])
    hist = np.zeros((H, W), rtw.HISTORY_DTYPE)
    ya = (0.2126 * float(A[0]) + 0.7152 * float(A[1])) + 0.0722 * float(A[2])
    yb = (0.2126 * float(B[0]) + 0.7152 * float(B[1])) + 0.0722 * float(B[2])
    hist["mean"], hist["len"], hist["m1"], hist["m2"] = A, 8, ya, ya * ya
    hist["depth"], hist["prim"] = g["depth"], g["prim"]
    cur = np.broadcast_to(B, (H, W, 3)).copy()
    for gamma in (0.0, 0.5, 3.0):  # (0: the default)
        ho, mo, vo = rtw.temporal_clamped_host(cur, g, cam, cam, hist_in=hist, clamp=rtw.temporal_clamp(gamma=gamma, radius=2))
        assert mo.tobytes() == cur.tobytes() and (ho["len"] == 9).all()
        np.testing.assert_allclose(ho["m1"], yb, rtol=1e-6, atol=0)
    _, mo, _ = rtw.temporal_host(cur, g, cam, cam, hist_in=hist)
    lag = (A.astype(np.float64) + (1.0 / 9.0) * (B.astype(np.float64) - A.astype(np.float64))).astype(np.float32)
    assert (mo == lag).all()


def test_refused_arguments(rtw, frames):
    W, H, g, means, cam, first = frames
    L = rtw.lib()
    m = np.ascontiguousarray(means[0])
    ho = np.zeros((H, W), rtw.HISTORY_DTYPE)
    mo, vo = np.zeros((H, W, 3), np.float32), np.zeros((H, W), np.float32)
    ok_clamp = rtw.temporal_clamp(1.0, 1)

    def call(mean=m.ctypes.data, guides=g.ctypes.data, prev_p=None, cam_prev=C.byref(cam), cam_now=C.byref(cam), hist_in=None,
             w=W, h=H, opts=None, clamp=C.byref(ok_clamp), hist_out=ho.ctypes.data, mean_out=mo.ctypes.data,
             var_out=vo.ctypes.data):
        return L.rtw_temporal_clamped_host(mean, guides, prev_p, cam_prev, cam_now, hist_in, w, h, opts, clamp, hist_out,
                                           mean_out, var_out, None)
    assert call() == rtw.RTW_OK
    assert call(mean_out=None, var_out=None) == rtw.RTW_OK  # the optional outputs
    for clamp in (None, C.byref(ok_clamp)):  # every check of rtw_temporal_host, with and without a clamp
        for bad in (dict(mean=None), dict(guides=None), dict(cam_prev=None), dict(cam_now=None), dict(hist_out=None),
                    dict(w=1), dict(h=1), dict(guides=g.ctypes.data + 8), dict(hist_out=ho.ctypes.data + 4),
                    dict(hist_in=ho.ctypes.data + 8), dict(prev_p=mo.ctypes.data + 4), dict(hist_in=ho.ctypes.data),
                    dict(mean_out=m.ctypes.data), dict(mean_out=m.ctypes.data + 12),
                    dict(var_out=g.ctypes.data + 32 * (W * H - 1)), dict(w=65537), dict(h=65537), dict(w=65536, h=4097),
                    dict(opts=C.byref(rtw.temporal_opts(max_history=4097))), dict(opts=C.byref(rtw.temporal_opts(depth_tol=-0.1))),
                    dict(opts=C.byref(rtw.temporal_opts(min_len_var=1))), dict(opts=C.byref(rtw.temporal_opts(flags=1))),
                    dict(opts=C.byref(rtw.temporal_opts(flags=2)))):
            assert call(clamp=clamp, **bad) == rtw.RTW_EINVAL, bad
            assert rtw.lib().rtw_last_error()
    for k in (rtw.TemporalClamp(-0.5, 0, 0), rtw.TemporalClamp(np.nan, 0, 0), rtw.TemporalClamp(np.inf, 0, 0),
              rtw.TemporalClamp(-np.inf, 0, 0), rtw.TemporalClamp(1e30, 0, 0), rtw.TemporalClamp(1.0, 4, 0),
              rtw.TemporalClamp(1.0, 1, 1), rtw.TemporalClamp(0.0, 0, 0x80000000)):
        assert call(clamp=C.byref(k)) == rtw.RTW_EINVAL, (k.gamma, k.radius, k.reserved)
        assert b"clamp" in rtw.lib().rtw_last_error()
    for k in (rtw.TemporalClamp(0.0, 0, 0), rtw.TemporalClamp(9.9e29, 3, 0), rtw.TemporalClamp(1e-3, 2, 0)):
        assert call(clamp=C.byref(k)) == rtw.RTW_OK
