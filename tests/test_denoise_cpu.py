"""The feature-guided denoiser on the CPU: the filter's
properties with a plain C++ compiler (tests/native/denoise_check.cpp), the new
entry points declared, exported and bound, bad arguments refused, and the
filter's quality against the oracle: rtw_denoise_host on noisy oracle renders
with oracle guides must beat both its input and the unguided blur.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG_ROOT, REPO
from denoise_helpers import b3_blur, guides_record, luminance, oracle_guides, rmse

DENOISE_SYMBOLS = ["rtw_scene_guides_device", "rtw_world_guides_device", "rtw_denoise_workspace_bytes",
                   "rtw_denoise_device", "rtw_denoise_host", "rtw_accum_variance_device",
                   "rtw_accum_denoise_workspace_bytes", "rtw_accum_denoise_device"]
REF_SPP = 1000  # the reference render's samples per pixel (the issue's figure, kept)


def test_filter_properties_native(tmp_path):
    exe = tmp_path / "denoise_check"
    src = os.path.join(REPO, "tests", "native", "denoise_check.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(PKG_ROOT, "csrc"), src,
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and "bad 0/" in r.stdout, r.stdout + r.stderr


def test_header_declares_library_exports_and_python_binds(rtw):
    syms = rtw.header_symbols()
    for s in DENOISE_SYMBOLS:
        assert s in syms, s
        assert hasattr(rtw.lib(), s), s
        assert getattr(rtw.lib(), s).argtypes, s
    assert callable(rtw.denoise_host) and callable(rtw.DeviceScene.guides)
    for m in ("denoise", "variance", "denoise_workspace_bytes"):
        assert callable(getattr(rtw.Accumulator, m)), m
    from rtw_amd import world
    assert callable(world.DeviceWorld.guides)
    assert rtw.abi_version() == 4
    assert C.sizeof(rtw.Guide) == 32 and rtw.GUIDE_DTYPE.itemsize == 32
    assert C.sizeof(rtw.DenoiseOpts) == 48
    assert rtw.denoise_workspace_bytes(1200, 675) >= 2 * 1200 * 675 * 16


def test_bad_arguments_are_refused(rtw):
    L, E = rtw.lib(), rtw.RTW_EINVAL
    W, H = 8, 6
    mean = np.zeros((H, W, 3), np.float32)
    out = np.zeros((H, W, 3), np.float32)
    rgb = np.zeros((H, W, 3), np.uint8)
    nbytes = rtw.denoise_workspace_bytes(W, H)
    ws = np.zeros(nbytes // 4 + 8, np.float32)
    wp = (ws.ctypes.data + 15) & ~15

    def call(mean_p=mean.ctypes.data, opts=None, ws_p=wp, ws_n=nbytes, rgb_p=rgb.ctypes.data, out_p=out.ctypes.data,
             w=W, h=H):
        return L.rtw_denoise_host(mean_p, None, None, w, h, C.byref(opts) if opts is not None else None,
                                  C.c_void_p(ws_p) if ws_p else None, ws_n, rgb_p, out_p, None)

    def refused(st):
        return st == E and len(L.rtw_last_error()) > 0

    assert call() == rtw.RTW_OK
    assert refused(call(mean_p=None))
    assert refused(call(rgb_p=None, out_p=None))
    assert call(rgb_p=None) == rtw.RTW_OK and call(out_p=None) == rtw.RTW_OK  # (one output is enough)
    assert refused(call(ws_p=None))
    assert refused(call(ws_n=nbytes - 1))
    assert refused(call(opts=rtw.denoise_opts(levels=7)))
    assert call(opts=rtw.denoise_opts(levels=6)) == rtw.RTW_OK
    assert refused(call(opts=rtw.denoise_opts(sigma_color=-1.0)))
    assert refused(call(opts=rtw.denoise_opts(sigma_depth=float("nan"))))
    assert refused(call(opts=rtw.denoise_opts(flags=1 << 7)))
    assert refused(call(w=0))
    assert L.rtw_denoise_workspace_bytes(W, H, C.byref(rtw.denoise_opts(levels=7))) == 0
    assert L.rtw_denoise_workspace_bytes(0, H, None) == 0
    # the device entries check their arguments before they touch the GPU
    assert refused(L.rtw_denoise_device(None, None, None, W, H, None, C.c_void_p(wp), nbytes, None, None, None))
    assert refused(L.rtw_accum_variance_device(None, None, None))
    assert refused(L.rtw_accum_denoise_device(None, None, None, None, 0, None, None, None))
    assert L.rtw_accum_denoise_workspace_bytes(None, None) == 0
    assert refused(L.rtw_scene_guides_device(None, None, None, None, None))
    assert refused(L.rtw_world_guides_device(None, None, None, None, None))


def test_unknown_variance_is_the_colour_term_off(rtw):
    rng = np.random.default_rng(5)
    mean = rng.uniform(0.0, 1.0, (19, 33, 3)).astype(np.float32)
    var = rng.uniform(1e-4, 1e-2, (19, 33)).astype(np.float32)
    unknown = np.full((19, 33), rtw.VAR_UNKNOWN, np.float32)
    rgb_a, a = rtw.denoise_host(mean, unknown)
    rgb_b, b = rtw.denoise_host(mean, var, opts=rtw.denoise_opts(flags=rtw.DENOISE_NO_COLOR))
    rgb_c, c = rtw.denoise_host(mean, None)
    assert a.tobytes() == b.tobytes() == c.tobytes() and rgb_a.tobytes() == rgb_b.tobytes() == rgb_c.tobytes()
    assert rtw.denoise_host(mean, var)[1].tobytes() != a.tobytes()


# ------------------------------------------------------------ quality ----
SCENES = {"cover": (1, 60, 33), "cornell": (6, 40, 40)}
_cache = {}


def quality_case(oracle, rtw, name):
    """Input, variance, guides and reference of one scene, computed once."""
    if name in _cache:
        return _cache[name]
    scene_id, W, H = SCENES[name]
    ow = oracle.OracleWorld(scene_id, 42)
    cam = ow.camera(W / H)
    means = [ow.render_tier_b(cam, W, H, 20, seed=s, want_mean=True)[1].astype(np.float64) for s in (1, 2, 3, 4)]
    noisy = np.mean(means, axis=0)
    ys = np.stack([luminance(m) for m in means])
    var = ys.var(axis=0, ddof=1) / len(means)  # squared standard error of the mean luminance
    ref = ow.render_tier_b(cam, W, H, REF_SPP, seed=99, want_mean=True)[1].astype(np.float64)
    guides = guides_record(rtw, oracle_guides(oracle, ow, cam, W, H, ow.background))
    _cache[name] = noisy, var, guides, ref
    return _cache[name]


@pytest.mark.parametrize("name", sorted(SCENES))
def test_denoised_beats_input_and_unguided_blur(oracle, rtw, name):
    """Measured, RMSE against the 1000-spp oracle frame, linear mean:
    cover 60x33: input 0.02561, blur 0.20121, denoised 0.02380 (0.929 x input, 0.118 x blur);
    cornell 40x40: input 0.10023, blur 0.95524, denoised 0.06003 (0.599 x input, 0.063 x blur).
    (At 60x33 the cover scene's small spheres are one or two pixels wide and defocused: little
    of its error is noise a guide can tell from detail.)"""
    noisy, var, guides, ref = quality_case(oracle, rtw, name)
    _, den = rtw.denoise_host(noisy.astype(np.float32), var.astype(np.float32), guides)
    e_in, e_blur, e_den = rmse(noisy, ref), rmse(b3_blur(noisy, 5), ref), rmse(den, ref)
    print(f"{name}: rmse input {e_in:.5f} blur {e_blur:.5f} denoised {e_den:.5f} "
          f"(x input {e_den / e_in:.3f}, x blur {e_den / e_blur:.3f})")
    assert (guides["prim"] == 0).any() or name == "cornell"
    assert (guides["prim"] > 0).sum() > guides.size // 2
    assert e_den < e_in
    assert e_den < e_blur
