"""The spatial variance estimate on the CPU: its properties
with a plain C++ compiler (tests/native/denoise_spatial_check.cpp), the new
entry points declared, exported and bound, bad arguments refused, the flagged
filter call = the unflagged call on the stand-alone entry's map, and the
quality of a single-chunk preview against the oracle: with the flag,
rtw_denoise_host must beat both its input and the unflagged call.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG_ROOT, REPO
from denoise_helpers import rmse

SPATIAL_SYMBOLS = ["rtw_denoise_spatial_variance_host", "rtw_denoise_spatial_variance_device"]


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_estimate_properties_native(tmp_path):
    exe = tmp_path / "denoise_spatial_check"
    src = os.path.join(REPO, "tests", "native", "denoise_spatial_check.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(PKG_ROOT, "csrc"), src,
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and "bad 0/" in r.stdout, r.stdout + r.stderr


def test_header_declares_library_exports_and_python_binds(rtw):
    syms = rtw.header_symbols()
    for s in SPATIAL_SYMBOLS:
        assert s in syms, s
        assert hasattr(rtw.lib(), s), s
        assert getattr(rtw.lib(), s).argtypes, s
    assert callable(rtw.spatial_variance_host) and callable(rtw.spatial_variance_device)
    assert rtw.DENOISE_SPATIAL_VAR == 4
    assert "RTW_DENOISE_SPATIAL_VAR 4u" in open(os.path.join(REPO, "include", "rtw_hip.h")).read()
    assert rtw.abi_version() == 4 and C.sizeof(rtw.DenoiseOpts) == 48


def test_bad_arguments_are_refused(rtw):
    L, E = rtw.lib(), rtw.RTW_EINVAL
    W, H = 8, 6
    mean = np.zeros((H, W, 3), np.float32)
    var = np.full((H, W), rtw.VAR_UNKNOWN, np.float32)
    out = np.zeros((H, W), np.float32)

    def refused(st):
        return st == E and len(L.rtw_last_error()) > 0

    for f in (L.rtw_denoise_spatial_variance_host, L.rtw_denoise_spatial_variance_device):
        # (the device entry checks its arguments before it touches the GPU: host pointers are never read)
        def call(mean_p=mean.ctypes.data, var_p=var.ctypes.data, opts=None, out_p=out.ctypes.data, w=W, h=H, f=f):
            return f(mean_p, var_p, None, w, h, C.byref(opts) if opts is not None else None, out_p, None)

        assert refused(call(mean_p=None))
        assert refused(call(out_p=None))
        assert refused(call(w=0)) and refused(call(h=0))
        assert refused(call(opts=rtw.denoise_opts(flags=1 << 7)))
        assert refused(call(opts=rtw.denoise_opts(sigma_depth=-1.0)))
        assert refused(call(out_p=var.ctypes.data)) and refused(call(out_p=mean.ctypes.data))  # var_out aliases an input
    assert L.rtw_denoise_spatial_variance_host(mean.ctypes.data, var.ctypes.data, None, W, H, None, out.ctypes.data,
                                               None) == rtw.RTW_OK
    for flags in (0, rtw.DENOISE_SPATIAL_VAR, rtw.DENOISE_DIRECT | rtw.DENOISE_SPATIAL_VAR | rtw.DENOISE_NO_COLOR):
        assert L.rtw_denoise_spatial_variance_host(mean.ctypes.data, None, None, W, H,
                                                   C.byref(rtw.denoise_opts(flags=flags)), out.ctypes.data,
                                                   None) == rtw.RTW_OK
    # the filter entries still refuse an unknown flag
    assert L.rtw_denoise_workspace_bytes(W, H, C.byref(rtw.denoise_opts(flags=8))) == 0


def test_workspace_sizes_do_not_change(rtw):
    for w, h in ((1, 1), (19, 33), (1200, 675)):
        for levels in (0, 1, 2, 6):
            plain = rtw.denoise_workspace_bytes(w, h, rtw.denoise_opts(levels=levels))
            assert rtw.denoise_workspace_bytes(w, h, rtw.denoise_opts(levels=levels,
                                                                      flags=rtw.DENOISE_SPATIAL_VAR)) == plain
            assert plain == rtw.denoise_workspace_bytes(w, h)


def mixed_case(rtw, w=33, h=19, seed=11):
    """Random data with a mixed known / unknown / empty variance map and guides with misses."""
    rng = np.random.default_rng(seed)
    mean = rng.uniform(0.0, 1.0, (h, w, 3)).astype(np.float32)
    var = rng.uniform(1e-4, 1e-2, (h, w)).astype(np.float32)
    kind = rng.integers(0, 6, (h, w))
    var[kind <= 2] = rtw.VAR_UNKNOWN
    var[kind == 3] = rtw.VAR_EMPTY
    mean[kind == 3] = 0.0
    g = np.zeros((h, w), rtw.GUIDE_DTYPE)
    y, x = np.mgrid[0:h, 0:w]
    prim = 1 + (x // 6 + 2 * (y // 5)) % 4
    miss = (x + 3 * y) % 17 < 3
    prim[miss] = 0
    ang = 0.03 * x + 0.02 * y + 0.5 * prim
    g["normal"] = np.stack([np.cos(ang), np.sin(ang) * 0.6, np.sin(ang) * 0.8], axis=-1)
    g["depth"] = 2.0 + 0.02 * x + 0.4 * (prim % 3) + rng.uniform(0.0, 0.05, (h, w))
    g["albedo"] = 0.3 + 0.1 * (prim[..., None] % 3) + rng.uniform(0.0, 0.05, (h, w, 3))
    g["prim"] = prim
    g["normal"][miss] = 0.0
    g["depth"][miss] = 0.0
    g["albedo"][miss] = (0.7, 0.8, 1.0)
    return mean, var, g


@pytest.mark.parametrize("levels", [1, 2, 5])
def test_flagged_call_is_the_unflagged_call_on_the_estimated_map(rtw, levels):
    mean, var, guides = mixed_case(rtw)  # 19 rows of 33 pixels
    assert mean.shape == (19, 33, 3)
    for v, g in ((var, guides), (None, guides), (var, None), (None, None)):
        sig = dict(levels=levels, sigma_normal=0.2, sigma_depth=0.3, sigma_albedo=0.15)
        est = rtw.spatial_variance_host(mean, v, g, rtw.denoise_opts(**sig))
        if v is not None:
            known, empty = v >= 0, v == rtw.VAR_EMPTY
            assert known.any() and empty.any() and (v == rtw.VAR_UNKNOWN).any()
            assert np.array_equal(u32(est)[known], u32(v)[known]) and (est[empty] == rtw.VAR_EMPTY).all()
            e = est[~known & ~empty]
        else:
            e = est.ravel()
        # estimated, or left unknown where fewer than 4 taps are kept (a sliver of misses; never without guides)
        assert ((e >= 0) | (e == rtw.VAR_UNKNOWN)).all() and (e >= 0).mean() > (0.9 if g is not None else 0.999)
        rgb_f, out_f = rtw.denoise_host(mean, v, g, rtw.denoise_opts(flags=rtw.DENOISE_SPATIAL_VAR, **sig))
        rgb_u, out_u = rtw.denoise_host(mean, est, g, rtw.denoise_opts(**sig))
        assert np.array_equal(u32(out_f), u32(out_u)) and np.array_equal(rgb_f, rgb_u)
        rgb_p, out_p = rtw.denoise_host(mean, v, g, rtw.denoise_opts(**sig))
        assert not np.array_equal(u32(out_p), u32(out_f))  # (the flag did something)
        # the sigmas are the call's: the default ones give another map
        if g is not None:
            assert not np.array_equal(u32(est), u32(rtw.spatial_variance_host(mean, v, g)))


def test_flag_changes_nothing_without_an_unknown_pixel(rtw):
    mean, var, guides = mixed_case(rtw)
    var = np.where(var == rtw.VAR_UNKNOWN, np.float32(2e-3), var)
    assert (var == rtw.VAR_EMPTY).any() and not (var == rtw.VAR_UNKNOWN).any()
    assert np.array_equal(u32(rtw.spatial_variance_host(mean, var, guides)), u32(var))
    for g in (guides, None):
        for levels in (1, 5):
            a = rtw.denoise_host(mean, var, g, rtw.denoise_opts(levels=levels, flags=rtw.DENOISE_SPATIAL_VAR))
            b = rtw.denoise_host(mean, var, g, rtw.denoise_opts(levels=levels))
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


# ------------------------------------------------------------ quality ----
@pytest.mark.parametrize("name", ["cornell", "cover"])
def test_single_chunk_preview_beats_input_and_the_unflagged_filter(oracle, rtw, name):
    """One 20-spp oracle Tier-B frame at seed 1, no variance, oracle guides; RMSE of the linear
    mean against the 1000-spp oracle frame at seed 99.  Measured:
    cover 60x33: input 0.05301, unflagged 0.06819 (1.286 x input), flagged 0.04495 (0.848 x input);
    cornell 40x40: input 0.21219, unflagged 0.38252 (1.803 x input), flagged 0.16833 (0.793 x input)."""
    from test_denoise_cpu import SCENES, quality_case  # (shares the scene's guides and 1000-spp reference)
    _, _, guides, ref = quality_case(oracle, rtw, name)
    scene_id, W, H = SCENES[name]
    ow = oracle.OracleWorld(scene_id, 42)
    noisy = ow.render_tier_b(ow.camera(W / H), W, H, 20, seed=1, want_mean=True)[1].astype(np.float32)
    _, plain = rtw.denoise_host(noisy, None, guides)
    _, flagged = rtw.denoise_host(noisy, None, guides, rtw.denoise_opts(flags=rtw.DENOISE_SPATIAL_VAR))
    e_in, e_plain, e_flag = rmse(noisy, ref), rmse(plain, ref), rmse(flagged, ref)
    print(f"{name}: rmse input {e_in:.5f} unflagged {e_plain:.5f} ({e_plain / e_in:.3f} x input) "
          f"flagged {e_flag:.5f} ({e_flag / e_in:.3f} x input)")
    assert e_flag < e_in
    assert e_flag < e_plain
