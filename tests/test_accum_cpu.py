"""Progressive rendering (rtw_accum_*) on the CPU: the library exports the new
entry points, a pass's workspace is the one-shot workspace of its samples,
the pass rules refuse in the sizing call what a pass would refuse, and the
ABI the existing callers bind is unchanged.  No compute call here."""
import ctypes as C

import pytest

ACCUM_SYMBOLS = ["rtw_accum_create", "rtw_accum_destroy", "rtw_accum_samples", "rtw_accum_workspace_bytes",
                 "rtw_accum_world_workspace_bytes", "rtw_accum_render_device", "rtw_accum_world_render_device",
                 "rtw_accum_resolve_device", "rtw_accum_noise", "rtw_accum_read", "rtw_accum_load"]


def test_header_declares_and_library_exports_the_accumulator(rtw):
    syms = rtw.header_symbols()
    for s in ACCUM_SYMBOLS:
        assert s in syms, s
        assert hasattr(rtw.lib(), s), s


def test_abi_unchanged(rtw):
    assert rtw.abi_version() == 4
    assert C.sizeof(rtw.Params) == 16 + 8 + 24 + 12 + 12 + 8 + 8 * 4


@pytest.mark.parametrize("kw", [dict(), dict(chunk=7), dict(precision="f32", engine="wavefront", wf_paths=4096),
                                dict(row_begin=1, row_stride=3)])
def test_pass_workspace_is_the_one_shot_workspace_of_its_samples(rtw, kw):
    p = rtw.make_params(60, 33, 50, **kw)
    chunk = rtw.effective_chunk(p)
    assert chunk == (kw.get("chunk") or rtw.DEFAULT_CHUNK)
    f = rtw.lib().rtw_accum_workspace_bytes
    for n in (chunk, 2 * chunk, 50):
        q = rtw.make_params(60, 33, n, **kw)
        assert f(C.byref(p), n) == rtw.workspace_bytes(q) > 0, n
    for n in (0, 13, chunk + 1, 51, 60):  # off the chunk grid, or beyond the frame
        assert f(C.byref(p), n) == 0, n
        assert rtw.lib().rtw_last_error()


def test_frame_shorter_than_a_chunk_is_one_pass(rtw):
    p = rtw.make_params(60, 33, 8)  # effective chunk = 8
    assert rtw.effective_chunk(p) == 8
    f = rtw.lib().rtw_accum_workspace_bytes
    assert f(C.byref(p), 8) == rtw.workspace_bytes(p)
    assert f(C.byref(p), 4) == 0 and f(C.byref(p), 16) == 0


def test_config3_pass_memory_is_a_tenth_of_the_one_shot(rtw):
    """BASELINE configs[2] (3840x2160x2000, chunk 20): a pass of 100 samples
    holds 5 chunk sums, the accumulator 40 bytes per pixel; the one-shot
    workspace holds 100 chunk sums (19.9 GB)."""
    p = rtw.make_params(3840, 2160, 2000)
    one_shot = rtw.workspace_bytes(p)
    assert one_shot > 19.9e9
    npix = 3840 * 2160
    progressive = rtw.lib().rtw_accum_workspace_bytes(C.byref(p), 100) + npix * 40
    assert 0 < progressive < one_shot / 10, (progressive, one_shot)


def test_null_arguments_are_refused(rtw):
    L = rtw.lib()
    p = rtw.make_params(60, 33, 50)
    cam = rtw.cover_camera(16 / 9)
    h = C.c_void_p()
    n = C.c_uint32()
    x = C.c_double()
    E = rtw.RTW_EINVAL
    assert L.rtw_accum_create(None, C.byref(h)) == E and not h.value
    assert L.rtw_accum_create(C.byref(p), None) == E
    assert L.rtw_accum_samples(None, C.byref(n)) == E
    assert L.rtw_accum_render_device(None, None, C.byref(cam), 20, None, 0, None, None) == E
    assert L.rtw_accum_world_render_device(None, None, C.byref(cam), 20, None, 0, None, None) == E
    assert L.rtw_accum_resolve_device(None, None, None, None) == E
    assert L.rtw_accum_noise(None, None, C.byref(x)) == E
    assert L.rtw_accum_read(None, None, None) == E
    assert L.rtw_accum_load(None, None, None, 0) == E
    assert L.rtw_accum_workspace_bytes(None, 20) == 0
    assert L.rtw_accum_world_workspace_bytes(None, C.byref(p), 20) == 0
    assert L.rtw_last_error()
    assert L.rtw_accum_destroy(None) == rtw.RTW_OK  # as the other destroy calls
    bad = rtw.make_params(1, 33, 50)
    assert L.rtw_accum_create(C.byref(bad), C.byref(h)) == E and not h.value
