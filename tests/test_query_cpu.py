"""Ray queries, the part that needs no GPU (rtw_hip.h "ray queries"): the
exported symbols, the record layouts, and the host helper rtw_pixel_ray
against the guides' feature ray, bit for bit."""
import ctypes as C

import numpy as np
import pytest

from denoise_helpers import feature_ray

QUERY_SYMBOLS = ["rtw_pixel_ray", "rtw_world_trace_device", "rtw_world_occluded_device", "rtw_scene_trace_device",
                 "rtw_scene_occluded_device", "rtw_world_trace", "rtw_scene_trace", "rtw_world_query_info"]


def test_query_symbols_declared_and_exported(rtw):
    declared = rtw.header_symbols()
    for s in QUERY_SYMBOLS:
        assert s in declared, s
        assert hasattr(rtw.lib(), s), s
    assert rtw.abi_version() == 4  # new entries alone do not bump it


def test_record_layouts(rtw):
    assert C.sizeof(rtw.Ray) == 72 and C.sizeof(rtw.Hit) == 80 and C.sizeof(rtw.QueryOpts) == 8
    assert rtw.RAY_DTYPE.itemsize == 72 and rtw.HIT_DTYPE.itemsize == 80
    ray_off = {n: rtw.RAY_DTYPE.fields[n][1] for n in rtw.RAY_DTYPE.names}
    assert ray_off == {"origin": 0, "dir": 24, "time": 48, "t_min": 56, "t_max": 64}
    hit_off = {n: rtw.HIT_DTYPE.fields[n][1] for n in rtw.HIT_DTYPE.names}
    assert hit_off == {"t": 0, "p": 8, "normal": 32, "u": 56, "v": 64, "prim": 72, "front": 76}
    for name, off in ray_off.items():
        assert getattr(rtw.Ray, name).offset == off, name
    for name, off in hit_off.items():
        assert getattr(rtw.Hit, name).offset == off, name


def _bits(x):
    return np.array(x, np.float64).view(np.uint64).tolist()


@pytest.mark.parametrize("W,H", [(24, 14), (60, 33)])
def test_pixel_ray_is_the_guides_feature_ray(rtw, W, H):
    cam = rtw.camera_init((13, 2, 3), (0.5, 0.25, -0.125), (0, 1, 0), 20.0, W / H, 0.1, 9.7, 0.125, 0.875)
    pixels = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 3, H // 2), (W - 5, 3)]
    for x, y in pixels:
        r = rtw.pixel_ray(cam, W, H, x, y)
        o, d, time = feature_ray(cam, W, H, x, y)
        assert _bits(list(r.origin)) == _bits(o), (x, y)
        assert _bits(list(r.dir)) == _bits(d), (x, y)
        assert _bits(r.time) == _bits(time), (x, y)
        assert r.t_min == 0.001 and r.t_max == np.inf


def test_pixel_ray_rejects_bad_arguments(rtw):
    cam = rtw.cover_camera(16 / 9)
    L, r = rtw.lib(), rtw.Ray()
    assert L.rtw_pixel_ray(C.byref(cam), 24, 14, 23, 13, C.byref(r)) == rtw.RTW_OK
    assert L.rtw_pixel_ray(C.byref(cam), 24, 14, 24, 0, C.byref(r)) == rtw.RTW_EINVAL   # x >= width
    assert L.rtw_pixel_ray(C.byref(cam), 24, 14, 0, 14, C.byref(r)) == rtw.RTW_EINVAL   # y >= height
    assert L.rtw_pixel_ray(C.byref(cam), 1, 14, 0, 0, C.byref(r)) == rtw.RTW_EINVAL     # width < 2
    assert L.rtw_pixel_ray(C.byref(cam), 24, 1, 0, 0, C.byref(r)) == rtw.RTW_EINVAL     # height < 2
    assert L.rtw_pixel_ray(None, 24, 14, 0, 0, C.byref(r)) == rtw.RTW_EINVAL
    assert L.rtw_pixel_ray(C.byref(cam), 24, 14, 0, 0, None) == rtw.RTW_EINVAL
    with pytest.raises(rtw.RtwError):
        rtw.pixel_ray(cam, 24, 14, 24, 0)
