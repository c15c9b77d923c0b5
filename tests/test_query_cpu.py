"""Ray queries, the part that needs no GPU (rtw_hip.h "ray queries"): the
exported symbols, the record layouts, and the host helper rtw_pixel_ray
against the guides' feature ray, bit for bit; then the conditions on the edge
sets of tests/test_gpu_query_edges.py, on the oracle's answers alone."""
import ctypes as C

import numpy as np
import pytest

import query_helpers as Q
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


# The edge sets of tests/test_gpu_query_edges.py (query_helpers.derive), on the oracle's answers alone:
# what each set must contain so that the device cannot pass it vacuously.
EDGE_WORLDS = ("scene1", "scene6", "scene7", "small", "spheres_image")


@pytest.fixture(scope="module")
def worlds(rtw, oracle):
    from rtw_amd import world as W

    def get(name):
        return Q.get_world(rtw, oracle, W, name)
    return get


@pytest.mark.parametrize("name", EDGE_WORLDS)
def test_big_batch_orders(worlds, name):
    w = worlds(name)
    rays, ref, kinds = Q.verified(w)
    assert not np.isnan(ref["t"]).any() and len(rays) == len(w.rays) - (1 if name == "scene6" else 0)
    n = 70 * 64 + 13
    idx = Q.big_index(kinds, ref, n, "random", 1)
    assert idx.min() >= 0 and idx.max() < len(rays) and set("abcd") <= set(kinds[idx])
    idx = Q.big_index(kinds, ref, n, "stragglers", 2)
    lane0 = np.arange(n) % 64 == 0
    assert idx.min() >= 0 and idx.max() < len(rays)
    assert np.isin(kinds[idx[lane0]], ("b", "c")).all() and (ref["prim"][idx[lane0]] > 0).all()
    assert (kinds[idx[~lane0]] == "d").all() and (ref["prim"][idx[~lane0]] == 0).all()
    assert (rays["t_max"][idx[~lane0]] == 1.0).all() and np.isinf(rays["t_max"][idx[lane0]]).all()


@pytest.mark.parametrize("name", ["scene1", "scene7"])
def test_times_outside_the_shutter(worlds, name):
    w = worlds(name)
    base = Q.words(w.ref)
    for time in Q.TIMES_OUTSIDE:
        rays, ref = w.derive("time", time)
        assert (rays["time"] == time).all() and not 0.0 <= time <= 1.0
        hit = ref["prim"] > 0
        assert np.isin(ref["prim"][hit] - 1, w.moving).sum() >= 10, (name, time)
        assert (Q.words(ref) != base).any(axis=1).sum() >= 30, (name, time)
    rays, ref = w.derive("time", "mixed")
    assert (rays["time"][1::2] == 1.5).all() and (rays["time"][0::2] == w.rays["time"][0::2]).all()
    assert (rays["time"][0::2] < 1.0).all()  # every pair of lanes holds both kinds
    assert (Q.words(ref) != base).any(axis=1)[1::2].sum() >= 10, name


@pytest.mark.parametrize("name", EDGE_WORLDS)
def test_interval_ends(worlds, name):
    w = worlds(name)
    rows = Q.finite_hits(w)
    assert len(rows) >= 300
    base, t = Q.words(w.ref[rows]), w.ref["t"][rows]
    for v in ("V1", "V2", "V3", "V4", "V5"):
        rays, ref = w.derive("interval", v)
        assert len(rays) == len(rows) and (rays["t_min"] <= rays["t_max"]).all() and not np.isnan(ref["t"]).any()
        same = (Q.words(ref) == base).all(axis=1)
        if v in ("V1", "V3", "V5"):  # a root equal to t_max, to t_min, to both: the same hit
            assert same.all(), (name, v, np.nonzero(~same)[0][:5])
        elif v == "V2":  # t_max just below the root: nothing nearer exists
            assert (ref["prim"] == 0).all(), (name, v)
        else:  # t_min just above it: never the same record, and often something behind
            assert not same.any() and (ref["prim"] > 0).mean() >= 0.20, (name, v, (ref["prim"] > 0).mean())
            assert (ref["t"][ref["prim"] > 0] > t[ref["prim"] > 0]).all()
    rays, ref = w.derive("plain")
    n = len(rays) // 3
    assert n >= 64 and (rays["t_min"][:n] == 0.0).all() and (rays["t_min"][n:2 * n] < 0.0).all()
    assert (rays["t_max"][2 * n:] == 1e300).all() and not np.isnan(ref["t"]).any()
    # t_min = 0 from a surface point meets the surface it starts on (|t| tiny); a negative t_min finds roots behind
    # the origin on the worlds that have something there (scene 6's rays start on the inside of a closed box)
    assert ((ref["prim"][:n] > 0) & (np.abs(ref["t"][:n]) < 1e-6)).sum() >= 32, name
    assert name == "scene6" or (ref["t"][n:2 * n] < 0.0).sum() >= 16, name
    assert Q.words(ref[2 * n:]).tobytes() == Q.words(w.ref[np.nonzero(np.isin(w.kinds, ("b", "c")))[0][:n]]).tobytes()


@pytest.mark.parametrize("name", ["scene1", "scene7", "small"])
def test_origin_scale_and_component_sets(rtw, worlds, name):
    from rtw_amd import world as W
    w = worlds(name)
    n_a = ((w.kinds == "a") & (w.ref["prim"] > 0)).sum()
    assert n_a >= 250
    for D in Q.FAR_D:
        rays, ref = w.derive("far", D)
        dist = np.sqrt((rays["origin"] ** 2).sum(axis=1))
        assert len(rays) == n_a and (dist > 0.9 * D - 2000.0).all() and not np.isnan(ref["t"]).any()
        assert (ref["prim"] > 0).mean() >= 0.5, (name, D)
        ex = np.log2(np.abs(rays["dir"]).max(axis=1))
        assert ex.min() < -30 and ex.max() > 30
        ends, eref = w.derive("far_ends", D)  # a root equal to t_max (and to t_min): the same record
        rows = Q.far_hit_rows(w, D)
        assert (ends["t_max"] == ref["t"][rows]).all() and (ends["t_min"][1::2] == ends["t_max"][1::2]).all()
        assert Q.words(eref).tobytes() == Q.words(ref[rows]).tobytes(), (name, D)
    rays, ref = w.derive("scaled")
    ex = np.log2(np.sqrt((rays["dir"] ** 2).sum(axis=1)))
    assert ((np.abs(ex) > 79.5) & (np.abs(ex) < 100.5)).all() and (ex > 0).any() and (ex < 0).any()
    assert (np.abs(rays["origin"]) < 2.0 ** 11).all()
    assert (ref["prim"] > 0).all(), name  # (a power of two scales every root exactly: the rays still hit)
    rays, ref = w.derive("axis")
    assert len(rays) == 6 * n_a and ((rays["dir"] == 0.0).sum(axis=1) == 2).all() and not np.isnan(ref["t"]).any()
    assert np.signbit(rays["dir"][rays["dir"] == 0.0]).any() and not np.signbit(rays["dir"][rays["dir"] == 0.0]).all()
    hit = ref["prim"] > 0
    assert hit.mean() >= 0.5, name
    if name == "small":
        kind = np.array([w.desc.prims[int(p) - 1].kind for p in ref["prim"][hit]])
        assert ((kind != W.PRIM_SPHERE) & (kind != W.PRIM_MOVING_SPHERE)).sum() >= 100
    rays, ref = w.derive("tiny")
    d = np.abs(rays["dir"])
    small = (d > 0.0) & (d < d.max(axis=1)[:, None] * 2.0 ** -60)
    assert len(rays) == 5 * n_a and (small.sum(axis=1) == 1).all()
    assert (ref["prim"] > 0).mean() >= 0.9 and not np.isnan(ref["t"]).any(), name
