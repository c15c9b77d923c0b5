"""Ray queries at the edges tests/test_gpu_query.py's batches of ~1,400 rays
never reach, every record against the oracle's rw_hit bit for
bit and every occlusion byte against it:

* batches larger than the device — 2 cap + 3*64 + 13 and cap + 1 rays, cap =
  8 * CUs * 256 the most threads that can be resident — so the grid-stride
  step of world_query_kernel / scene_query_kernel runs, and in
  world_query_lane_kernel a wave's second and third 64-ray blocks, the yield
  and the lane-level regeneration; in a random order and with one long walk
  next to 63 short ones in every block;
* times outside [0, 1] on a BVH over moving spheres (seq_times);
* t_max and t_min on the root and next to it (round_up, next_down);
* origins far outside the world (ray_margin), directions scaled by 2^-100 ..
  2^100, axis-aligned rays through rects and box faces under Translate /
  RotateY, components below 2^-60 of the largest (box_dir);
* two side streams at once, nothing synchronized between the fill, the query
  and the compare.

The sets and their conditions: tests/query_helpers.py, tests/test_query_cpu.py."""
import numpy as np
import pytest

import query_helpers as Q

pytestmark = pytest.mark.gpu

import torch  # noqa: E402  (device buffers and streams)


@pytest.fixture(scope="module")
def W():
    from rtw_amd import world
    return world


@pytest.fixture(scope="module")
def worlds(rtw, oracle, W):
    def get(name):
        return Q.get_world(rtw, oracle, W, name)
    return get


@pytest.fixture(scope="module")
def scene1_api(rtw):
    sph, mats, _ = rtw.cover_scene(42)
    sc = rtw.DeviceScene(sph, mats)
    yield sc
    sc.close()


def _target(worlds, scene1_api, name, asked, runs, rtw):
    """(world, query target, opts): a DeviceWorld with the traversal asked, or the scene API (asked "scene")."""
    w = worlds(name)
    if asked == "scene":
        return w, scene1_api, None
    opts = rtw.query_opts(asked)
    assert w.dev.query_info(opts)["traversal"] == runs
    return w, w.dev, opts


def _launch(target, d_rays, n, buf, opts, occluded, stream):
    f = target.occluded if occluded else target.trace
    if hasattr(target, "query_info"):  # a DeviceWorld; a DeviceScene takes no opts
        f(d_rays.data_ptr(), n, buf.data_ptr(), opts, stream)
    else:
        f(d_rays.data_ptr(), n, buf.data_ptr(), stream)


def _device_equal(target, d_rays, n, expect, opts, occluded, where):
    """n rays into a buffer pre-filled with 0xA5 with a 256-byte guard behind it; the records (int64 words) or
    the occlusion bytes compared with `expect` on the device.  Only the first differing rows come back."""
    size = n * (1 if occluded else 80)
    buf = torch.full((size + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    _launch(target, d_rays, n, buf, opts, occluded, torch.cuda.current_stream().cuda_stream)
    got = buf[:size] if occluded else buf[:size].view(torch.int64).view(n, 10)
    assert bool((buf[size:] == 0xA5).all()), (where, "guard")
    if not torch.equal(got, expect):
        bad = (got != expect).nonzero()[:, 0].unique()
        first = bad[:4]
        raise AssertionError((where, f"{bad.numel()} of {n} rows differ", first.cpu().numpy(),
                              got[first].cpu().numpy(), expect[first].cpu().numpy()))


def _host_equal(rtw, target, rays, ref, opts, where, is_world=True):
    """A small set as its own batch: records and occlusion bytes against the oracle's, guards intact."""
    n = len(rays)
    d_rays = Q.to_device(rays)
    got, guard = Q._trace(rtw, target, d_rays, n, opts, is_world=is_world)
    assert (guard == 0xA5).all(), where
    bad = np.nonzero((Q.words(got) != Q.words(ref)).any(axis=1))[0]
    assert bad.size == 0, (where, f"{bad.size} of {n} rows differ", bad[:5], got[bad[:2]], ref[bad[:2]])
    occ, guard = Q._trace(rtw, target, d_rays, n, opts, occluded=True, is_world=is_world)
    assert (guard == 0xA5).all(), where
    bad = np.nonzero(occ != (ref["prim"] > 0))[0]
    assert bad.size == 0, (where, f"occlusion: {bad.size} of {n} rows differ", bad[:5])


# ------------------------------------------- 1. batches larger than the device

BIG = [("scene6", "auto", "linear"), ("scene1", "union", "union"), ("scene1", "lane", "lane"),
       ("scene7", "union", "union"), ("scene7", "lane", "lane"), ("spheres_image", "lane", "lane"),
       ("small", "auto", "union"), ("scene1", "scene", None)]


@pytest.mark.parametrize("name,asked,runs", BIG, ids=[f"{c[0]}-{c[1]}" for c in BIG])
def test_batches_larger_than_the_device(rtw, worlds, scene1_api, name, asked, runs):
    w, target, opts = _target(worlds, scene1_api, name, asked, runs, rtw)
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    cap = 8 * cus * 256  # 2,048 resident threads per CU: no grid of 256-thread workgroups holds more
    assert w.dev.query_info(opts)["grid"] <= 8 * cus  # (the scene entries launch exactly min(ceil(n / 256), 8 CUs))
    rays, ref, kinds = Q.verified(w)
    hit = ref["prim"] > 0
    d_set = Q.to_device(rays).view(torch.float64).view(len(rays), 9)
    d_words = torch.from_numpy(Q.words(ref).view(np.int64).copy()).cuda()
    d_occ = torch.from_numpy(hit.astype(np.uint8)).cuda()
    for order in ("random", "stragglers"):
        for n in (2 * cap + 3 * 64 + 13, cap + 1):
            assert n > cap
            idx = Q.big_index(kinds, ref, n, order, 77)
            if order == "random":
                assert set("abcd") <= set(np.unique(kinds[idx]))
            else:
                lane0 = np.arange(n) % 64 == 0
                assert hit[idx[lane0]].all() and np.isin(kinds[idx[lane0]], ("b", "c")).all()
                assert not hit[idx[~lane0]].any() and (kinds[idx[~lane0]] == "d").all()
            d_idx = torch.from_numpy(idx).cuda()
            d_rays = d_set[d_idx].contiguous()
            where = (name, asked, order, n)
            _device_equal(target, d_rays, n, d_words[d_idx], opts, False, where)
            _device_equal(target, d_rays, n, d_occ[d_idx], opts, True, where)
            del d_idx, d_rays
    torch.cuda.synchronize()
    del d_set, d_words, d_occ
    torch.cuda.empty_cache()


# ------------------------------------------------- 2. times outside [0, 1]

TIMED = [("scene1", "union", "union"), ("scene1", "lane", "lane"), ("scene7", "union", "union"),
         ("scene7", "lane", "lane"), ("scene1", "scene", None)]


@pytest.mark.parametrize("name,asked,runs", TIMED, ids=[f"{c[0]}-{c[1]}" for c in TIMED])
def test_times_outside_the_shutter_equal_the_oracle(rtw, worlds, scene1_api, name, asked, runs):
    w, target, opts = _target(worlds, scene1_api, name, asked, runs, rtw)
    for time in (*Q.TIMES_OUTSIDE, "mixed"):
        rays, ref = w.derive("time", time)
        _host_equal(rtw, target, rays, ref, opts, (name, asked, "time", time), is_world=asked != "scene")


# ------------------------------------------------------- 3. interval ends

ENDS = [("scene1", "union", "union"), ("scene1", "lane", "lane"), ("scene7", "union", "union"),
        ("scene7", "lane", "lane"), ("scene6", "auto", "linear"), ("small", "auto", "union"),
        ("spheres_image", "lane", "lane")]


@pytest.mark.parametrize("name,asked,runs", ENDS, ids=[f"{c[0]}-{c[1]}" for c in ENDS])
def test_interval_ends_equal_the_oracle(rtw, worlds, scene1_api, name, asked, runs):
    """(What this cannot show: the direction in which the walks round the closest to f32.  The boxes' margin
    exceeds that rounding twentyfold for every ray)"""
    w, target, opts = _target(worlds, scene1_api, name, asked, runs, rtw)
    for v in ("V1", "V2", "V3", "V4", "V5"):
        rays, ref = w.derive("interval", v)
        _host_equal(rtw, target, rays, ref, opts, (name, asked, v))
    rays, ref = w.derive("plain")
    _host_equal(rtw, target, rays, ref, opts, (name, asked, "plain"))


# --------------------- 4. origins, direction scales and small components

SHAPES = [("scene1", "union", "union"), ("scene1", "lane", "lane"), ("scene7", "lane", "lane"),
          ("small", "auto", "union")]
SETS = [("far", 1e3), ("far", 1e5), ("far", 1e7), ("far_ends", 1e3), ("far_ends", 1e7), ("scaled",), ("axis",),
        ("tiny",)]
SET_IDS = ["far1e3", "far1e5", "far1e7", "far_ends1e3", "far_ends1e7", "scaled", "axis", "tiny"]


@pytest.mark.parametrize("name,asked,runs", SHAPES, ids=[f"{c[0]}-{c[1]}" for c in SHAPES])
@pytest.mark.parametrize("key", SETS, ids=SET_IDS)
def test_far_scaled_axis_and_tiny_rays_equal_the_oracle(rtw, worlds, scene1_api, name, asked, runs, key):
    w, target, opts = _target(worlds, scene1_api, name, asked, runs, rtw)
    rays, ref = w.derive(*key)  # each set a batch of its own: no lane's box tests can lean on a neighbour's
    _host_equal(rtw, target, rays, ref, opts, (name, asked, key))


# ------------------------------------------------------- 5. a side stream

def test_two_side_streams_at_once(rtw, worlds):
    w = worlds("scene7")
    opts = rtw.query_opts("lane")
    assert w.dev.query_info(opts)["traversal"] == "lane"
    rays, ref, _ = Q.verified(w)
    n = 40 * len(rays) + 5
    d_idx = torch.from_numpy(np.random.default_rng(3).integers(0, len(rays), n)).cuda()
    d_rays = Q.to_device(rays).view(torch.float64).view(len(rays), 9)[d_idx].contiguous()
    e_words = torch.from_numpy(Q.words(ref).view(np.int64).copy()).cuda()[d_idx]
    e_occ = torch.from_numpy((ref["prim"] > 0).astype(np.uint8)).cuda()[d_idx]
    torch.cuda.synchronize()
    verdict = []
    for occluded, expect in ((False, e_words), (True, e_occ)):
        s = torch.cuda.Stream()
        assert s.cuda_stream != torch.cuda.default_stream().cuda_stream
        size = n * (1 if occluded else 80)
        with torch.cuda.stream(s):
            # work ahead of the fill: a query launched on another stream would run first and be overwritten
            busy = torch.ones(1 << 26, dtype=torch.float32, device="cuda")
            for _ in range(16):
                busy.mul_(1.0001)
            buf = torch.empty(size + 256, dtype=torch.uint8, device="cuda")
            buf.fill_(0xA5)
            _launch(w.dev, d_rays, n, buf, opts, occluded, s.cuda_stream)
            got = buf[:size] if occluded else buf[:size].view(torch.int64).view(n, 10)
            verdict.append(((got == expect).all() & (buf[size:] == 0xA5).all(), s, buf, busy))
    for ok, s, _, _ in verdict:  # the first synchronisation
        s.synchronize()
    assert [bool(v[0]) for v in verdict] == [True, True]
