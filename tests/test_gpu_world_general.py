"""The world kernel's BVH on MIXED worlds, and the kernel at its parameter
edges: the BVH counterpart of test_gpu_world.py, whose worlds with rects,
boxes, transform chains, lights or noise all hold <= 32 primitives and so run
the linear loop, and whose BVH worlds are spheres only.

helpers.mixed_bvh_world builds worlds of ~120 primitives (leaves of up to 2)
and >= 512 (leaves of 1; the depth-capped rebuild runs) that hold every
primitive kind, chains of 1-4 Translate / RotateY ops in both orders,
moving spheres with their own time ranges, negative radii, every material and
texture, and three COINCIDENT pairs of lights whose list indices lie far apart
(the tie rule of accept(): the later list index wins, in tree order too); and
three reduced variants, so that every compiled feature set meets a BVH.
tests/test_world_cpu.py shows on the oracle alone that every class is visible.

  * BVH == linear, bit for bit (rgb, the f32 mean, samples, segments), under
    every traversal, feature set and register budget;
  * what rtw_world_launch_info reports for a forced per-lane walk;
  * against oracle.TableWorld Tier B (the linear CPU restatement), bar as
    test_gpu_parity.assert_parity (observed: max|d| 0, frac_exact 1.0);
  * the tie rule, under linear / union / lane;
  * rtw_params edges on the Cornell box (scene 6: the linear loop) and the
    small mixed world (BVH): max_depth 0-3, units longer than the tail
    dealing's 32-entry ring, frames of fewer units than lanes, row shards,
    64-bit seeds, the camera shutter.
"""
import numpy as np
import pytest

from helpers import MIXED_CAMERA, MIXED_SIZES, _to_desc, diff_stats, mixed_bvh_world, to_oracle_camera
from test_gpu_parity import SEEDS, assert_parity

pytestmark = pytest.mark.gpu

SKY, BLACK = (0.7, 0.8, 1.0), (0.0, 0.0, 0.0)
GEN_SEED = 5  # mixed_bvh_world's seed (as tests/test_world_cpu.py)
# name -> (n_boxes, n_spheres, variant)
WORLDS = {"small": (*MIXED_SIZES["small"], None), "large": (*MIXED_SIZES["large"], None),
          "rects": (7, 0, "rects"), "spheres_xform": (0, 60, "spheres_xform"),
          "spheres_image": (0, 520, "spheres_image")}
SPHERES_ONLY = {"spheres_image"}


@pytest.fixture(scope="module")
def W():
    from rtw_amd import world
    return world


@pytest.fixture(scope="module")
def earth(W):
    return W.earth_map()


class Mixed:
    """One mixed world: its tables, the product's desc and the oracle's world."""

    def __init__(self, W, oracle, earth, name, swap):
        nb, ns, variant = WORLDS[name]
        self.name, self.swap = name, swap
        self.tables = mixed_bvh_world(W, earth, nb, ns, GEN_SEED, swap=swap, variant=variant)
        self.desc, self._keep = _to_desc(W, *self.tables)
        self.oracle = oracle.TableWorld(*self.tables, background=SKY)
        self._ref = {}

    def ref(self, ocam, w, h, spp, bg=SKY, **kw):
        """Oracle Tier B (rendered once per argument set, never modified)."""
        cam_key = (ocam.time0, ocam.time1)
        key = (cam_key, w, h, spp, bg, tuple(sorted(kw.items())))
        if key not in self._ref:
            img = self.oracle.render_tier_b(ocam, w, h, spp, bg=bg, threads=16, **kw)[0]
            img.setflags(write=False)
            self._ref[key] = img
        return self._ref[key]


@pytest.fixture(scope="module")
def mixed(W, oracle, earth):
    cache = {}

    def get(name, swap=False):
        if (name, swap) not in cache:
            cache[(name, swap)] = Mixed(W, oracle, earth, name, swap)
        return cache[(name, swap)]
    return get


def mixed_camera(rtw, time0=0.0, time1=1.0, aspect=16 / 9):
    m = MIXED_CAMERA
    return rtw.camera_init(m["look_from"], m["look_at"], (0, 1, 0), m["vfov"], aspect, m["aperture"], m["focus"],
                           time0, time1)


@pytest.fixture(scope="module")
def cam(rtw, oracle):
    c = mixed_camera(rtw)
    return c, to_oracle_camera(oracle, c)


class Dev:
    """A DeviceWorld with the _render_dev pattern of test_gpu_world.py: device
    buffers, the caller's workspace (with or without the tail dealing's rings)."""

    def __init__(self, W, desc, linear=False):
        self.dw = W.DeviceWorld(desc, linear=linear)

    def render(self, rtw, cam, p, rings=True, counts=True):
        import torch
        need = self.dw.workspace_bytes(p) if rings else rtw.workspace_bytes(p)
        ws = torch.empty(need + 256, dtype=torch.uint8, device="cuda:0")
        ptr = (ws.data_ptr() + 255) & ~255
        rgb = torch.empty((p.row_count, p.width, 3), dtype=torch.uint8, device="cuda:0")
        mean = torch.empty((p.row_count, p.width, 3), dtype=torch.float32, device="cuda:0")
        self.dw.render_async(cam, p, ptr, need, rgb.data_ptr(), mean.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        c = self.dw.counts(cam, p, ptr, need) if counts else None
        return rgb.cpu().numpy(), mean.cpu().numpy(), c

    def close(self):
        self.dw.close()


def assert_same(a, b, what):
    (ra, ma, ca), (rb, mb, cb) = a, b
    assert (ra == rb).all(), (what, diff_stats(ra, rb))
    assert np.array_equal(ma.view(np.uint32), mb.view(np.uint32)), what
    assert ca["samples"] == cb["samples"] and ca["segments"] == cb["segments"], (what, ca, cb)


# ------------------------------------------------------------ BVH == linear ----
@pytest.mark.parametrize("name,swap", [("small", False), ("small", True), ("large", False), ("large", True),
                                       ("rects", False), ("spheres_xform", False), ("spheres_image", False)])
def test_mixed_bvh_equals_linear(rtw, W, mixed, cam, name, swap):
    """The BVH render (union walk of a world with transformed leaves, rects,
    mixed pretest-eligible / ineligible leaves, coincident primitives) equals
    the linear loop's bit for bit — rgb, the f32 mean, samples, segments —
    under every traversal request, both feature sets, and (small) every
    register budget."""
    m = mixed(name, swap)
    gcam = cam[0]
    w, h, spp = 128, 72, 8
    lin, bvh = Dev(W, m.desc, linear=True), Dev(W, m.desc)
    try:
        info = bvh.dw.bvh_info()
        assert lin.dw.bvh_info()["nodes"] == 0 and info["nodes"] > 0, info
        if name == "small":
            assert info["max_leaf"] == 2, info
        if name in ("large", "spheres_image"):
            assert info["max_leaf"] == 1 and m.desc.n_prims >= 512, info
        assert info["max_depth"] <= 32, info
        ref = lin.render(rtw, gcam, rtw.make_params(w, h, spp, background=SKY))
        assert ref[2]["samples"] == w * h * spp and ref[0].std() > 5
        waves = (0, 1, 3, 4) if name == "small" else (0,)
        for trav in ("auto", "union", "lane"):
            for feat in ("auto", "all"):
                for wv in waves:
                    if wv and (trav, feat) != ("auto", "auto"):
                        continue
                    p = rtw.make_params(w, h, spp, background=SKY, world_traversal=trav, world_features=feat,
                                        world_waves=wv)
                    got = bvh.render(rtw, gcam, p)
                    what = f"{name} swap {swap} traversal {trav} features {feat} waves {wv}"
                    assert_same(got, ref, what)
                    assert got[2]["prim_tests"] < ref[2]["prim_tests"], (what, got[2], ref[2])
                    # (the per-lane walk is compiled for the spheres-only feature set alone)
                    want = "lane" if (name in SPHERES_ONLY and trav != "union" and feat == "auto") else "union"
                    assert got[2]["traversal"] == want, (what, got[2])
        print(name, swap, info, "prim tests bvh / linear", got[2]["prim_tests"], ref[2]["prim_tests"],
              "max|d| 0 frac_exact 1.0")
    finally:
        lin.close()
        bvh.close()


@pytest.mark.parametrize("name", list(WORLDS))
def test_mixed_traversal_reporting(rtw, W, mixed, cam, name):
    """rtw_world_launch_info with world_traversal = lane: a world that is not
    spheres only reports (and runs) the union walk; the spheres-only >= 512
    variant reports lane, its walk's own iteration count is > 0, and its image
    equals the union walk's and the linear loop's."""
    m = mixed(name)
    bvh = Dev(W, m.desc)
    try:
        p = rtw.make_params(128, 72, 8, background=SKY, world_traversal="lane")
        li = bvh.dw.launch_info(p)
        if name not in SPHERES_ONLY:
            assert li["traversal"] == "union", li
            return
        assert li["traversal"] == "lane", li
        lane = bvh.render(rtw, cam[0], p)
        assert lane[2]["traversal"] == "lane" and lane[2]["lane_interior_iters"] > 0, lane[2]
        pu = rtw.make_params(128, 72, 8, background=SKY, world_traversal="union")
        union = bvh.render(rtw, cam[0], pu)
        assert union[2]["traversal"] == "union" and union[2]["lane_interior_iters"] == 0, union[2]
        lin = Dev(W, m.desc, linear=True)
        try:
            linear = lin.render(rtw, cam[0], pu)
        finally:
            lin.close()
        assert_same(lane, union, "lane vs union")
        assert_same(lane, linear, "lane vs linear")
    finally:
        bvh.close()


# ------------------------------------------------------- against the oracle ----
@pytest.mark.parametrize("bg", [SKY, BLACK])
@pytest.mark.parametrize("name", ["small", "large"])
def test_mixed_world_equals_oracle(rtw, W, mixed, cam, name, bg):
    m = mixed(name)
    g = W.render_world(cam[0], m.desc, rtw.make_params(128, 72, 8, background=bg))
    assert_parity(g, m.ref(cam[1], 128, 72, 8, bg=bg), f"mixed {name} bg {bg}")
    assert g.std() > 5


@pytest.mark.parametrize("name,mode", [("small", "linear"), ("small", "union"), ("large", "linear"), ("large", "union"),
                                       ("spheres_image", "linear"), ("spheres_image", "union"),
                                       ("spheres_image", "lane")])
def test_tie_rule_later_index_wins(rtw, W, mixed, cam, name, mode):
    """Coincident primitives (helpers.PAIR_COLOURS): on t == h.t the later list
    index wins (accept(), as the reference's sequential HittableList.hit) — in
    a BVH the two are met in tree order.  The world and its pair-swapped twin
    each equal their own oracle render and differ from each other, under the
    linear loop, the union walk and the per-lane walk."""
    outs = []
    for swap in (False, True):
        m = mixed(name, swap)
        d = Dev(W, m.desc, linear=mode == "linear")
        try:
            p = rtw.make_params(128, 72, 8, background=SKY, world_traversal="auto" if mode == "linear" else mode)
            rgb, _, c = d.render(rtw, cam[0], p)
        finally:
            d.close()
        assert c["traversal"] == mode, c
        assert_parity(rgb, m.ref(cam[1], 128, 72, 8), f"tie {name} {mode} swap {swap}")
        outs.append(rgb)
    changed = float((outs[0] != outs[1]).any(axis=2).mean())
    print(name, mode, "pixels the pair order changes:", changed)
    assert changed >= 0.02  # the pairs cover far more (tests/test_world_cpu.py)


# ------------------------------------------- the kernel at its parameter edges ----
class Cornell:
    """Scene 6 (rects, transforms, a light, black background; 18 primitives: the linear loop)."""
    name = "cornell"

    def __init__(self, W, oracle):
        self.b = W.BuiltScene(6, 42)
        self.desc = self.b.desc
        self.o = oracle.OracleWorld(6, 42)
        self.bg = self.b.background
        self._ref = {}

    def ref(self, ocam, w, h, spp, bg=None, **kw):
        key = ((ocam.time0, ocam.time1), w, h, spp, tuple(sorted(kw.items())))
        if key not in self._ref:
            img = self.o.render_tier_b(ocam, w, h, spp, threads=16, **kw)[0]
            img.setflags(write=False)
            self._ref[key] = img
        return self._ref[key]


@pytest.fixture(scope="module")
def edge_world(rtw, W, oracle, mixed, cam):
    """name -> (world with .desc / .ref, product camera, oracle camera, background)."""
    cornell = Cornell(W, oracle)
    ccam = cornell.b.camera()

    def get(name):
        if name == "cornell":
            return cornell, ccam, to_oracle_camera(oracle, ccam), cornell.bg
        return mixed("small"), cam[0], cam[1], SKY
    return get


EDGE_WORLDS = ["cornell", "small"]


@pytest.mark.parametrize("depth", [0, 1, 2, 3])
@pytest.mark.parametrize("name", EDGE_WORLDS)
def test_world_max_depth_edges(rtw, W, edge_world, name, depth):
    """The world kernel adds emission forward (rad += T * emitted) and has its
    own end-of-path rule: depths 0-3 against the oracle; depth 0 is black."""
    m, gcam, ocam, bg = edge_world(name)
    g = W.render_world(gcam, m.desc, rtw.make_params(128, 72, 8, max_depth=depth, background=bg))
    assert_parity(g, m.ref(ocam, 128, 72, 8, bg=bg, depth=depth), f"{name} depth {depth}")
    if depth == 0:
        assert (g == 0).all()
    else:
        assert g.any()


@pytest.mark.parametrize("spp,chunk", [(1, 0), (19, 0), (21, 0), (7, 1), (40, 33), (100, 64), (70, 70)])
@pytest.mark.parametrize("w,h", [(40, 40), (37, 23)])
@pytest.mark.parametrize("name", EDGE_WORLDS)
def test_world_spp_chunk_edges(rtw, W, edge_world, name, w, h, spp, chunk):
    """Units of 1 sample, one short of / one past the default chunk, and units
    LONGER than the tail dealing's ring (kTailWin = 32 entries per lane,
    indexed modulo), on whole tiles (40x40) and partial ones (37x23).  Tail
    dealing ran (rtw_world_render_counts_ex); for chunk > 32 a render without
    the rings (a workspace of rtw_workspace_bytes only) gives the same bytes."""
    m, gcam, ocam, bg = edge_world(name)
    p = rtw.make_params(w, h, spp, background=bg, chunk=chunk)
    d = Dev(W, m.desc)
    try:
        rgb, mean, c = d.render(rtw, gcam, p)
        assert c["tail_dealing"] and c["samples"] == w * h * spp, c
        assert_parity(rgb, m.ref(ocam, w, h, spp, bg=bg, chunk=chunk), f"{name} {w}x{h}x{spp} chunk {chunk}")
        if chunk > 32:
            rgb2, mean2, c2 = d.render(rtw, gcam, p, rings=False)
            assert not c2["tail_dealing"], c2
            assert (rgb2 == rgb).all() and np.array_equal(mean2.view(np.uint32), mean.view(np.uint32))
            assert c2["samples"] == c["samples"] and c2["segments"] == c["segments"]
    finally:
        d.close()


@pytest.mark.parametrize("w,h", [(2, 2), (9, 3), (65, 2)])
@pytest.mark.parametrize("name", EDGE_WORLDS)
def test_world_tiny_frames(rtw, W, edge_world, name, w, h):
    """2 is the smallest width / height validate accepts; these frames give
    fewer units than one wave has lanes, or a single partial tile."""
    m, gcam, ocam, bg = edge_world(name)
    g = W.render_world(gcam, m.desc, rtw.make_params(w, h, 8, background=bg))
    assert_parity(g, m.ref(ocam, w, h, 8, bg=bg), f"{name} {w}x{h}x8")


@pytest.mark.parametrize("name", EDGE_WORLDS)
def test_world_row_shards(rtw, W, edge_world, name):
    """row_begin / row_stride / row_count with rtw_world_*: every shard of
    strides 2, 3 and 8 equals full[r::s]; a shorter row_count, its prefix."""
    m, gcam, ocam, bg = edge_world(name)
    w, h = 120, 68
    full = W.render_world(gcam, m.desc, rtw.make_params(w, h, 8, background=bg))
    assert_parity(full, m.ref(ocam, w, h, 8, bg=bg), f"{name} {w}x{h}x8")
    for s in (2, 3, 8):
        for r in range(s):
            part = W.render_world(gcam, m.desc, rtw.make_params(w, h, 8, background=bg, row_begin=r, row_stride=s))
            assert part.shape[0] == len(range(r, h, s)) and (part == full[r::s]).all(), (s, r)
        short = W.render_world(gcam, m.desc, rtw.make_params(w, h, 8, background=bg, row_begin=s - 1, row_stride=s,
                                                             row_count=3))
        assert (short == full[s - 1::s][:3]).all(), s
    o = m.ref(ocam, w, h, 8, bg=bg, row_begin=1, row_stride=3, row_count=5)
    assert_parity(full[1::3][:5], o, f"{name} oracle rows 1::3 x5")


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", EDGE_WORLDS)
def test_world_seeds(rtw, W, edge_world, name, seed):
    """rtw_params.seed is a uint64 (every other world render uses 42): zero,
    its low and high words, all ones; 2^32 + 5 is not seed 5."""
    m, gcam, ocam, bg = edge_world(name)
    g = W.render_world(gcam, m.desc, rtw.make_params(48, 27, 4, seed=seed, background=bg))
    assert_parity(g, m.ref(ocam, 48, 27, 4, bg=bg, seed=seed), f"{name} seed {seed}")
    if seed == 2**32 + 5:
        low = W.render_world(gcam, m.desc, rtw.make_params(48, 27, 4, seed=5, background=bg))
        assert_parity(low, m.ref(ocam, 48, 27, 4, bg=bg, seed=5), f"{name} seed 5")
        assert (g != low).mean() > 0.1  # another stream (the oracle's two frames differ in 0.19 / 0.70 of the channels)


@pytest.mark.parametrize("t0,t1", [(0.25, 0.75), (0.5, 0.5)])
def test_world_shutter_inside_unit_interval(rtw, W, oracle, mixed, t0, t1):
    m = mixed("small")
    gcam = mixed_camera(rtw, t0, t1)
    g = W.render_world(gcam, m.desc, rtw.make_params(128, 72, 8, background=SKY))
    assert_parity(g, m.ref(to_oracle_camera(oracle, gcam), 128, 72, 8), f"small shutter [{t0}, {t1}]")


def test_world_shutter_outside_unit_interval(rtw, W, oracle, mixed):
    """The BVH boxes of moving spheres cover shutter times [0, 1]: a camera
    with [-0.5, 1.5] is refused for the BVH (RTW_UNSUPPORTED, the only refusal
    of a world launch that depends on the camera); the same world created
    linear renders it and equals the oracle."""
    m = mixed("small")
    gcam = mixed_camera(rtw, -0.5, 1.5)
    p = rtw.make_params(128, 72, 8, background=SKY)
    with pytest.raises(rtw.RtwError) as e:
        W.render_world(gcam, m.desc, p)
    assert e.value.status == rtw.RTW_UNSUPPORTED, e.value
    d = Dev(W, m.desc)
    try:
        with pytest.raises(rtw.RtwError) as e:
            d.render(rtw, gcam, p, counts=False)
        assert e.value.status == rtw.RTW_UNSUPPORTED, e.value
    finally:
        d.close()
    lin = Dev(W, m.desc, linear=True)
    try:
        rgb, _, c = lin.render(rtw, gcam, p)
    finally:
        lin.close()
    assert c["traversal"] == "linear"
    assert_parity(rgb, m.ref(to_oracle_camera(oracle, gcam), 128, 72, 8), "small linear, shutter [-0.5, 1.5]")
