"""Ray queries on the GPU (rtw_hip.h "ray queries"): closest hit
and occlusion of caller-supplied rays over worlds and scenes, against the
oracle's rw_hit (OracleWorld.hit / TableWorld.hit) bit for bit — records are
compared as uint64 words, no tolerance, no ray left out.

Worlds: scene 6 (linear loop, rects, boxes under Translate / RotateY), 5
(rects + spheres), 4 with the synthetic map (sphere uv), 3, scene 1 as a world
(a BVH; moving spheres) and scene 7 (9,982 primitives) with the union and the
per-lane walk, helpers.mixed_bvh_world "small" and its swap twin (every kind,
chains, negative radii, coincident pairs; union walk) and "spheres_image" (520
spheres; both walks).  Ray sets: tests/query_helpers.py (feature rays with
their own times, bounces, inward rays, shadow rays with t_max = 1), plus for
scene 6 axis-aligned rays and one ray lying in a rect's plane (a 0/0 root),
and for the mixed worlds rays aimed at each coincident pair."""
import ctypes as C

import numpy as np
import pytest

import query_helpers as Q
from helpers import MIXED_CAMERA, MIXED_SIZES, _to_desc, chain_to_world, mixed_bvh_world

pytestmark = pytest.mark.gpu

import torch  # noqa: E402  (device buffers and streams)

SKY = (0.7, 0.8, 1.0)
GEN_SEED = 5  # mixed_bvh_world's seed (as tests/test_gpu_world_general.py)
MIXED = {"small": (*MIXED_SIZES["small"], None, False, 100), "small_swap": (*MIXED_SIZES["small"], None, True, 100),
         "spheres_image": (0, 520, "spheres_image", False, 101)}
# (world, traversal asked, traversal rtw_world_query_info must report)
CASES = [("scene6", "auto", "linear"), ("scene6", "lane", "linear"), ("scene5", "auto", "linear"),
         ("scene4", "auto", "linear"), ("scene3", "auto", "linear"),
         ("scene1", "union", "union"), ("scene1", "lane", "lane"), ("scene7", "union", "union"),
         ("scene7", "lane", "lane"), ("small", "auto", "union"), ("small", "lane", "union"),
         ("small_swap", "auto", "union"), ("spheres_image", "union", "union"), ("spheres_image", "lane", "lane")]
SIZES = (1, 63, 64, 65, 257)


@pytest.fixture(scope="module")
def W():
    from rtw_amd import world
    return world


def _pair_rays(W, tables, look_from, rng):
    """For each coincident-pair class of a mixed world, rays aimed at the pair: from the camera origin and
    from one unit in front of its surface.  Returns (rows, [(class, later list index, [row indices])])."""
    prims, xf = tables[0], tables[1]
    rows, want = [], []
    for cls in ("pair_rect", "pair_sphere", "pair_face"):
        idx = [i for i, p in enumerate(prims) if p["cls"] == cls]
        if not idx:
            continue
        first = prims[idx[0]]
        same = [i for i in idx if (prims[i]["kind"], list(prims[i]["a"]), prims[i]["xform"]) ==
                (first["kind"], list(first["a"]), first["xform"])]
        assert len(same) >= 2, cls
        a = first["a"]
        if first["kind"] == W.PRIM_SPHERE:
            c, r = np.array(a[0:3]), a[6]
            to_cam = np.array(look_from) - c
            to_cam /= np.sqrt((to_cam * to_cam).sum())
            centre, front = c + r * to_cam, c + (r + 1.0) * to_cam
        else:  # an XY rect, facing +z in its object space
            mid = np.array([(a[0] + a[1]) / 2, (a[2] + a[3]) / 2, a[4]])
            centre, front = mid, mid + np.array([0.0, 0.0, 1.0])
            if first["xform"] >= 0:
                centre, front = chain_to_world(xf[first["xform"]], centre), chain_to_world(xf[first["xform"]], front)
        mine = []
        for o in (np.array(look_from, float), front):
            mine.append(len(rows))
            rows.append((o, centre - o, float(rng.random()), 0.001, np.inf))
        want.append((cls, max(same), mine))
    return rows, want


class World:
    """One world: the device's, the oracle's, the ray set and the oracle's records (computed once, read-only)."""

    def __init__(self, rtw, oracle, W, name):
        self.name = name
        self.pairs, extra = [], []
        if name.startswith("scene"):
            sid = int(name[5:])
            img = W.synthetic_world_map() if sid in (4, 7) else None
            self.built = W.BuiltScene(sid, 42, img)
            self.desc = self.built.desc
            self.oracle = oracle.OracleWorld(sid, 42, img)
            cam = self.built.camera(Q.QW / Q.QH)
            look_from, seed = tuple(self.built.settings.look_from), 1234 + sid
            self.moving = [i for i in range(self.desc.n_prims) if self.desc.prims[i].kind == W.PRIM_MOVING_SPHERE]
            if sid == 6:  # direction components exactly 0, from inside the box; then the ray in the back wall's plane
                rng = np.random.default_rng(99)
                for o in ((278.0, 278.0, 10.0), (100.0, 400.0, 300.0), (500.0, 50.0, 540.0)):
                    for d in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1)):
                        extra.append((o, tuple(float(x) for x in d), float(rng.random()), 0.001, np.inf))
                extra.append(((100.0, 100.0, 555.0), (1.0, 0.5, 0.0), 0.5, 0.001, np.inf))
        else:
            nb, ns, variant, swap, k = MIXED[name]
            self.tables = mixed_bvh_world(W, W.earth_map(), nb, ns, GEN_SEED, swap=swap, variant=variant)
            self.desc, self._keep = _to_desc(W, *self.tables)
            self.oracle = oracle.TableWorld(*self.tables, background=SKY)
            m = MIXED_CAMERA
            cam = rtw.camera_init(m["look_from"], m["look_at"], (0, 1, 0), m["vfov"], Q.QW / Q.QH, m["aperture"],
                                  m["focus"], 0.0, 1.0)
            look_from, seed = m["look_from"], 1234 + k
            self.moving = []
            extra, self.pairs = _pair_rays(W, self.tables, look_from, np.random.default_rng(7))
        rays, kinds = Q.ray_set(rtw, self.oracle, cam, look_from, seed)
        self.n_main = len(rays)
        if extra:
            rays = np.concatenate([rays, Q.make_rays(rtw, extra)])
            kinds = np.concatenate([kinds, np.array(["x"] * len(extra))])
        self.rays, self.kinds = rays, kinds
        self.ref = Q.oracle_hits(rtw, self.oracle, rays)
        self.rays.setflags(write=False)
        self.ref.setflags(write=False)
        self._W, self._dev, self._d_rays = W, None, None

    @property
    def dev(self):
        if self._dev is None:
            self._dev = self._W.DeviceWorld(self.desc)
        return self._dev

    @property
    def d_rays(self):
        if self._d_rays is None:
            self._d_rays = torch.from_numpy(np.frombuffer(self.rays.tobytes(), np.uint8).copy()).cuda()
        return self._d_rays


@pytest.fixture(scope="module")
def worlds(rtw, oracle, W):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = World(rtw, oracle, W, name)
        return cache[name]
    return get


def _trace(rtw, target, d_rays, n, opts=None, occluded=False, is_world=True):
    """n rays through the pointer API into a buffer pre-filled with 0xA5, with a 256-byte guard behind
    the last record (or byte).  Returns (records or bytes, guard)."""
    size = n * (1 if occluded else 80)
    buf = torch.full((size + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    f = target.occluded if occluded else target.trace
    if is_world:
        f(d_rays.data_ptr(), n, buf.data_ptr(), opts, stream)
    else:
        f(d_rays.data_ptr(), n, buf.data_ptr(), stream)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    out = host[:size].copy()
    return (out if occluded else out.view(rtw.HIT_DTYPE)), host[size:]


def _assert_records(got, ref, where):
    """Bit for bit, except a record whose oracle root is NaN (a ray in a rect's plane): prim, and t NaN on both sides."""
    nan = np.isnan(ref["t"])
    assert (got["prim"] == ref["prim"]).all(), where
    assert np.isnan(got["t"][nan]).all(), where
    gw, rw = Q.words(got)[~nan], Q.words(ref)[~nan]
    bad = np.nonzero((gw != rw).any(axis=1))[0]
    assert bad.size == 0, (where, bad[:5], got[~nan][bad[:2]], ref[~nan][bad[:2]])


def test_ray_sets_cannot_pass_vacuously(worlds):
    for name in ("scene1", "scene3", "scene4", "scene5", "scene6", "scene7", "small", "small_swap", "spheres_image"):
        w = worlds(name)
        main = slice(0, w.n_main)
        Q.check_conditions(w.rays[main], w.kinds[main], w.ref[main], w.moving if name in ("scene1", "scene7") else None)
        assert np.isnan(w.ref["t"]).sum() == (1 if name == "scene6" else 0), name
    w = worlds("scene6")
    assert (w.ref["prim"][w.kinds == "x"] > 0).all()  # the axis-aligned rays start inside the box: all hit
    assert (w.rays["dir"][w.kinds == "x"] == 0.0).any(axis=1).all()


@pytest.mark.parametrize("name,asked,runs", CASES, ids=[f"{c[0]}-{c[1]}" for c in CASES])
def test_trace_and_occluded_equal_the_oracle(rtw, worlds, name, asked, runs):
    w = worlds(name)
    opts = rtw.query_opts(asked)
    assert w.dev.query_info(opts)["traversal"] == runs
    n_all = len(w.rays)
    first = None
    for n in (*SIZES, n_all, n_all):  # prefixes of the same set; the full set twice
        got, guard = _trace(rtw, w.dev, w.d_rays, n, opts)
        assert (guard == 0xA5).all(), (name, n)
        _assert_records(got, w.ref[:n], (name, asked, n))
        if n == n_all:
            if first is None:
                first = got
            else:
                assert Q.words(first).tobytes() == Q.words(got).tobytes()  # the same input, the same bytes
        occ, guard = _trace(rtw, w.dev, w.d_rays, n, opts, occluded=True)
        assert (guard == 0xA5).all(), (name, n)
        assert (occ == (w.ref["prim"][:n] > 0).astype(np.uint8)).all(), (name, asked, n)


@pytest.mark.parametrize("name", ["scene1", "scene7", "spheres_image"])
def test_lane_walk_gives_the_union_walks_bytes(rtw, worlds, name):
    w = worlds(name)
    a, _ = _trace(rtw, w.dev, w.d_rays, len(w.rays), rtw.query_opts("union"))
    b, _ = _trace(rtw, w.dev, w.d_rays, len(w.rays), rtw.query_opts("lane"))
    c, _ = _trace(rtw, w.dev, w.d_rays, len(w.rays), None)  # AUTO, opts NULL
    assert Q.words(a).tobytes() == Q.words(b).tobytes() == Q.words(c).tobytes()


def _axis_rays(rtw, W, desc):
    """Rays whose direction has two components exactly 0 (+0 and -0), aimed at spheres spread over the list
    from outside them along each axis: a batch of nothing else, so no lane's box tests can lean on a
    neighbour's (the union walk descends where ANY lane's box test passes)."""
    idx = [i for i in range(desc.n_prims) if desc.prims[i].kind == W.PRIM_SPHERE and 0 < desc.prims[i].a[6] < 50]
    idx = idx[::max(1, len(idx) // 24)]
    rows = []
    for j, i in enumerate(idx):
        # (off the centre by a little: a ray in the plane y = r of spheres resting on the ground lies in the
        # plane of a rect placed there, the reference's 0/0 case, which scene 6's own ray covers)
        c, r = np.array(desc.prims[i].a[0:3]) + np.array([0.0137, 0.0071, -0.0113]), desc.prims[i].a[6]
        z = -0.0 if j % 2 else 0.0
        for axis in range(3):
            o, d = c.copy(), np.array([z, z, z])
            o[axis] += r + 2.5
            d[axis] = -1.0 - 0.25 * (j % 3)
            rows.append((o, d, 0.5, 0.001, np.inf if j % 4 else 3.0))
    return Q.make_rays(rtw, rows)


@pytest.mark.parametrize("name,asked", [("scene1", "union"), ("scene1", "lane"), ("scene7", "lane"), ("small", "auto"),
                                        ("spheres_image", "union"), ("spheres_image", "lane")])
def test_axis_aligned_rays_through_the_bvh(rtw, W, worlds, name, asked):
    w = worlds(name)
    rays = _axis_rays(rtw, W, w.desc)
    ref = Q.oracle_hits(rtw, w.oracle, rays)
    assert len(rays) >= 36 and 0.5 <= (ref["prim"] > 0).mean() and np.isfinite(ref["t"]).all()
    assert ((rays["dir"] == 0.0).sum(axis=1) == 2).all()
    d_rays = torch.from_numpy(np.frombuffer(rays.tobytes(), np.uint8).copy()).cuda()
    opts = rtw.query_opts(asked)
    for n in (1, len(rays)):
        got, guard = _trace(rtw, w.dev, d_rays, n, opts)
        assert (guard == 0xA5).all()
        _assert_records(got, ref[:n], (name, asked, n))
        occ, _ = _trace(rtw, w.dev, d_rays, n, opts, occluded=True)
        assert (occ == (ref["prim"][:n] > 0)).all(), (name, asked, n)


@pytest.mark.parametrize("name", ["small", "small_swap"])
def test_coincident_pairs_later_index_wins(rtw, worlds, name):
    w = worlds(name)
    got, _ = _trace(rtw, w.dev, w.d_rays, len(w.rays), None)
    assert len(w.pairs) == 3
    for cls, later, rows in w.pairs:
        prims = [int(w.ref["prim"][w.n_main + r]) - 1 for r in rows]
        in_pair = [p for p in prims if p >= 0 and w.tables[0][p]["cls"] == cls]
        assert in_pair, (cls, prims)  # at least one ray's winner belongs to the pair ...
        assert all(p == later for p in in_pair), (cls, prims, later)  # ... and is its later list index
        assert [int(got["prim"][w.n_main + r]) - 1 for r in rows] == prims


def test_scene_api_equals_the_world_of_scene_1(rtw, worlds):
    w = worlds("scene1")
    sph, mats, _ = rtw.cover_scene(42)
    sc = rtw.DeviceScene(sph, mats)
    n = len(w.rays)
    a, ga = _trace(rtw, sc, w.d_rays, n, is_world=False)
    b, _ = _trace(rtw, w.dev, w.d_rays, n, None)
    assert (ga == 0xA5).all()
    assert Q.words(a).tobytes() == Q.words(b).tobytes()
    oa, ga = _trace(rtw, sc, w.d_rays, n, occluded=True, is_world=False)
    ob, _ = _trace(rtw, w.dev, w.d_rays, n, None, occluded=True)
    assert (ga == 0xA5).all() and (oa == ob).all() and (oa == (w.ref["prim"] > 0)).all()
    for m in (1, 65):
        c, g = _trace(rtw, sc, w.d_rays, m, is_world=False)
        assert (g == 0xA5).all() and Q.words(c).tobytes() == Q.words(a[:m]).tobytes()
    assert Q.words(sc.trace_host(w.rays[:70])).tobytes() == Q.words(a[:70]).tobytes()
    sc.close()


@pytest.mark.parametrize("name", ["scene6", "scene7"])
def test_torch_tracer_and_host_form(rtw, worlds, name):
    from rtw_amd.device import TorchTracer
    w = worlds(name)
    ok = ~np.isnan(w.ref["t"])
    rays, ref = w.rays[ok], w.ref[ok]
    tr = TorchTracer(w.dev)
    o, d = torch.from_numpy(rays["origin"].copy()).cuda(), torch.from_numpy(rays["dir"].copy()).cuda()
    time, t_max = torch.from_numpy(rays["time"].copy()).cuda(), torch.from_numpy(rays["t_max"].copy())
    h = tr.trace(o, d, time=time, t_min=0.001, t_max=t_max)
    torch.cuda.synchronize()
    assert h["prim"].dtype == torch.int64 and h["front"].dtype == torch.bool
    assert (h["prim"].cpu().numpy() == ref["prim"].astype(np.int64) - 1).all()
    assert (h["prim"].cpu().numpy()[ref["prim"] == 0] == -1).all()
    assert Q.words(h["records"].cpu().numpy().view(rtw.HIT_DTYPE).reshape(-1)).tobytes() == Q.words(ref).tobytes()
    for key, field in (("t", "t"), ("p", "p"), ("normal", "normal")):
        assert h[key].cpu().numpy().tobytes() == np.ascontiguousarray(ref[field]).tobytes(), key
    assert (h["uv"].cpu().numpy() == np.stack([ref["u"], ref["v"]], axis=1)).all()
    assert (h["front"].cpu().numpy() == (ref["front"] != 0)).all()
    occ = tr.occluded(o, d, time=time, t_max=t_max)
    assert occ.dtype == torch.bool and (occ.cpu().numpy() == (ref["prim"] > 0)).all()
    assert tr.trace(o[:0], d[:0])["prim"].numel() == 0
    # the host form (rtw_world_trace) on one batch
    assert Q.words(w.dev.trace_host(rays[:300])).tobytes() == Q.words(ref[:300]).tobytes()


def test_errors(rtw, worlds):
    w = worlds("scene5")
    L = rtw.lib()
    n = 64
    out = torch.full((n * 80 + 8,), 0xA5, dtype=torch.uint8, device="cuda")
    rp, op = w.d_rays.data_ptr(), out.data_ptr()

    def trace(world, rays, count, hits, opts=None):
        return L.rtw_world_trace_device(world, C.c_void_p(rays), count, opts, C.c_void_p(hits), None)

    def msg():
        return (L.rtw_last_error() or b"").decode()

    for args in ((None, rp, n, op), (w.dev.h, None, n, op), (w.dev.h, rp, n, None),      # null pointers
                 (w.dev.h, rp + 4, n, op), (w.dev.h, rp, n, op + 4),                        # misaligned
                 (w.dev.h, rp, (1 << 31) + 1, op)):                                        # n > 2^31
        assert trace(*args) == rtw.RTW_EINVAL and "rtw_world_trace_device" in msg(), args
    assert trace(w.dev.h, rp, n, op, C.byref(rtw.QueryOpts(3, 0))) == rtw.RTW_EINVAL
    assert L.rtw_world_occluded_device(w.dev.h, None, n, None, C.c_void_p(op), None) == rtw.RTW_EINVAL
    assert L.rtw_world_trace(w.dev.h, None, n, None, C.c_void_p(op)) == rtw.RTW_EINVAL
    sph, mats, _ = rtw.cover_scene(42)
    sc = rtw.DeviceScene(sph, mats)
    assert L.rtw_scene_trace_device(sc.h, C.c_void_p(rp + 4), n, C.c_void_p(op), None) == rtw.RTW_EINVAL
    assert "rtw_scene_trace_device" in msg()
    assert L.rtw_scene_occluded_device(sc.h, C.c_void_p(rp), n, None, None) == rtw.RTW_EINVAL
    # n == 0: RTW_OK, nothing launched, the output untouched
    assert trace(w.dev.h, rp, 0, op) == rtw.RTW_OK
    assert L.rtw_world_occluded_device(w.dev.h, C.c_void_p(rp), 0, None, C.c_void_p(op), None) == rtw.RTW_OK
    assert L.rtw_scene_trace_device(sc.h, C.c_void_p(rp), 0, C.c_void_p(op), None) == rtw.RTW_OK
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0xA5).all()
    sc.close()
