"""Dynamic worlds on the GPU (rtw_hip.h "dynamic worlds"):
rtw_world_update / rtw_world_update_device give an uploaded world new numbers
in place and refit its BVH (csrc/rtw_world_update.hip).

  * the device tables after an update are, byte for byte, what the host refit
    (rtw_world_refit_tables_host) computes — through the host-array and the
    device-array entry, after an identity and after a displacement update;
  * every render, guide buffer, query and accumulator pass of an updated world
    equals that of a world freshly created from the updated description, and
    the oracle's linear list (bar: test_gpu_parity.assert_parity);
  * A -> B -> A gives the original world's bytes and its node visits and
    primitive tests: the boxes are no looser;
  * the leaf pretest's bits follow a radius across 100 and a centre across 2^20;
  * refusals (RTW_EINVAL) leave the world as it was;
  * worlds without a BVH update their records.

Inputs: helpers.mixed_bvh_world moved by update_helpers.displace (every sphere
by 3-10 radii, every transform re-angled and re-offset, two moving spheres with
a new centre1); tests/test_refit_host.py shows on the oracle alone that these
stay in the input domain and keep every class visible.  Frames: 64x36 at 20 and
40 spp (one and two chunks), max_depth 50, seeds of test_gpu_parity.SEEDS."""
import ctypes as C

import numpy as np
import pytest

from helpers import MIXED_CAMERA, MIXED_SIZES, _to_desc, diff_stats, mixed_bvh_world, to_oracle_camera
from test_gpu_parity import SEEDS, assert_parity
from update_helpers import blob_nodes, cull_bits, displace, numbers, prims_with, truncated, xforms_with

pytestmark = pytest.mark.gpu

SKY = (0.7, 0.8, 1.0)
GEN_SEED = 5
FW, FH = 64, 36
WORLDS = {"small": (*MIXED_SIZES["small"], None), "large": (*MIXED_SIZES["large"], None),
          "spheres_image": (0, 520, "spheres_image")}
RTW_EINVAL = -1


@pytest.fixture(scope="module")
def W():
    from rtw_amd import world
    return world


@pytest.fixture(scope="module")
def earth(W):
    return W.earth_map()


class Case:
    """A world and its update: tables / descriptor / numbers before (0) and after (1)."""

    def __init__(self, W, oracle, earth, name):
        self.name = name
        if name == "globe300":
            self.built = W.BuiltScene(7, 42, image=earth)
            self.desc0 = truncated(W, self.built.desc, 300)
            self.a0, self.xv0 = W.desc_numbers(self.desc0)
            rng = np.random.default_rng(7)
            self.a1, self.xv1 = self.a0.copy(), self.xv0.copy()
            small = np.abs(self.a0[:, 6]) < 100
            th = rng.uniform(0, 2 * np.pi, len(self.a0))
            d = rng.uniform(3, 10, len(self.a0)) * np.abs(self.a0[:, 6])
            for c, f in ((0, np.cos(th)), (2, np.sin(th))):
                self.a1[small, c] += (d * f)[small]
                self.a1[small, 3 + c] += (d * f)[small]
            self.tables1 = None
        else:
            nb, ns, variant = WORLDS[name]
            self.tables0 = mixed_bvh_world(W, earth, nb, ns, GEN_SEED, variant=variant)
            self.tables1 = displace(self.tables0)
            self.desc0, self._k0 = _to_desc(W, *self.tables0)
            self.a0, self.xv0 = numbers(self.tables0)
            self.a1, self.xv1 = numbers(self.tables1)
        self._oracle, self._o = oracle, {}

    def desc(self, W, a, xv):
        """The descriptor with other numbers (fresh arrays; keep the result alive while it is used)."""
        d = truncated(W, self.desc0, self.desc0.n_prims)
        keep = (prims_with(W, self.desc0, a), xforms_with(W, self.desc0, xv))
        d.prims, d.xforms = C.cast(keep[0], C.POINTER(W.Prim)), C.cast(keep[1], C.POINTER(W.Xform))
        return d, keep

    def oracle1(self):
        if 1 not in self._o:
            self._o[1] = self._oracle.TableWorld(*self.tables1, background=SKY)
        return self._o[1]


@pytest.fixture(scope="module")
def cases(W, oracle, earth):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Case(W, oracle, earth, name)
        return cache[name]
    return get


@pytest.fixture(scope="module")
def cam(rtw, oracle):
    m = MIXED_CAMERA
    c = rtw.camera_init(m["look_from"], m["look_at"], (0, 1, 0), m["vfov"], 16 / 9, m["aperture"], m["focus"], 0.0, 1.0)
    return c, to_oracle_camera(oracle, c)


def render(rtw, dw, cam, p, counts=True):
    import torch
    need = dw.workspace_bytes(p)
    ws = torch.empty(need + 256, dtype=torch.uint8, device="cuda:0")
    ptr = (ws.data_ptr() + 255) & ~255
    rgb = torch.empty((p.row_count, p.width, 3), dtype=torch.uint8, device="cuda:0")
    mean = torch.empty((p.row_count, p.width, 3), dtype=torch.float32, device="cuda:0")
    dw.render_async(cam, p, ptr, need, rgb.data_ptr(), mean.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    c = dw.counts(cam, p, ptr, need) if counts else None
    return rgb.cpu().numpy(), mean.cpu().numpy(), c


def assert_same(a, b, what, visits=False):
    (ra, ma, ca), (rb, mb, cb) = a, b
    assert (ra == rb).all(), (what, diff_stats(ra, rb))
    assert np.array_equal(ma.view(np.uint32), mb.view(np.uint32)), what
    if ca is not None and cb is not None:
        assert ca["samples"] == cb["samples"] and ca["segments"] == cb["segments"], (what, ca, cb)
        if visits:
            assert ca["node_visits"] == cb["node_visits"] and ca["prim_tests"] == cb["prim_tests"], (what, ca, cb)


def apply(W, case, dw, entry, a, xv):
    """One update through the host-array or the device-array entry."""
    if entry == "host":
        d, keep = case.desc(W, a, xv)
        dw.update(d)
    else:
        import torch

        from rtw_amd.device import update_world
        update_world(dw, torch.from_numpy(np.ascontiguousarray(a)).cuda(),
                     torch.from_numpy(np.ascontiguousarray(xv)).cuda() if len(xv) else None)


def same_tables(got, want, what, bounds_bits=True):
    assert got["blob"].size == want["blob"].size, what
    diff = np.nonzero(got["blob"] != want["blob"])[0]
    assert diff.size == 0, (what, diff.size, diff[:8])
    assert np.array_equal(got["cull"].view(np.uint32), want["cull"].view(np.uint32)), (what, got["cull"], want["cull"])
    if bounds_bits:
        assert np.array_equal(got["bounds"].view(np.uint64), want["bounds"].view(np.uint64)), (what, got["bounds"], want["bounds"])
    else:
        assert np.array_equal(got["bounds"], want["bounds"]), (what, got["bounds"], want["bounds"])


# ------------------------------------------------------------------ 1. bytes ----
@pytest.mark.parametrize("entry", ["host", "device"])
@pytest.mark.parametrize("name", ["small", "large", "globe300"])
def test_tables_equal_the_host_refit(rtw, W, cases, name, entry):
    c = cases(name)
    flags = W.WORLD_DYNAMIC
    dw = W.DeviceWorld(c.desc0, dynamic=True)
    try:
        n = dw.table_bytes()
        info = dw.bvh_info()
        assert info["nodes"] > (256 if name == "large" else 0), info
        created = W.refit_tables_host(c.desc0, flags, n)
        same_tables(dw.read_tables(), created, "as created")
        apply(W, c, dw, entry, c.a0, c.xv0)
        got = dw.read_tables()
        same_tables(got, W.refit_tables_host(c.desc0, flags, n, c.a0, c.xv0 if len(c.xv0) else None), "identity")
        same_tables(got, created, "identity against the created tables", bounds_bits=False)
        apply(W, c, dw, entry, c.a1, c.xv1)
        got = dw.read_tables()
        assert (got["blob"] != created["blob"]).sum() > 1000
        same_tables(got, W.refit_tables_host(c.desc0, flags, n, c.a1, c.xv1 if len(c.xv1) else None), "displaced")
        assert dw.bvh_info() == info
    finally:
        dw.close()


def test_frozen_worlds_are_unchanged(rtw, W, cases):
    """Without the flag: the same table bytes as with it, and no update."""
    c = cases("small")
    frozen, dyn = W.DeviceWorld(c.desc0), W.DeviceWorld(c.desc0, dynamic=True)
    try:
        same_tables(frozen.read_tables(), dyn.read_tables(), "frozen against dynamic")
        with pytest.raises(rtw.RtwError) as e:
            apply(W, c, frozen, "device", c.a1, c.xv1)
        assert e.value.status == RTW_EINVAL
    finally:
        frozen.close(), dyn.close()


# ----------------------------------------------------- 2. images, fresh world ----
@pytest.mark.parametrize("name,trav", [("small", "linear"), ("small", "union"), ("large", "union"),
                                       ("spheres_image", "union"), ("spheres_image", "lane")])
def test_updated_world_renders_as_a_fresh_one_and_the_oracle(rtw, W, cases, cam, name, trav):
    c = cases(name)
    linear = trav == "linear"
    dyn = W.DeviceWorld(c.desc0, linear=linear, dynamic=True)
    d1, keep = c.desc(W, c.a1, c.xv1)
    fresh = W.DeviceWorld(d1, linear=linear)
    try:
        apply(W, c, dyn, "device", c.a1, c.xv1)
        for spp, seed in ((20, SEEDS[1]), (40, SEEDS[2])):
            p = rtw.make_params(FW, FH, spp, 50, seed, background=SKY, world_traversal="auto" if linear else trav)
            assert dyn.launch_info(p)["traversal"] == trav
            got, want = render(rtw, dyn, cam[0], p), render(rtw, fresh, cam[0], p)
            assert_same(got, want, (name, trav, spp))
            assert got[0].std() > 5
            ref = c.oracle1().render_tier_b(cam[1], FW, FH, spp, seed=seed, bg=SKY, threads=16)[0]
            assert_parity(got[0], ref, f"updated {name} {trav} {FW}x{FH}x{spp}")
    finally:
        dyn.close(), fresh.close()


# ------------------------------------------------------------ 3. A -> B -> A ----
@pytest.mark.parametrize("name,trav,entries", [("large", "union", ("device", "host")), ("spheres_image", "lane", ("host", "device"))])
def test_there_and_back_gives_the_original_world(rtw, W, cases, cam, name, trav, entries):
    c = cases(name)
    orig, dyn = W.DeviceWorld(c.desc0), W.DeviceWorld(c.desc0, dynamic=True)
    try:
        p = rtw.make_params(FW, FH, 20, 50, SEEDS[3], background=SKY, world_traversal=trav)
        want = render(rtw, orig, cam[0], p)
        apply(W, c, dyn, entries[0], c.a1, c.xv1)
        moved = render(rtw, dyn, cam[0], p)
        assert (moved[0] != want[0]).any(axis=2).mean() > 0.2  # (the update did change the frame)
        apply(W, c, dyn, entries[1], c.a0, c.xv0)
        assert_same(render(rtw, dyn, cam[0], p), want, (name, "A -> B -> A"), visits=True)
    finally:
        orig.close(), dyn.close()


# ------------------------------------------- 4. queries, guides, accumulator ----
@pytest.mark.parametrize("name", ["small", "large"])
def test_queries_guides_and_passes_of_an_updated_world(rtw, oracle, W, cases, cam, name):
    from query_helpers import _assert_records, check_conditions, oracle_hits, ray_set
    from test_gpu_accum import same_image
    from test_gpu_accum_world import accumulate
    from test_gpu_guides import device_guides
    c = cases(name)
    dyn = W.DeviceWorld(c.desc0, dynamic=True)
    d1, keep = c.desc(W, c.a1, c.xv1)
    fresh = W.DeviceWorld(d1)
    try:
        apply(W, c, dyn, "device", c.a1, c.xv1)
        rays, kinds = ray_set(rtw, c.oracle1(), cam[0], MIXED_CAMERA["look_from"], 77)
        ref = oracle_hits(rtw, c.oracle1(), rays)
        check_conditions(rays, kinds, ref)
        _assert_records(dyn.trace_host(rays), ref, (name, "updated world's queries"))
        p1 = rtw.make_params(FW, FH, 1, background=SKY)
        g, gf = device_guides(rtw, dyn, cam[0], p1), device_guides(rtw, fresh, cam[0], p1)
        assert g.tobytes() == gf.tobytes() and len(np.unique(g["prim"])) > 10
        p = rtw.make_params(FW, FH, 40, 50, SEEDS[0], background=SKY)
        one_shot = render(rtw, dyn, cam[0], p, counts=False)
        assert same_image(accumulate(rtw, dyn, cam[0], p, [20, 20]), one_shot)
        assert_same(one_shot, render(rtw, fresh, cam[0], p, counts=False), (name, "one shot"))
    finally:
        dyn.close(), fresh.close()


# ------------------------------------------------------------ 5. pretest edges ----
def test_pretest_bits_follow_the_radius_and_the_centre(rtw, W, cases, cam):
    """In the large world (leaves of one) a small static sphere is a leaf with a pretest record.
    It is placed behind the scene at (0, 60, -300), 323 from the camera: radius 99 keeps the bit,
    101 loses exactly that one, 99 gets it back; its centre beyond 2^20 clears every bit, and
    back restores them.  The image equals the fresh world's every time."""
    c = cases("large")
    li = next(i for i, p in enumerate(c.tables0[0]) if p["kind"] == 0 and p["xform"] < 0 and p["cls"] == "base" and abs(p["a"][6]) < 1)
    dyn = W.DeviceWorld(c.desc0, dynamic=True)
    p = rtw.make_params(FW, FH, 20, 50, SEEDS[1], background=SKY)
    try:
        n_nodes = dyn.bvh_info()["nodes"]

        def step(centre, r):
            a = c.a0.copy()
            a[li, 0:3], a[li, 3:6], a[li, 6] = centre, centre, r
            apply(W, c, dyn, "device", a, c.xv0)
            d, keep = c.desc(W, a, c.xv0)
            fresh = W.DeviceWorld(d)
            try:
                assert_same(render(rtw, dyn, cam[0], p), render(rtw, fresh, cam[0], p), ("pretest edge", centre, r))
            finally:
                fresh.close()
            t = dyn.read_tables()
            return cull_bits(blob_nodes(c.desc0, n_nodes, t["blob"])), t["cull"]
        bits0 = cull_bits(blob_nodes(c.desc0, n_nodes, dyn.read_tables()["blob"]))
        assert bits0 > 100
        spot = (0.0, 60.0, -300.0)
        b99, _ = step(spot, 99.0)
        b101, _ = step(spot, 101.0)
        b99b, _ = step(spot, 99.0)
        assert (b99, b101, b99b) == (bits0, bits0 - 1, bits0)
        far, cull = step((2.0 ** 20 + 4096.0, 60.0, -300.0), 0.4)
        assert far == 0 and cull[0] > 2.0 ** 20
        back, cull = step(spot, 99.0)
        assert back == bits0 and cull[0] <= 2.0 ** 20
    finally:
        dyn.close()


# ---------------------------------------------------------------- 6. refusals ----
def test_refusals_leave_the_world_untouched(rtw, W, cases, cam):
    c = cases("small")
    dyn = W.DeviceWorld(c.desc0, dynamic=True)
    p = rtw.make_params(FW, FH, 20, 50, SEEDS[2], background=SKY)
    prims = c.tables0[0]
    sphere = next(i for i, q in enumerate(prims) if q["kind"] == 0)
    moving = next(i for i, q in enumerate(prims) if q["kind"] == 1)
    rect = next(i for i, q in enumerate(prims) if q["kind"] >= 2)
    try:
        before = render(rtw, dyn, cam[0], p)
        tables = dyn.read_tables()

        def refused(f, what):
            with pytest.raises(rtw.RtwError) as e:
                f()
            assert e.value.status == RTW_EINVAL, what
            same_tables(dyn.read_tables(), tables, what)
            assert_same(render(rtw, dyn, cam[0], p), before, what)

        def with_number(i, k, v, entry):
            a = c.a1.copy()
            a[i, k] = v
            return lambda: apply(W, c, dyn, entry, a, c.xv1)
        # wrong counts
        d, keep = c.desc(W, c.a1, c.xv1)
        d.n_prims -= 1
        refused(lambda: dyn.update(d), "one primitive fewer")
        d.n_prims += 1
        d.n_xforms -= 1
        refused(lambda: dyn.update(d), "one transform fewer")
        # a changed kind, material, transform index or op
        for field, i, v in (("kind", sphere, 1), ("mat", rect, (prims[rect]["mat"] + 1) % 3), ("xform", sphere, 0)):
            d, keep = c.desc(W, c.a1, c.xv1)
            setattr(keep[0][i], field, v)
            refused(lambda: dyn.update(d), "changed " + field)
        d, keep = c.desc(W, c.a1, c.xv1)
        keep[1][0].op[0] ^= 1
        refused(lambda: dyn.update(d), "changed op")
        # NaN / Inf in a used field, through both entries
        for entry in ("host", "device"):
            refused(with_number(sphere, 1, np.nan, entry), "NaN centre")
            refused(with_number(sphere, 6, np.inf, entry), "Inf radius")
            refused(with_number(rect, 4, -np.inf, entry), "Inf rect plane")
            refused(with_number(moving, 5, np.nan, entry), "NaN centre1")
            refused(with_number(moving, 8, c.a1[moving, 7], entry), "time1 == time0")
            refused(with_number(moving, 8, c.a1[moving, 7] - 1.0, entry), "time1 < time0")
            xv = c.xv1.copy()
            xv[0, 0, 0] = np.nan
            refused(lambda: apply(W, c, dyn, entry, c.a1, xv), "NaN transform value")
        # ... but not in a field the kind does not use
        a = c.a0.copy()
        a[sphere, 7], a[rect, 8] = np.nan, np.inf
        apply(W, c, dyn, "device", a, c.xv0)
        assert_same(render(rtw, dyn, cam[0], p), before, "unused fields")
    finally:
        dyn.close()


# ------------------------------------------------------------ 7. no-BVH worlds ----
def test_worlds_without_a_bvh_update_their_records(rtw, oracle, W):
    """Scene 6 (the Cornell box: 20 primitives, the linear loop): the inner boxes' RotateY angles
    change.  Equal to a fresh world and to the oracle."""
    b = W.BuiltScene(6, 42)
    a0, xv0 = W.desc_numbers(b.desc)
    xv1 = xv0.copy()
    rot = 0
    for i in range(b.desc.n_xforms):
        for k in range(b.desc.xforms[i].n):
            if b.desc.xforms[i].op[k] == W.XF_ROTATE_Y:
                t = xv0[i, k, 2] + (0.35 if rot % 2 else -0.3)
                xv1[i, k] = (np.sin(t), np.cos(t), t)
                rot += 1
    assert rot >= 2
    cam = b.camera()
    p = rtw.make_params(40, 40, 20, 50, SEEDS[1], background=b.background)
    keep = (prims_with(W, b.desc, a0), xforms_with(W, b.desc, xv1))
    d1 = truncated(W, b.desc, b.desc.n_prims)
    d1.prims, d1.xforms = C.cast(keep[0], C.POINTER(W.Prim)), C.cast(keep[1], C.POINTER(W.Xform))
    dyn, fresh, frozen = W.DeviceWorld(b.desc, dynamic=True), W.DeviceWorld(d1), W.DeviceWorld(b.desc)
    try:
        assert dyn.bvh_info()["nodes"] == 0
        before = render(rtw, frozen, cam, p)
        dyn.update(d1)
        got = render(rtw, dyn, cam, p)
        assert_same(got, render(rtw, fresh, cam, p), "Cornell box, rotated boxes")
        assert (got[0] != before[0]).any(axis=2).mean() > 0.05
        same_tables(dyn.read_tables(), W.refit_tables_host(b.desc, W.WORLD_DYNAMIC, dyn.table_bytes(), a0, xv1), "Cornell box")
        t = b.table()
        for i, x in enumerate(t["xforms"]):
            x["v"] = [list(xv1[i, k]) for k in range(x["n"])]
        o = oracle.TableWorld(t["prims"], t["xforms"], t["textures"], t["materials"], t["perlins"], [], background=b.background)
        ref = o.render_tier_b(to_oracle_camera(oracle, cam), 40, 40, 20, seed=SEEDS[1], bg=b.background, threads=16)[0]
        assert_parity(got[0], ref, "updated Cornell box 40x40x20")
    finally:
        dyn.close(), fresh.close(), frozen.close()


def test_linear_flag_world_updates_its_records(rtw, W, cases, cam):
    """A DYNAMIC world created with RTW_WORLD_LINEAR: device entry, against the fresh linear world and
    the fresh BVH world."""
    c = cases("small")
    dyn = W.DeviceWorld(c.desc0, linear=True, dynamic=True)
    d1, keep = c.desc(W, c.a1, c.xv1)
    fresh_lin, fresh_bvh = W.DeviceWorld(d1, linear=True), W.DeviceWorld(d1)
    try:
        assert dyn.bvh_info()["nodes"] == 0
        apply(W, c, dyn, "host", c.a1, c.xv1)
        p = rtw.make_params(FW, FH, 20, 50, SEEDS[3], background=SKY)
        got = render(rtw, dyn, cam[0], p)
        assert_same(got, render(rtw, fresh_lin, cam[0], p), "linear world")
        assert_same(got, render(rtw, fresh_bvh, cam[0], p), "linear world against the BVH")
        same_tables(dyn.read_tables(), fresh_lin.read_tables(), "linear world's tables are the fresh world's", bounds_bits=False)
    finally:
        dyn.close(), fresh_lin.close(), fresh_bvh.close()


# ------------------------------------------------------------------------ CLI ----
def test_cli_frames_and_orbit(rtw, tmp_path):
    """bin/rtw_render --frames N --orbit DEG: one upload, an update per frame.  --frames 1 is the
    plain run; with --orbit 0 every frame goes through an update with the creation's numbers and
    has the plain run's bytes; with --orbit 20 the Cornell box's boxes turn, so the frames differ,
    and the last one is --out."""
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(rtw.__file__), "..", "bin", "rtw_render")
    base = [exe, "--scene", "6", "--width", "40", "--spp", "20"]
    dirs = {n: tmp_path / n for n in ("plain", "one", "still", "turn")}
    for d in dirs.values():
        d.mkdir()
    runs = {"plain": [], "one": ["--frames", "1", "--orbit", "20"], "still": ["--frames", "3", "--orbit", "0"],
            "turn": ["--frames", "3", "--orbit", "20"]}
    for n, extra in runs.items():
        r = subprocess.run(base + ["--out", str(dirs[n] / "out.ppm")] + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
    plain = (dirs["plain"] / "out.ppm").read_bytes()
    assert (dirs["one"] / "out.ppm").read_bytes() == plain and os.listdir(dirs["one"]) == ["out.ppm"]
    frames = ["frame_0000.ppm", "frame_0001.ppm", "frame_0002.ppm"]
    for n in ("still", "turn"):
        assert sorted(os.listdir(dirs[n])) == frames + ["out.ppm"]
        assert (dirs[n] / "frame_0000.ppm").read_bytes() == plain
        assert (dirs[n] / "frame_0002.ppm").read_bytes() == (dirs[n] / "out.ppm").read_bytes()
    assert all((dirs["still"] / f).read_bytes() == plain for f in frames)
    turned = [(dirs["turn"] / f).read_bytes() for f in frames]
    assert len(set(turned)) == 3
    r = subprocess.run(base + ["--frames", "2", "--pass-spp", "10"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--frames" in r.stderr
