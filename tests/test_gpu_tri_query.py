"""Ray, surface and guide queries over worlds that hold triangles.

The expected record of a ray is the merge of rtw_world_trace_tri_host (the triangles: the reference's sequential loop
through csrc/rtw_tri.hpp, on the CPU) and the oracle's rw_hit over the other primitives: the smaller t, the later
list index on a tie; compared with the device's byte for byte (t, p, normal, u, v, front, prim).  Worlds: the
general-triangle world of T4(a) with one axis-aligned card and two image-textured meshes, the small mixed world with
its rects as triangles (T2), and T3's cards among >= 512 untransformed spheres, whose queries walk per lane
(world_query_lane_kernel's triangle sets, closest and ANY).  Ray sets: query_helpers.ray_set (48x27 feature rays, bounce, inward, shadow) at two seeds of times, rays
aimed exactly at vertices and edge points, rays in a triangle's plane, rays that start on a triangle (t_min = 0),
the interval variants V1-V5, directions scaled by 2^+-100, and axis rays with zero components (the ZDIR box path).
The entries the issue leaves out return RTW_UNSUPPORTED before any launch."""
import types

import numpy as np
import pytest

from helpers import MIXED_CAMERA, MIXED_SIZES, _to_desc, mixed_bvh_world
import query_helpers as Q
import tri_helpers as T

pytestmark = pytest.mark.gpu

SKY = (0.7, 0.8, 1.0)


@pytest.fixture(scope="module")
def W():
    from rtw_amd import world
    return world


class Merged:
    """One world on three sides: the device's (BVH and linear), the host triangle entry, the oracle's rest."""

    def __init__(self, rtw, oracle, W, tables, camera):
        self.rtw, self.W, self.tables = rtw, W, tables
        self.desc, self._keep = _to_desc(W, *tables)
        rest, self.index = T.split_triangles(W, tables)
        self.ow = oracle.TableWorld(*rest, background=SKY)
        c = camera
        self.look_from = c["look_from"]
        self.cam = rtw.camera_init(c["look_from"], c["look_at"], (0, 1, 0), c["vfov"], 16 / 9, 0.0, c["focus"], 0.0, 1.0)
        self.sets = {}

    def expected(self, rays):
        tri = self.W.trace_tri_host(self.desc, rays)
        return T.merge_hits(tri, Q.oracle_hits(self.rtw, self.ow, rays), self.index)

    def hit(self, o, d, time=0.0, t_min=0.001, t_max=float("inf")):  # OracleWorld.hit's shape, for query_helpers.ray_set
        r = Q.make_rays(self.rtw, [(o, d, time, t_min, t_max)])
        h = self.expected(r)[0]
        if h["prim"] == 0:
            return None
        return {"prim": int(h["prim"]) - 1, "t": float(h["t"]), "p": list(h["p"]), "normal": list(h["normal"]),
                "uv": [float(h["u"]), float(h["v"])], "front": bool(h["front"])}

    def base(self, seed):
        if seed not in self.sets:
            rays, kinds = Q.ray_set(self.rtw, self, self.cam, self.look_from, seed, w=48, h=27)
            self.sets[seed] = (rays, kinds, self.expected(rays))
        return self.sets[seed]

    def tri_rows(self):
        return [i for i, p in enumerate(self.tables[0]) if p["kind"] == self.W.PRIM_TRIANGLE and p["xform"] < 0]


@pytest.fixture(scope="module")
def worlds(rtw, oracle, W):
    earth = W.earth_map()
    general = list(T.general_world(W, 1, earth=earth))
    y = 2.5  # one axis-aligned card: rays in its plane have n . d == 0 exactly
    general[0] = general[0] + T.rect_tris(W, dict(kind=W.PRIM_XZ_RECT, mat=2, xform=-1, a=[-2.0, 2.0, -1.0, 3.0, y]))
    orig = mixed_bvh_world(W, earth, *MIXED_SIZES["small"], 5)
    mixed, _ = T.triangulate(W, orig, keep=T.reads_uv(W, orig))
    cards, _ = T.triangulate(W, T.cards_world(W, earth))
    return {"general": Merged(rtw, oracle, W, tuple(general), dict(T.T4_CAMERA)),
            "mixed": Merged(rtw, oracle, W, mixed, dict(MIXED_CAMERA)),
            "cards": Merged(rtw, oracle, W, cards, dict(MIXED_CAMERA))}


def special_rays(m):
    """Vertices, edge points, in-plane rays and rays that start on a triangle, over the untransformed triangles."""
    rng = np.random.default_rng(77)
    prims, rows = m.tables[0], []
    o0 = np.array(m.look_from, float)
    for i in m.tri_rows()[::3]:
        v = np.array(prims[i]["a"], float).reshape(3, 3)
        for k in range(3):
            rows.append((o0, v[k] - o0, 0.5, 0.001, np.inf))                                   # a vertex, exactly
            e = v[k] + rng.choice([0.5, 0.25, 0.8]) * (v[(k + 1) % 3] - v[k])
            rows.append((o0, (e - o0) * rng.choice([1.0, 0.5, 3.0]), 0.5, 0.001, np.inf))      # an edge point
        c = v.mean(axis=0)
        n = np.cross(v[1] - v[0], v[2] - v[0])
        rows.append((c, n + 0.3 * rng.normal(size=3), 0.5, 0.0, np.inf))                       # starts on it: t_min = 0
        rows.append((c, -n, 0.5, 0.0, 2.0))
    # (in a GENERAL triangle's plane n . d is rounding noise, not 0, and the root any number: as for rects, such a
    # ray is guaranteed the list's record only without a BVH — DESIGN.md §22 — so the set holds exact planes only)
    for x in np.linspace(-3, 3, 9):                                                            # in the plane y = 2.5 (the general world's card)
        rows.append(((x, 2.5, -4.0), (0.1 * x, 0.0, 1.0), 0.5, 0.001, np.inf))
        rows.append(((-5.0, 2.5, x), (1.0, 0.0, 0.0), 0.5, 0.001, np.inf))
    n_plane = 0
    for i in m.tri_rows():                                                                     # in the plane of every axis-aligned triangle
        v = np.array(prims[i]["a"], float).reshape(3, 3)
        if not (v == v[0]).all(axis=0).any():
            continue
        e, c = v[1] - v[0], v.mean(axis=0)
        c[(v == v[0]).all(axis=0)] = v[0][(v == v[0]).all(axis=0)]                             # (exactly in the plane: n . d == 0)
        rows.append((c - 2.0 * e, e, 0.5, 0.001, np.inf))
        n_plane += 1
    assert n_plane >= 2
    return Q.make_rays(m.rtw, rows)


def edge_sets(m):
    """(name, rays) beyond the base sets; the helpers of query_helpers on this world's verified set."""
    rays, kinds, ref = m.base(100)
    w = types.SimpleNamespace(rays=rays, ref=ref, kinds=kinds, _rtw=m.rtw)
    out = [("special", special_rays(m))]
    out += [(v, Q._interval(w, v)) for v in ("V1", "V2", "V3", "V4", "V5")]
    out += [("plain", Q._plain_interval(w)), ("scaled", Q._scaled(w)), ("axis", Q._axis(w))]
    return out


def run_all(m, dev, rays, ref, where, opts_list):
    d_rays = Q.to_device(rays)
    for opts in opts_list:
        got, guard = Q._trace(m.rtw, dev, d_rays, len(rays), opts)
        assert (guard == 0xA5).all(), where
        Q._assert_records(got, ref, (where, opts and opts.traversal))
        occ, guard = Q._trace(m.rtw, dev, d_rays, len(rays), opts, occluded=True)
        assert (guard == 0xA5).all() and np.array_equal(occ != 0, ref["prim"] > 0), (where, "occluded")


@pytest.mark.parametrize("name", ["general", "mixed", "cards"])
def test_records_equal_the_merged_reference(rtw, W, worlds, name):
    m = worlds[name]
    bvh, lin = W.DeviceWorld(m.desc), W.DeviceWorld(m.desc, linear=True)
    try:
        assert bvh.bvh_info()["nodes"] > 0 and bvh.query_info()["feature_set"] & 64
        opts = [None, rtw.QueryOpts(rtw.WORLD_TRAVERSAL["union"], 0), rtw.QueryOpts(rtw.WORLD_TRAVERSAL["lane"], 0)]
        if name == "cards":  # untransformed spheres and triangles, >= RTW_QUERY_LANE_NODES nodes: per lane, forced and by AUTO
            assert bvh.bvh_info()["nodes"] >= 256
            for o in (opts[2], None):
                qi = bvh.query_info(o)
                assert qi["traversal"] == "lane" and qi["feature_set"] & 16 and qi["feature_set"] & 64, qi
            assert bvh.query_info(opts[1])["traversal"] == "union"
            opts = [opts[2], opts[1]]  # (edge sets below: lane first)
        n_tri = 0
        for seed in (100, 101):
            rays, kinds, ref = m.base(seed)
            hit = ref["prim"] > 0
            is_tri = np.isin(ref["prim"][hit] - 1, [i for i, p in enumerate(m.tables[0]) if p["kind"] == W.PRIM_TRIANGLE])
            n_tri += int(is_tri.sum())
            assert 0.1 <= hit.mean() <= 0.95 and is_tri.any() and (~is_tri).any() and ((ref["front"] == 0) & hit).any()
            run_all(m, bvh, rays, ref, (name, seed, "bvh"), opts)
            run_all(m, lin, rays, ref, (name, seed, "linear"), [None])
        for label, rays in edge_sets(m):
            ref = m.expected(rays)
            if label == "special":
                assert (ref["prim"] > 0).mean() > 0.5
            run_all(m, bvh, rays, ref, (name, label, "bvh"), opts[:2])
            run_all(m, lin, rays, ref, (name, label, "linear"), [None])
        print(name, "rays whose record is a triangle:", n_tri)
    finally:
        bvh.close()
        lin.close()


@pytest.mark.parametrize("name", ["general", "mixed"])
def test_surface_and_guides_follow_the_records(rtw, W, worlds, name):
    """rtw_world_surface_device over the merged reference's records: the guides it writes must equal
    rtw_world_guides_device's buffer, whose rays are the camera's feature rays (so the guide kernel's records are the
    merged reference's too), and the material kinds are the tables'."""
    import torch
    m = worlds[name]
    w, h = 48, 27
    dw = W.DeviceWorld(m.desc)
    try:
        p = rtw.make_params(w, h, 1, background=SKY)
        g1 = torch.zeros(w * h * 32, dtype=torch.uint8, device="cuda")
        dw.guides(m.cam, p, g1.data_ptr(), torch.cuda.current_stream().cuda_stream)
        rays, kinds, ref = m.base(100)
        prim = rays[kinds == "a"].copy()
        prim["time"] = 0.5 * (m.cam.time0 + m.cam.time1)
        want = m.expected(prim)
        d_rays = Q.to_device(prim)
        hits, _ = Q._trace(rtw, dw, d_rays, len(prim))
        Q._assert_records(hits, want, "feature rays")
        d_hits = Q.to_device(hits)
        g2 = torch.zeros(w * h * 32, dtype=torch.uint8, device="cuda")
        surf = torch.zeros(w * h * 64, dtype=torch.uint8, device="cuda")
        dw.surface(d_hits.data_ptr(), len(prim), surf.data_ptr(), g2.data_ptr(), SKY, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        a, b = g1.cpu().numpy().view(rtw.GUIDE_DTYPE), g2.cpu().numpy().view(rtw.GUIDE_DTYPE)
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
        tri = np.isin(a["prim"].astype(np.int64) - 1, [i for i, q in enumerate(m.tables[0]) if q["kind"] == W.PRIM_TRIANGLE])
        assert tri.sum() > 30 and (a["prim"] > 0).mean() > 0.5
        s = surf.cpu().numpy().view(rtw.SURFACE_DTYPE)
        mats = m.tables[3]
        hit = want["prim"] > 0
        kinds_want = np.array([mats[m.tables[0][i - 1]["mat"]]["kind"] + 1 if i else 0 for i in want["prim"]])
        assert np.array_equal(s["kind"], kinds_want) and hit.any()
    finally:
        dw.close()


def test_unbuilt_entries_refuse_a_triangle_world(rtw, W, worlds):
    """rtw_world_prev_points_device and rtw_world_mirror_points_device: RTW_UNSUPPORTED, the outputs untouched."""
    import torch
    m = worlds["general"]
    dw = W.DeviceWorld(m.desc)
    try:
        rays, kinds, ref = m.base(100)
        n = 64
        d_hits, d_rays = Q.to_device(ref[:n]), Q.to_device(rays[:n])
        out = torch.full((n * 24 + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        out2 = torch.full((n * 80 + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        with pytest.raises(rtw.RtwError) as e:
            dw.prev_points_device(d_hits.data_ptr(), n, 0.5, out.data_ptr())
        assert e.value.status == rtw.RTW_UNSUPPORTED and "triangle" in str(e.value)
        with pytest.raises(rtw.RtwError) as e:
            dw.mirror_points_device(d_rays.data_ptr(), d_hits.data_ptr(), n, m.cam, out.data_ptr(), out2.data_ptr())
        assert e.value.status == rtw.RTW_UNSUPPORTED and "triangle" in str(e.value)
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == 0xA5).all() and (out2.cpu().numpy() == 0xA5).all()
    finally:
        dw.close()
