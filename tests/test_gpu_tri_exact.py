"""Device records of triangle hits against exact rational arithmetic (tests/tri_exact.py), not
against the host entry (which includes the header the kernels run).

E1: a tetrahedron, an icosahedron, a jittered level-2 icosphere, a 64-gon bipyramid, a sliver strip of aspect
10^4 : 1 and an icosahedron of size 2^-20 at offset ~1000, each twice: untransformed, and under a chain of its
own (1, 2, 3 and 4 ops, Translate and RotateY mixed); 40 static spheres and the ground sphere.  E2: the
untransformed half among enough untransformed spheres that the queries walk per lane.  Rays: the ladder of
tests/test_tri_exact_host.py (offsets 2^-20 .. 2^-54 of an edge length beside edges and about vertices), rays
aimed at vertices and edge points and 1-3 ulps beside, from world-space origins at world-space points of both
copies, and the 48x27 feature rays with their bounce, inward and shadow rays.

Per ray tri_exact gives the exact winner among the triangles and whether rounding could have changed it
(`decided`); the spheres' record is the oracle's, merged by tri_helpers.merge_hits.  A decided ray's prim and
front are exact, its t, p, u, v and normal within §22's bounds of the exact ones (a sphere's record equals the
oracle's bits); an undecided ray may return only a triangle that is `in` or `band` and in reach, with that
triangle's record; a ray with an `in` triangle inside its interval must hit and must be occluded, a ray whose
every triangle is `out` and which the oracle's spheres miss must not be.  (The six meshes, twice, hold 992
triangles, so E1 has 1033 primitives.)"""
from collections import Counter
from fractions import Fraction as Fr

import numpy as np
import pytest

from helpers import chain_to_object, chain_to_world
import query_helpers as Q
import tri_helpers as T
import tri_exact as X
from test_tri_exact_host import DECIDED_RUNG, make_chain

pytestmark = pytest.mark.gpu

SKY = (0.7, 0.8, 1.0)
CAMERA = dict(look_from=(0.0, 4.5, 14.0), look_at=(0.0, 1.6, 0.0), vfov=42.0, focus=13.0)
# where each mesh stands untransformed (a dyadic offset: the vertices keep short significands), where its chained
# copy stands in the world, and that copy's chain (op, value); the tiny mesh's chain starts with the Translate
# that carries its offset, the sliver's is one Translate: see the conditions in reference()
PLACE = {"tetrahedron": ((-7.0, 1.5, 1.0), (-6.0, 1.5, 5.0), [(1, 0.7), (0, (1.5, 0.25, -1.0))]),
         "icosahedron": ((-4.0, 1.5, -1.5), (-2.5, 1.25, 4.5), [(0, (1.5, -0.25, 2.0)), (1, -0.4)]),
         "icosphere": ((0.0, 2.0, -2.5), (6.5, 2.0, -4.0), [(1, 0.9), (0, (-2.0, 0.5, 1.25)), (1, -1.1)]),
         "bipyramid": ((4.0, 1.5, 0.5), (2.0, 1.5, 5.5), [(0, (0.5, 1.0, -1.5)), (1, 0.35), (0, (2.0, 0.0, 0.75)), (1, 1.2)]),
         "sliver": ((-1.0, 4.5, 2.0), (-1.5, 3.5, 6.0), [(0, (-1.5, 3.5, 6.0))]),
         "tiny": (None, None, [(0, (-1000.5, 2.0, 1000.25)), (1, 0.8), (1, -0.3)])}
LADDER_TRIS = {"tetrahedron": (0, 3), "icosahedron": (1, 14), "icosphere": (7, 200), "bipyramid": (5, 64 + 30),
               "sliver": (0, 3), "tiny": (2, 17)}


@pytest.fixture(scope="module")
def W():
    from rtw_amd import world
    return world


def mesh_set():
    M = X.meshes()
    lv, lf = X.sliver_strip(quads=2, length=2.5, centred=True)
    M["sliver"] = (X.f32(lv), lf, 8.0)
    return M


def build_world(W, chained, n_spheres, seed=3):
    """(tables, targets): targets = [(mesh, copy, world-space triangle (3, 3), near, its exact vertices or None)]."""
    rng = np.random.default_rng(seed)
    tex = [dict(kind=W.TEX_CHECKER, odd=(0.2, 0.3, 0.1), even=(0.9, 0.9, 0.9)), dict(kind=W.TEX_SOLID, color=(0.7, 0.3, 0.2)),
           dict(kind=W.TEX_SOLID, color=(0.2, 0.4, 0.7))]
    mats = [dict(kind=W.WMAT_LAMBERT, tex=0), dict(kind=W.WMAT_LAMBERT, tex=1), dict(kind=W.WMAT_LAMBERT, tex=2),
            dict(kind=W.WMAT_METAL, albedo=(0.8, 0.8, 0.9), fuzz=0.0), dict(kind=W.WMAT_DIELECTRIC, ir=1.5)]
    prims = [dict(kind=W.PRIM_SPHERE, mat=0, xform=-1, a=[0, -1000, 0, 0, -1000, 0, 1000.0, 0, 0])]
    xf, targets = [], []
    for name, (v, f, near) in mesh_set().items():
        at, at_chained, ops = PLACE[name]
        vu = v if at is None else v + np.array(at)
        prims += T.mesh_dicts(W, vu, f, 1 + len(prims) % 4)
        targets += [(name, "plain", vu[f[i]], near, None) for i in LADDER_TRIS[name]]
        if not chained:
            continue
        x = make_chain(ops)
        xf.append(x)
        if name == "tiny":    # object space: the mesh about the origin; the chain's first Translate carries it away
            vo = v - np.array([1000.25, 1.5, -999.75])
        elif name == "sliver":
            vo = v
        else:
            vo = v + np.round(chain_to_object(x, at_chained) * 256.0) / 256.0
        prims += T.mesh_dicts(W, vo, f, 1 + len(prims) % 4, len(xf) - 1)
        for i in LADDER_TRIS[name]:  # (the world-space vertices exactly too: doubles are too coarse for the tiny mesh's rungs)
            ex = [X.chain_world(x, X.fr3(q), (0, 0, 0))[0] for q in vo[f[i]]]
            targets.append((name, "chained", np.array([chain_to_world(x, q) for q in vo[f[i]]]), near, ex))
    for i in range(n_spheres):
        r = float(rng.uniform(0.25, 0.55)) if n_spheres <= 64 else float(rng.uniform(0.1, 0.3))
        c = (float(rng.uniform(-9, 9)), r, float(rng.uniform(-7, 7)))
        prims.append(dict(kind=W.PRIM_SPHERE, mat=1 + i % 4, xform=-1, a=[*c, *c, r, 0, 0]))
    return (prims, xf, tex, mats, [], []), targets


class Reference:
    """One world: its description, the ray sets and, per ray, the exact trace over the triangles and the oracle's
    record over the rest; computed once, on the CPU."""

    def __init__(self, rtw, oracle, W, name):
        from test_gpu_tri_query import Merged
        self.name = name
        tables, targets = build_world(W, chained=name == "E1", n_spheres=40 if name == "E1" else 330)
        self.m = Merged(rtw, oracle, W, tables, dict(CAMERA, aperture=0.0))
        self.prims, self.desc = tables[0], self.m.desc
        self.exact = X.World(tables[0], tables[1], W.PRIM_TRIANGLE)
        self.row_of = {k: i for i, k in enumerate(self.exact.rows)}
        self.chained_rows = {i for i, q in enumerate(tables[0]) if q["kind"] == W.PRIM_TRIANGLE and q["xform"] >= 0}
        rows, self.labels = [], []
        for j, (mesh, copy, tri, near, ex) in enumerate(targets):
            own = self._row(tri, tables, copy)
            for o, d, rung, side in X.ladder(tri, 300 + j, near, exact=ex) + X.exact_points(tri, 400 + j, near):
                rows.append((o, d, 0.5, 0.001, np.inf))
                self.labels.append((mesh, copy, rung, side, own))
        ladder = Q.make_rays(rtw, rows)
        # (the bounce, inward and shadow rays start from the host entry's hit points: a way to place rays, no reference)
        feat, kinds = Q.ray_set(rtw, self.m, self.m.cam, self.m.look_from, 100, w=48, h=27)
        self.n_ladder = len(ladder)
        self.rays = np.concatenate([ladder, feat])
        assert len(self.rays) <= 20000
        self.traces = self.exact.trace(self.rays)
        self.other = Q.oracle_hits(rtw, self.m.ow, self.rays)
        self.index = self.m.index
        self.rtw = rtw
        self._expected()

    def _row(self, tri, tables, copy):
        """The index in self.exact.tris of the triangle whose world-space vertices are `tri`."""
        for i, k in enumerate(self.exact.rows):
            q, t = tables[0][k], self.exact.tris[i]
            if (q["xform"] >= 0) != (copy == "chained"):
                continue
            v = np.array(t.a).reshape(3, 3)
            if q["xform"] >= 0:
                v = np.array([chain_to_world(tables[1][q["xform"]], x) for x in v])
            if np.array_equal(v, tri):
                return i
        raise AssertionError("target triangle not found")

    def _expected(self):
        """Merge each ray's exact trace with the oracle's record: decided[i], and the record a decided ray has."""
        rtw, n = self.rtw, len(self.rays)
        tri = np.zeros(n, rtw.HIT_DTYPE)
        self.decided = np.zeros(n, bool)
        self.must_hit = np.zeros(n, bool)
        self.all_out = np.zeros(n, bool)
        for i, tr in enumerate(self.traces):
            oh = self.other[i]
            ts = Fr(float(oh["t"])) if oh["prim"] > 0 else None
            dec = tr.decided
            if ts is not None:
                # the sphere's root against every triangle that may be returned: clear of each by its t bound
                if any(abs(r.t - ts) <= tr.tols[k] for k, r in tr.allowed.items()):
                    dec = False
                elif tr.hit is None or tr.rec.t > ts:  # the sphere's record, unless a band triangle lies before it
                    dec = not tr.edge and not any(r.t < ts for r in tr.allowed.values())
            self.decided[i] = dec
            self.must_hit[i] = tr.must_hit or oh["prim"] > 0
            self.all_out[i] = not tr.cls and oh["prim"] == 0
            if tr.hit is not None:
                r = tr.rec
                r.p is None and r._exact()
                tri[i]["t"], tri[i]["p"] = float(r.t), [float(c) for c in r.p]
                tri[i]["prim"], tri[i]["front"] = self.exact.rows[tr.hit] + 1, int(r.front)
        self.want = T.merge_hits(tri, self.other, self.index)

    def conditions(self):
        """The issue's conditions on the sets, from the reference alone; prints the per-rung table."""
        table = Counter()
        for lab, tr in zip(self.labels, self.traces[:self.n_ladder]):
            mesh, copy, rung, side, own = lab
            table[(mesh, copy, rung, side, tr.cls.get(own, "out"))] += 1
        print(f"{self.name}: ladder rays against their own triangle: mesh copy rung side in/out/band")
        for mesh, copy in sorted({k[:2] for k in table}):
            for rung in sorted({k[2] for k in table if k[:2] == (mesh, copy)}):
                cells = [f"{side:+d}:" + "/".join(str(table[(mesh, copy, rung, side, c)]) for c in ("in", "out", "band"))
                         for side in (1, -1, 0) if any(table[(mesh, copy, rung, side, c)] for c in ("in", "out", "band"))]
                print(f"  {mesh:12s} {copy:8s} {rung:3d}  " + "  ".join(cells))
        for (mesh, copy, rung, side, cls), cnt in table.items():
            if 20 <= rung <= DECIDED_RUNG and cls == "band":
                raise AssertionError((self.name, mesh, copy, rung, side, cnt, "a band ray on a rung that must be decided"))
        feat = slice(self.n_ladder, len(self.rays))
        und = 1.0 - self.decided[feat].mean()
        print(f"{self.name}: rays {len(self.rays)} (ladder {self.n_ladder}); undecided: feature set {und:.4f}, all {1 - self.decided.mean():.4f}")
        assert und <= 0.02, und
        hit = self.decided & (self.want["prim"] > 0)
        rows = self.want["prim"][hit].astype(np.int64) - 1
        on_tri = np.isin(rows, self.exact.rows)
        on_chain = np.isin(rows, list(self.chained_rows))
        print(f"{self.name}: decided hits {hit.sum()}, on triangles {on_tri.mean():.3f}, of those chained {on_chain.sum() / max(1, on_tri.sum()):.3f}")
        assert on_tri.mean() >= 0.30
        if self.name == "E1":
            assert on_chain.sum() >= 0.25 * on_tri.sum()
        else:
            assert not self.chained_rows  # (E2 holds no chain by construction)
        assert set(self.want["front"][hit][on_tri].tolist()) == {0, 1} and (~on_tri).any()
        f_hit = hit[feat]
        assert 0.1 <= f_hit.mean() <= 0.98 and (self.decided[feat] & (self.want["prim"][feat] == 0)).any()

    def check(self, got, occ, where, ratios):
        """The device's closest-hit records and occlusion bytes against the reference."""
        bad = []
        for i, tr in enumerate(self.traces):
            g, k = got[i], int(got[i]["prim"]) - 1
            is_tri = k in self.row_of
            if self.decided[i] and k + 1 != int(self.want["prim"][i]):
                bad.append((i, "prim", k + 1, int(self.want["prim"][i])))
                continue
            if self.must_hit[i] and k < 0:
                bad.append((i, "a ray with an inside triangle or a sphere in its interval misses"))
            if self.must_hit[i] and not occ[i]:
                bad.append((i, "not occluded"))
            if self.all_out[i] and (occ[i] or k >= 0):
                bad.append((i, "a ray that misses everything is occluded or hits"))
            if k < 0:
                continue
            if is_tri:
                idx = self.row_of[k]
                if idx not in tr.allowed:
                    bad.append((i, "an out triangle is returned", k))
                    continue
                key = "chained" if k in self.chained_rows else "plain"
                for what in tr.allowed[idx].compare(g, ratios.setdefault(key, {})):
                    bad.append((i, what, k))
            else:  # a sphere: the oracle's record, bit for bit
                o = self.other[i].copy()
                if o["prim"] == 0 or self.index[o["prim"] - 1] != k:
                    bad.append((i, "a sphere the oracle does not return", k))
                    continue
                o["prim"] = k + 1
                if not np.array_equal(Q.words(np.array([g])), Q.words(np.array([o]))):
                    bad.append((i, "a sphere's record differs from the oracle's", k))
        assert not bad, (where, len(bad), bad[:6])


_REFS = {}


def reference(rtw, oracle, W, name):
    if name not in _REFS:
        _REFS[name] = Reference(rtw, oracle, W, name)
    return _REFS[name]


@pytest.mark.parametrize("name", ["E1", "E2"])
def test_device_records_against_exact_rationals(rtw, oracle, W, name):
    ref = reference(rtw, oracle, W, name)
    ref.conditions()
    bvh, lin = W.DeviceWorld(ref.desc), W.DeviceWorld(ref.desc, linear=True)
    try:
        union, lane = rtw.QueryOpts(rtw.WORLD_TRAVERSAL["union"], 0), rtw.QueryOpts(rtw.WORLD_TRAVERSAL["lane"], 0)
        assert bvh.bvh_info()["nodes"] > 0 and bvh.query_info()["feature_set"] & 64
        if name == "E1":
            assert len(ref.prims) < 1100 and {x["n"] for x in ref.m.tables[1]} == {1, 2, 3, 4}
            runs = [(bvh, None, "bvh auto"), (bvh, union, "bvh union"), (lin, None, "linear")]
        else:
            assert bvh.bvh_info()["nodes"] >= 256
            for o in (lane, None):
                qi = bvh.query_info(o)
                assert qi["traversal"] == "lane" and qi["feature_set"] & 16 and qi["feature_set"] & 64, qi
            assert bvh.query_info(union)["traversal"] == "union"
            runs = [(bvh, lane, "bvh lane"), (bvh, None, "bvh auto"), (bvh, union, "bvh union")]
        d_rays, n = Q.to_device(ref.rays), len(ref.rays)
        ratios = {}
        for dev, opts, label in runs:
            got, guard = Q._trace(rtw, dev, d_rays, n, opts)
            assert (guard == 0xA5).all(), (name, label)
            occ, guard = Q._trace(rtw, dev, d_rays, n, opts, occluded=True)
            assert (guard == 0xA5).all(), (name, label, "occluded")
            ref.check(got, occ, (name, label), ratios)
        print(f"{name}: device, largest error / bound:", {k: {q: float(f"{x:.3g}") for q, x in sorted(v.items())} for k, v in ratios.items()})
        assert all(x <= 1.0 for v in ratios.values() for x in v.values())
    finally:
        bvh.close()
        lin.close()
