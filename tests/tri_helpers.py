"""Worlds and meshes for the triangle tests (tests/test_tri_host.py, tests/test_gpu_tri_*.py).

The oracle cannot express a triangle, so the references are: the oracle's own worlds of axis-aligned
rects, whose rects the device holds as two triangles each (rect_tris winds them so that n = +e_k, and the
triangle's arithmetic then gives the rect's bits: csrc/rtw_tri.hpp); the host entry
rtw_world_trace_tri_host merged with the oracle's record of the other primitives (merge_hits); and the
render's own traversals against each other."""
import numpy as np


# ------------------------------------------------------------------ rects as triangles ----
def rect_tris(W, p):
    """The two triangles (dicts as helpers._to_desc takes) that tile the rect dict `p` along a diagonal,
    wound so that (v1 - v0) x (v2 - v0) points along +e_k."""
    a0, a1, b0, b1, k = [float(x) for x in p["a"][:5]]
    ax = {W.PRIM_XY_RECT: (0, 1, 2), W.PRIM_XZ_RECT: (0, 2, 1), W.PRIM_YZ_RECT: (1, 2, 0)}[p["kind"]]

    def pt(a, b):
        q = [0.0, 0.0, 0.0]
        q[ax[0]], q[ax[1]], q[ax[2]] = a, b, k
        return q

    c00, c10, c11, c01 = pt(a0, b0), pt(a1, b0), pt(a1, b1), pt(a0, b1)
    tris = [(c00, c10, c11), (c00, c11, c01)]
    e = np.zeros(3)
    e[ax[2]] = 1.0
    out = []
    for v0, v1, v2 in tris:
        if np.dot(np.cross(np.subtract(v1, v0), np.subtract(v2, v0)), e) < 0:
            v1, v2 = v2, v1
        q = {key: val for key, val in p.items() if key != "a"}
        q["kind"], q["a"] = W.PRIM_TRIANGLE, [*v0, *v1, *v2]
        out.append(q)
    return out


def triangulate(W, tables, keep=None):
    """tables = (prims, xforms, textures, mats, perlins, images) with every rect replaced by its two triangles in
    place (list order kept, so coincident pairs keep their tie), except rects for which keep(prim) holds.  Returns
    (tables, n_replaced)."""
    prims, rest = tables[0], tables[1:]
    out, n = [], 0
    for p in prims:
        if p["kind"] in (W.PRIM_XY_RECT, W.PRIM_XZ_RECT, W.PRIM_YZ_RECT) and not (keep and keep(p)):
            out += rect_tris(W, p)
            n += 1
        else:
            out.append(p)
    return (out, *rest), n


def reads_uv(W, tables):
    """keep() for triangulate: rects whose material reads an image texture (u, v differ between a rect and a triangle)."""
    _, _, tex, mats = tables[:4]

    def keep(p):
        m = mats[p["mat"]]
        return m["kind"] in (W.WMAT_LAMBERT, W.WMAT_LIGHT) and tex[m.get("tex", 0)]["kind"] == W.TEX_IMAGE
    return keep


# ------------------------------------------------------------------------------ meshes ----
def tetrahedron():
    v = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], float) / np.sqrt(3.0)
    return v, np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]])


def icosahedron():
    t = (1.0 + np.sqrt(5.0)) / 2.0
    v = np.array([[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t],
                  [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]], float)
    f = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2],
                  [10, 7, 6], [7, 1, 8], [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11],
                  [6, 2, 10], [8, 6, 7], [9, 8, 1]])
    return v / np.linalg.norm(v[0]), f


def icosphere(level):
    """Unit icosphere: 20 * 4^level faces, outward winding, shared vertices by index."""
    v, f = icosahedron()
    v = [tuple(x) for x in v]
    for _ in range(level):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                c = (np.array(v[a]) + np.array(v[b])) / 2
                v.append(tuple(c / np.linalg.norm(c)))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        f = np.array(nf)
    return np.array(v, float), np.array(f)


def mesh_dicts(W, v, f, mat, xform=-1):
    return [dict(kind=W.PRIM_TRIANGLE, mat=mat, xform=xform, a=[float(x) for x in v[list(t)].reshape(9)]) for t in f]


def rot_y(v, t):
    sn, cs = np.sin(t), np.cos(t)
    return np.stack([cs * v[:, 0] + sn * v[:, 2], v[:, 1], -sn * v[:, 0] + cs * v[:, 2]], 1)


# ------------------------------------------------------------------------------ worlds ----
T4_CAMERA = dict(look_from=(0.0, 4.0, 13.0), look_at=(0.0, 1.2, 0.0), vfov=40.0, aperture=0.05, focus=13.0)


def general_world(W, seed, n_meshes=14, n_spheres=40, earth=None):
    """T4(a): jittered icosahedra and tetrahedra (Lambert, metal, glass, light), every third one under a
    Translate / RotateY chain of 1-3 ops, among static spheres on a ground sphere; > 32 primitives, leaves of two.
    earth (an RGBA image): two more meshes carry an image texture, which reads the triangles' barycentrics."""
    from helpers import chain_to_object
    rng = np.random.default_rng(seed)
    tex = [dict(kind=W.TEX_CHECKER, odd=(0.2, 0.3, 0.1), even=(0.9, 0.9, 0.9)), dict(kind=W.TEX_SOLID, color=(4.0, 3.5, 3.0)),
           dict(kind=W.TEX_SOLID, color=(0.7, 0.3, 0.2)), dict(kind=W.TEX_SOLID, color=(0.2, 0.4, 0.7))]
    mats = [dict(kind=W.WMAT_LAMBERT, tex=0), dict(kind=W.WMAT_LIGHT, tex=1), dict(kind=W.WMAT_LAMBERT, tex=2),
            dict(kind=W.WMAT_LAMBERT, tex=3), dict(kind=W.WMAT_METAL, albedo=(0.8, 0.8, 0.9), fuzz=0.0),
            dict(kind=W.WMAT_METAL, albedo=(0.8, 0.6, 0.3), fuzz=0.3), dict(kind=W.WMAT_DIELECTRIC, ir=1.5)]
    prims, xf = [dict(kind=W.PRIM_SPHERE, mat=0, xform=-1, a=[0, -1000, 0, 0, -1000, 0, 1000.0, 0, 0])], []
    for i in range(n_meshes):
        v, f = icosahedron() if i % 2 == 0 else tetrahedron()
        s = rng.uniform(0.5, 1.0)
        v = v * s * (1 + 0.15 * rng.uniform(-1, 1, v.shape))
        centre = np.array([rng.uniform(-7, 7), s * 1.1 + rng.uniform(0, 1.5), rng.uniform(-6, 5)])
        xi = -1
        if i % 3 == 0:
            n_ops = 1 + (i // 3) % 3
            ops = [(W.XF_TRANSLATE if (k + i) % 2 == 0 else W.XF_ROTATE_Y) for k in range(n_ops)]
            vs = [tuple(float(x) for x in rng.uniform(-2, 2, 3)) if o == W.XF_TRANSLATE else
                  (float(np.sin(a)), float(np.cos(a)), float(a)) for o in ops for a in [rng.uniform(-1.2, 1.2)]]
            x = dict(n=n_ops, op=ops, v=vs)
            xf.append(x)
            xi, centre = len(xf) - 1, chain_to_object(x, centre)
        prims += mesh_dicts(W, v + centre, f, [2, 4, 6, 1, 3, 5][i % 6], xi)
    for i in range(n_spheres):
        r = float(rng.uniform(0.25, 0.55))
        c = (float(rng.uniform(-9, 9)), r, float(rng.uniform(-7, 6)))
        prims.append(dict(kind=W.PRIM_SPHERE, mat=[2, 3, 4, 5, 6][i % 5], xform=-1, a=[*c, *c, r, 0, 0]))
    imgs = []
    if earth is not None:
        tex.append(dict(kind=W.TEX_IMAGE, image=0))
        mats.append(dict(kind=W.WMAT_LAMBERT, tex=len(tex) - 1))
        imgs = [earth]
        for k, (v, f) in enumerate((icosahedron(), tetrahedron())):
            v = v * 1.6 * (1 + 0.1 * rng.uniform(-1, 1, v.shape)) + np.array([-2.5 + 5.0 * k, 2.2, 3.0])
            prims += mesh_dicts(W, v, f, len(mats) - 1)
    return prims, xf, tex, mats, [], imgs


ENCLOSURE_EMIT = (0.25, 0.5, 0.75)


def enclosure_world(W, seed, level=2):
    """T4(b): a jittered, rotated icosphere of solid-colour LIGHT triangles around the origin (the camera sits
    inside); with a black background every camera ray must end on the emit colour."""
    rng = np.random.default_rng(seed)
    v, f = icosphere(level)
    v = rot_y(v * 6.0 * (1 + 0.08 * rng.uniform(-1, 1, v.shape)), 0.37)
    v = v[:, [1, 0, 2]] * np.array([1.0, 1.0, 1.3])  # (tilted and stretched: no face is axis-aligned)
    f = f[:, [0, 2, 1]]  # (the axis swap mirrors the mesh: keep the winding outward)
    tex = [dict(kind=W.TEX_SOLID, color=ENCLOSURE_EMIT)]
    mats = [dict(kind=W.WMAT_LIGHT, tex=0)]
    return mesh_dicts(W, v, f, 0), [], tex, mats, [], []


def cards_world(W, earth, n_spheres=520, n_cards=24, seed=9):
    """T3: the spheres_image variant of helpers.mixed_bvh_world (untransformed spheres, >= kLeafOneMin) plus
    axis-aligned cards of all three orientations.  Returns (tables with the cards as rects, for the oracle)."""
    from helpers import mixed_bvh_world
    prims, xf, tex, mats, perl, imgs = mixed_bvh_world(W, earth, 0, n_spheres, 5, variant="spheres_image")
    rng = np.random.default_rng(seed)
    tex = tex + [dict(kind=W.TEX_SOLID, color=(0.8, 0.7, 0.2)), dict(kind=W.TEX_SOLID, color=(2.5, 2.0, 1.5))]
    mats = mats + [dict(kind=W.WMAT_LAMBERT, tex=len(tex) - 2), dict(kind=W.WMAT_LIGHT, tex=len(tex) - 1),
                   dict(kind=W.WMAT_METAL, albedo=(0.9, 0.9, 0.9), fuzz=0.05)]
    cards = []
    for i in range(n_cards):
        kind = (W.PRIM_XY_RECT, W.PRIM_XZ_RECT, W.PRIM_YZ_RECT)[i % 3]
        c = np.array([rng.uniform(-9, 9), rng.uniform(0.8, 3.5), rng.uniform(-7, 5)])
        s = rng.uniform(0.5, 1.4, 2)
        ax = {W.PRIM_XY_RECT: (0, 1, 2), W.PRIM_XZ_RECT: (0, 2, 1), W.PRIM_YZ_RECT: (1, 2, 0)}[kind]
        a = [c[ax[0]] - s[0], c[ax[0]] + s[0], c[ax[1]] - s[1], c[ax[1]] + s[1], c[ax[2]]]
        cards.append(dict(kind=kind, mat=len(mats) - 3 + i % 3, xform=-1, a=[float(x) for x in a], cls="card"))
    # cards in the middle of the list, so that spheres come before and after them
    half = len(prims) // 2
    return prims[:half] + cards + prims[half:], xf, tex, mats, perl, imgs


# ------------------------------------------------------------------- expected records ----
def split_triangles(W, tables):
    """(tables without the triangles, list index of each kept primitive in the full list)."""
    prims = tables[0]
    keep = [i for i, p in enumerate(prims) if p["kind"] != W.PRIM_TRIANGLE]
    return ([prims[i] for i in keep], *tables[1:]), np.array(keep, np.int64)


def merge_hits(tri, other, other_index):
    """The record of the whole world from the triangles' (rtw_world_trace_tri_host: prim = index in the full list + 1)
    and the other primitives' (the oracle's, prim = index among the non-triangles + 1): the smaller t; on a tie the
    later list index.  A NaN t never occurs in these sets (asserted)."""
    other = other.copy()
    hit_o = other["prim"] > 0
    other["prim"][hit_o] = other_index[other["prim"][hit_o] - 1] + 1
    hit_t = tri["prim"] > 0
    assert not np.isnan(tri["t"][hit_t]).any() and not np.isnan(other["t"][hit_o]).any()
    take_t = hit_t & (~hit_o | (tri["t"] < other["t"]) | ((tri["t"] == other["t"]) & (tri["prim"] > other["prim"])))
    out = other.copy()
    out[take_t] = tri[take_t]
    return out
