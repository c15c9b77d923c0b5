"""Scenes and ray sets of the scene API's tests (tests/test_gpu_scene_queries.py,
tests/test_scene_query_cpu.py): what scene_query_kernel, scene_guides_kernel and
scene_surface_kernel are asked beyond cover_scene(42).

Every scene is a product scene (rtw_sphere / rtw_material arrays) mirrored into an
oracle.TableWorld: prim kind 0 or 1 with a = c0, c1, r, t0, t1; a material becomes Lambert
over a solid or a checker texture (albedo the EVEN colour, albedo_odd the odd one), Metal or
Dielectric.  The scenes:

  custom     test_gpu_parity.custom_scene: hollow glass, a mover with range [0.25, 0.75], a wide mover
  clustered  test_gpu_parity.clustered_scene: 102 spheres, three time groups
  ties       40 spheres with four bitwise-identical pairs of different materials; in pair C the
             earlier list entry is a mover with c0 == c1 and the later one static, so the table
             (static first) holds them in the opposite order
  limits     4096 spheres, 4096 materials, 64 time ranges; list sphere 4095 (material 4095, time
             group 63) stands alone in front of the camera
  empty, one no sphere; a single static sphere

and per scene the ray sets (Scene.sets()): the 48x27 feature rays with random times plus bounce,
inward and shadow rays (query_helpers.ray_set), that set at five times, the interval variants
V1-V5, rays from inside spheres, rays at the pairs, and directions of length 2^520 .. 2^1000 and
2^-560.  The oracle's records are computed once per process and are read-only."""
import types

import numpy as np

import query_helpers as Q
from surface_helpers import guides_of, host_frame_rays, texture_value

FW, FH = 48, 27
BACKGROUND = (0.7, 0.8, 1.0)
TIMES = (-0.75, 0.1, 0.5, 1.5, 3.0)
VARIANTS = ("V1", "V2", "V3", "V4", "V5")
SCENES = ("custom", "clustered", "ties", "limits", "empty", "one")
OVERFLOW_SCENES = ("custom", "ties", "one")
SHUTTERS = ((0.0, 1.0), (0.25, 2.0))  # the second leaves two of clustered's groups; its mid time 1.125 leaves [0, 1]
ROWS = (None, (5, 1, 9), (3, 4, 6))  # (row_begin, row_stride, row_count) of a guides call
LIMITS_LAST = 4095
LIMITS_LAST_RANGE = (0.3, 1.7)


def _fill(rtw, specs, mat_specs):
    """specs: (c0, c1, radius, t0, t1, moving, mat); mat_specs: (kind, albedo, albedo_odd, fuzz, ir)."""
    sph = (rtw.Sphere * len(specs))()
    for s, (c0, c1, r, t0, t1, mv, m) in zip(sph, specs):
        s.c0[:], s.c1[:] = c0, c1
        s.radius, s.t0, s.t1, s.moving, s.mat = r, t0, t1, mv, m
    mats = (rtw.Material * len(mat_specs))()
    for m, (kind, albedo, odd, fuzz, ir) in zip(mats, mat_specs):
        m.kind, m.fuzz, m.ir = kind, fuzz, ir
        m.albedo[:], m.albedo_odd[:] = albedo, odd
    return sph, mats


# ties: name -> (list index of the earlier entry, of the later one)
TIE_PAIRS = {"A": (3, 20), "B": (5, 27), "C": (8, 25), "D": (10, 30)}


def ties_scene(rtw):
    """Four coincident pairs on a row in front of the camera, 31 unrelated spheres behind them, the ground.
    A: two static spheres.  B: two movers with the same c0, c1, t0, t1.  C: a mover with c0 == c1 listed first
    (its centre is c0 + 0 * fraction = c0 at every time: the same roots), the same sphere static listed later.
    D: the static one first, the mover later."""
    rng = np.random.default_rng(31)
    L, C_, M, D = rtw.LAMBERT_SOLID, rtw.LAMBERT_CHECKER, rtw.METAL, rtw.DIELECTRIC
    mat_specs = [(C_, (0.9, 0.9, 0.9), (0.2, 0.3, 0.1), 0.0, 0.0),
                 (L, (0.8, 0.1, 0.1), (0, 0, 0), 0.0, 0.0), (M, (0.1, 0.8, 0.1), (0, 0, 0), 0.25, 0.0),     # A
                 (M, (0.7, 0.6, 0.5), (0, 0, 0), 0.0, 0.0), (D, (0, 0, 0), (0, 0, 0), 0.0, 1.5),             # B
                 (D, (0, 0, 0), (0, 0, 0), 0.0, 2.4), (C_, (0.1, 0.1, 0.9), (0.9, 0.9, 0.1), 0.0, 0.0),      # C
                 (L, (0.3, 0.3, 0.9), (0, 0, 0), 0.0, 0.0), (L, (0.9, 0.5, 0.1), (0, 0, 0), 0.0, 0.0),       # D
                 (L, (0.5, 0.5, 0.5), (0, 0, 0), 0.0, 0.0), (M, (0.8, 0.8, 0.9), (0, 0, 0), 1.0, 0.0),
                 (D, (0, 0, 0), (0, 0, 0), 0.0, 1.33)]
    pair = {"A": ((-4.5, 1.0, 0.5), (-4.5, 1.0, 0.5), 0.0, 0.0), "B": ((-1.5, 1.0, 0.5), (-1.5, 1.6, 0.5), 0.0, 1.0),
            "C": ((1.5, 1.0, 0.5), (1.5, 1.0, 0.5), 0.0, 1.0), "D": ((4.5, 1.0, 0.5), (4.5, 1.0, 0.5), 0.0, 1.0)}
    moving = {"A": (0, 0), "B": (1, 1), "C": (1, 0), "D": (0, 1)}
    mat_of = {"A": (1, 2), "B": (3, 4), "C": (5, 6), "D": (7, 8)}
    specs = [None] * 40
    specs[0] = ((0, -1000, 0), (0, -1000, 0), 1000.0, 0.0, 0.0, 0, 0)
    for name, idx in TIE_PAIRS.items():
        c0, c1, t0, t1 = pair[name]
        for k in range(2):
            mv = moving[name][k]
            specs[idx[k]] = (c0, c1, 0.8, t0 if mv else 0.0, t1 if mv else 0.0, mv, mat_of[name][k])
    ranges = [(0.0, 1.0), (-0.5, 1.5), (0.2, 0.8)]
    for i in range(40):
        if specs[i] is not None:
            continue
        r = 0.3 + 0.3 * rng.random()
        c0 = (-7 + 14 * rng.random(), r, -8 + 5 * rng.random())
        if i % 3 == 0:
            t0, t1 = ranges[(i // 3) % 3]
            c1 = (c0[0] + 0.5 * rng.random(), c0[1] + 0.5 * rng.random(), c0[2])
            specs[i] = (c0, c1, r, t0, t1, 1, 9 + i % 3)
        else:
            specs[i] = (c0, c0, r, 0.0, 0.0, 0, 9 + i % 3)
    return _fill(rtw, specs, mat_specs)


def _limits_range(g):
    """63 distinct time ranges in three families; the third excludes the times 0.1 and 0.5."""
    if g % 3 == 0:
        return 0.0, 1.0 + 0.01 * g
    if g % 3 == 1:
        return -1.0 - 0.01 * g, 2.0
    return 0.6 + 0.005 * g, 1.6


def limits_scene(rtw, n=4096, extra_range=False):
    """The tops of the packed meta word's fields: list index 4095, material index 4095, time group 63.  Sphere 0 is
    the ground, spheres 1 .. 4094 a 64-wide grid of small spheres behind the look-at point (every fifth a mover in
    one of 63 ranges), sphere 4095 a mover with a 64th range of its own, alone between the camera and the grid.
    n = 4097 and extra_range (a 65th range) are the two the library must refuse."""
    rng = np.random.default_rng(4096)
    kinds = (rtw.LAMBERT_CHECKER, rtw.LAMBERT_SOLID, rtw.METAL, rtw.DIELECTRIC)
    nm = 4096
    col, odd = rng.random((nm, 3)), rng.random((nm, 3))
    mat_specs = [(kinds[i % 4], tuple(col[i]), tuple(odd[i]), 0.25 * (i % 5), 1.3 + 0.0001 * i) for i in range(nm)]
    specs = [((0, -1000, 0), (0, -1000, 0), 1000.0, 0.0, 0.0, 0, 0)]
    for i in range(1, n):
        q = (i - 1) % 4094
        c0 = (-15.75 + 0.5 * (q % 64), 0.18, -3.0 - 0.6 * (q // 64))
        if i % 5 == 0:
            g = (i // 5) % 63
            t0, t1 = _limits_range(g)
            dv = [0.0, 0.0, 0.0]
            dv[g % 3] = 0.25
            specs.append((c0, tuple(c + d for c, d in zip(c0, dv)), 0.18, t0, t1, 1, i % nm))
        else:
            specs.append((c0, c0, 0.18, 0.0, 0.0, 0, i % nm))
    t0, t1 = LIMITS_LAST_RANGE
    specs[LIMITS_LAST] = ((-0.2, 4.68, 7.18), (0.6, 4.68, 7.18), 0.5, t0, t1, 1, LIMITS_LAST)
    if extra_range:
        c0, c1, r, _, _, _, m = specs[5]
        specs[5] = (c0, c1, r, 9.0, 10.0, 1, m)
    return _fill(rtw, specs, mat_specs)


def one_scene(rtw):
    return _fill(rtw, [((0.0, 1.0, 0.0), (0.0, 1.0, 0.0), 1.0, 0.0, 0.0, 0, 0)],
                 [(rtw.LAMBERT_CHECKER, (0.9, 0.9, 0.9), (0.2, 0.3, 0.1), 0.0, 0.0)])


# name -> (look_from, look_at, vfov); spheres whose inside rays start from: (centre, radius, where)
CAMERAS = {"custom": ((9.0, 2.0, 5.0), (0.5, 0.5, 0.5), 30.0), "clustered": ((13.0, 2.0, 3.0), (0.0, 0.3, 0.0), 30.0),
           "ties": ((0.0, 2.5, 12.0), (0.0, 1.0, 0.0), 40.0), "limits": ((0.0, 6.0, 12.0), (0.0, 0.0, -10.0), 40.0),
           "empty": ((13.0, 2.0, 3.0), (0.0, 0.0, 0.0), 20.0), "one": ((0.0, 2.0, 8.0), (0.0, 1.0, 0.0), 30.0)}
GROUND = ((0.0, -1000.0, 0.0), 1000.0, "top")
INSIDE = {"custom": (((0.0, 1.0, 0.0), 0.9, "ball"), GROUND), "clustered": (GROUND,), "ties": (GROUND,), "limits": (GROUND,),
          "empty": (), "one": (((0.0, 1.0, 0.0), 1.0, "ball"),)}


def table_world(rtw, oracle, sph, mats):
    """The scene as an oracle.TableWorld; material i's texture (Lambert only) is texture i."""
    prims = [{"kind": oracle.RW_MOVING if s.moving else oracle.RW_SPHERE, "mat": int(s.mat), "xform": -1,
              "a": [*s.c0, *s.c1, s.radius, s.t0, s.t1]} for s in (sph or ())]
    texs, omats = [], []
    for m in (mats or ()):
        if m.kind == rtw.LAMBERT_CHECKER:
            texs.append({"kind": oracle.RW_TEX_CHECKER, "even": list(m.albedo), "odd": list(m.albedo_odd)})
        else:
            texs.append({"kind": oracle.RW_TEX_SOLID, "color": list(m.albedo)})
        if m.kind == rtw.METAL:
            omats.append({"kind": oracle.RW_METAL, "albedo": list(m.albedo), "fuzz": m.fuzz})
        elif m.kind == rtw.DIELECTRIC:
            omats.append({"kind": oracle.RW_DIELECTRIC, "ir": m.ir})
        else:
            omats.append({"kind": oracle.RW_LAMBERT, "tex": len(texs) - 1})
    return oracle.TableWorld(prims, textures=texs, materials=omats, background=BACKGROUND)


def scene_surface(rtw, oracle, sc, hits):
    """The surface records of hit records over scene `sc`, from its sphere and material arrays and the oracle's
    checker value at the record's p -> (n,) SURFACE_DTYPE; a miss (prim 0 or beyond the list) all zero.  The
    kinds are the world's enumerations + 1: Lambert 1 (tex_kind 1 solid, 2 checker; tex 0), Metal 2, Dielectric 3."""
    out = np.zeros(len(hits), rtw.SURFACE_DTYPE)
    n = len(sc.sph) if sc.sph is not None else 0
    for i, h in enumerate(hits):
        k = int(h["prim"])
        if k == 0 or k > n:
            continue
        mi = int(sc.sph[k - 1].mat)
        m = sc.mats[mi]
        out["mat"][i] = mi + 1
        if m.kind == rtw.METAL:
            out["kind"][i], out["value"][i], out["fuzz"][i] = 2, list(m.albedo), m.fuzz
        elif m.kind == rtw.DIELECTRIC:
            out["kind"][i], out["value"][i], out["ir"][i] = 3, (1.0, 1.0, 1.0), m.ir
        else:
            out["kind"][i], out["tex_kind"][i] = 1, m.kind + 1
            out["value"][i] = (texture_value(oracle, sc.oracle, mi, h["u"], h["v"], h["p"]) if m.kind == rtw.LAMBERT_CHECKER
                               else list(m.albedo))
    return out


def _unit(rng):
    v = rng.normal(size=3)
    return v / np.sqrt((v * v).sum())


class Scene:
    """One scene on both sides, its cameras, its ray sets and the oracle's records of them."""

    def __init__(self, rtw, oracle, name):
        self.name, self._rtw, self._oracle = name, rtw, oracle
        if name == "custom":
            from test_gpu_parity import custom_scene
            self.sph, self.mats = custom_scene(rtw)
        elif name == "clustered":
            from test_gpu_parity import clustered_scene
            self.sph, self.mats = clustered_scene(rtw)
        elif name == "empty":
            self.sph, self.mats = None, None
        else:
            self.sph, self.mats = {"ties": ties_scene, "limits": limits_scene, "one": one_scene}[name](rtw)
        self.n = len(self.sph) if self.sph is not None else 0
        self.oracle = table_world(rtw, oracle, self.sph, self.mats)
        self.look_from, self.look_at, self.vfov = CAMERAS[name]
        self.moving = np.array([bool(s.moving) for s in (self.sph or ())], bool)
        self.radius = np.array([s.radius for s in (self.sph or ())], float)
        self.t0 = np.array([s.t0 for s in (self.sph or ())], float)
        self.t1 = np.array([s.t1 for s in (self.sph or ())], float)
        self._sets, self._frames = None, {}

    def camera(self, shutter=(0.0, 1.0)):
        return self._rtw.camera_init(self.look_from, self.look_at, (0, 1, 0), self.vfov, FW / FH, 0.0, 10.0, *shutter)

    # ------------------------------------------------------------------ ray sets --
    def _inside_rays(self, rng):
        rows = []
        for c, r, where in INSIDE[self.name]:
            c = np.array(c)
            for _ in range(48):
                if where == "ball":  # anywhere inside, up to 0.8 r from the centre
                    o = c + 0.8 * r * rng.random() * _unit(rng)
                else:  # below the top of the ground sphere, under the scene
                    up = np.array([rng.normal() * 0.004, 1.0, rng.normal() * 0.004])
                    o = c + (r - 0.5 - 30.0 * rng.random()) * up / np.sqrt((up * up).sum())
                rows.append((o, _unit(rng) * (0.5 + rng.random()), float(rng.random()), 0.001, np.inf))
        return rows

    def pair_center(self, name, time):
        s = self.sph[TIE_PAIRS[name][0]]
        c0, c1 = np.array(s.c0), np.array(s.c1)
        return c0 + (c1 - c0) * ((time - s.t0) / (s.t1 - s.t0)) if s.moving else c0

    def _tie_rays(self, rng):
        """At each pair: at its centre and four points off it, from the camera and from one unit in front of the
        surface.  self.tie_rows[name] = the rows of the "ties" set aimed at pair `name`."""
        rows, self.tie_rows = [], {}
        cam = np.array(self.look_from)
        for name in TIE_PAIRS:
            mine = []
            for dx, dy in ((0.0, 0.0), (0.4, 0.0), (-0.4, 0.1), (0.0, 0.45), (0.2, -0.4)):
                time = float(rng.random())
                c = self.pair_center(name, time)
                to_cam = (cam - c) / np.sqrt(((cam - c) ** 2).sum())
                for o in (cam, c + 1.8 * to_cam):
                    mine.append(len(rows))
                    rows.append((o, (c + np.array([dx, dy, 0.0])) - o, time, 0.001, np.inf))
            self.tie_rows[name] = mine
        return rows

    def _overflow_rays(self, rng):
        """40 directions of length 2^520 .. 2^1000 (|dir|^2 overflows: disc = inf - inf), from the camera, from inside
        a sphere, from above the scene and from an origin of that size too, towards the scene and away from it;
        then 8 directions of length 2^-560 from the camera (|dir|^2 and half_b^2 underflow to 0: a root of +-inf),
        six towards the scene and two away.  Every component is non-zero."""
        rows = []
        cam, at = np.array(self.look_from), np.array(self.look_at)
        inside = np.array(INSIDE[self.name][0][0]) + np.array([0.05, 0.1, -0.07])
        for j in range(40):
            k = 520 + (j * 480) // 39
            o = (cam, inside, at + np.array([0.3, 6.0, 0.2]), _unit(rng) * np.ldexp(1.0, 520 + 12 * j))[j % 4]
            d = (at - o) if j % 4 != 3 else _unit(rng)
            d = d / np.sqrt((d * d).sum()) + 0.2 * _unit(rng)
            if (j // 4) % 2:
                d = -d
            rows.append((o, np.ldexp(d / np.sqrt((d * d).sum()), k), float(rng.random()), 0.001, np.inf))
        for j in range(8):
            d = (at + 0.5 * _unit(rng)) - cam
            d = d / np.sqrt((d * d).sum())
            rows.append((cam, np.ldexp(-d if j >= 6 else d, -560), float(rng.random()), 0.001, np.inf))
        return rows

    def sets(self):
        """{set name: (rays, oracle records)}; "main" carries self.kinds."""
        if self._sets is not None:
            return self._sets
        rtw, seed = self._rtw, 2200 + SCENES.index(self.name)
        rng = np.random.default_rng(seed)
        out = {}

        def add(key, rays):
            ref = Q.oracle_hits(rtw, self.oracle, rays)
            rays.setflags(write=False)
            ref.setflags(write=False)
            out[key] = (rays, ref)
        main, self.kinds = Q.ray_set(rtw, self.oracle, self.camera(), self.look_from, seed, FW, FH)
        add("main", main)
        for t in TIMES:
            r = main.copy()
            r["time"] = t
            add(f"time{t}", r)
        base = types.SimpleNamespace(rays=out["main"][0], ref=out["main"][1])
        for v in VARIANTS:
            add(v, Q._interval(base, v))
        if INSIDE[self.name]:
            add("inside", Q.make_rays(rtw, self._inside_rays(rng)))
        if self.name == "ties":
            add("ties", Q.make_rays(rtw, self._tie_rays(rng)))
        if self.name in OVERFLOW_SCENES:
            add("overflow", Q.make_rays(rtw, self._overflow_rays(rng)))
        self._sets = out
        return out

    # -------------------------------------------------------------------- frames --
    def frame(self, shutter):
        """The 48x27 frame of camera `shutter`: (camera, feature rays, oracle hits, surface records, guides)."""
        if shutter not in self._frames:
            rtw = self._rtw
            cam = self.camera(shutter)
            rays = host_frame_rays(rtw, cam, FW, FH)
            hits = Q.oracle_hits(rtw, self.oracle, rays)
            surf = scene_surface(rtw, self._oracle, self, hits)
            guides = guides_of(rtw, hits, surf, BACKGROUND)
            for a in (rays, hits, surf, guides):
                a.setflags(write=False)
            self._frames[shutter] = (cam, rays, hits, surf, guides)
        return self._frames[shutter]

    # -------------------------------------------------------------------- census --
    def time_groups(self):
        """The distinct (t0, t1) of the movers in list order of their first appearance: the packed group indices."""
        seen = []
        for s in (self.sph or ()):
            if s.moving and (s.t0, s.t1) not in seen:
                seen.append((s.t0, s.t1))
        return seen

    def table_position(self):
        """List index -> position in the packed table [static wide | static | moving wide | moving]
        (rtw_scene_pack.cpp; wide: radius >= 100)."""
        key = [(2 * int(s.moving) + int(not s.radius >= 100.0), i) for i, s in enumerate(self.sph or ())]
        pos = np.zeros(self.n, int)
        for p, (_, i) in enumerate(sorted(key)):
            pos[i] = p
        return pos


_SCENES = {}


def get_scene(rtw, oracle, name):
    """The Scene `name`, built once per process (the test modules share it)."""
    if name not in _SCENES:
        _SCENES[name] = Scene(rtw, oracle, name)
    return _SCENES[name]


def winners(ref):
    """List indices of the hits of a record array."""
    return ref["prim"][ref["prim"] > 0].astype(np.int64) - 1
