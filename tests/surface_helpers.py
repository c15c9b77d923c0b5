"""What the surface-query tests share (tests/test_gpu_surface.py, tests/test_surface_cpu.py):
the frames the issue names, each with the oracle's answer computed once on the CPU — rw_hit of
every feature ray, then the material table and rw_texture_value at that record's uv and p — as
numpy arrays of rtw_amd.HIT_DTYPE / SURFACE_DTYPE / GUIDE_DTYPE compared with the device's bit
for bit; and the census that keeps a frame from passing vacuously: how many of its records fall
in each class (material, texture, primitive kind and face, miss) it is there for.

A Case is built once per process and is read-only; nothing here needs a GPU."""
import ctypes as C

import numpy as np

from helpers import MIXED_CAMERA, MIXED_SIZES, _to_desc, mixed_bvh_world
from query_helpers import GEN_SEED, SKY, make_rays, oracle_hits, words

# name -> (scene id or "mixed", width, height)
FRAMES = {"scene1": (1, 48, 32), "scene2": (2, 48, 27), "scene3": (3, 48, 27), "scene4": (4, 48, 27),
          "scene5": (5, 48, 27), "scene6": (6, 40, 40), "scene7": (7, 48, 27), "mixed": ("mixed", 48, 27)}
# the classes a frame is there for: each must hold at least CENSUS_MIN of the oracle's records
CENSUS_MIN = 5
REQUIRED = {"scene1": ("solid", "solid_moving", "checker", "metal", "glass", "miss"),
            "scene2": ("checker",),
            "scene3": ("noise",),
            "scene4": ("image",),
            "scene5": ("light_rect", "noise"),
            # (a camera ray travels towards +z, so it meets every XY rect from behind: no xy_front in this frame)
            "scene6": ("xy_back", "xz_front", "xz_back", "yz_front", "yz_back", "light", "xform"),
            "scene7": ("image", "solid_moving", "metal", "glass", "checker"),
            "mixed": ("solid", "solid_moving", "checker", "image", "metal", "glass", "light", "xy_front", "xz_front",
                      "yz_front", "xform")}
RECT = {2: "xy", 3: "xz", 4: "yz"}


def host_frame_rays(rtw, cam, w, h):
    """The frame's feature rays through the host helper rtw_pixel_ray, row-major -> (w * h,) RAY_DTYPE."""
    rows = []
    for y in range(h):
        for x in range(w):
            r = rtw.pixel_ray(cam, w, h, x, y)
            rows.append((tuple(r.origin), tuple(r.dir), r.time, r.t_min, r.t_max))
    return make_rays(rtw, rows)


def oracle_surface(rtw, oracle, ow, hits, desc):
    """The definition: for each record of hits ((n,) HIT_DTYPE, the oracle's), the material of list entry
    prim - 1 and rw_texture_value at the record's u, v, p -> (n,) SURFACE_DTYPE (a miss: all zero).  Every
    number is the oracle's; `mat` and `tex` index the tables the caller uploaded (`desc`: the oracle's
    builders number their own tables otherwise), whose kinds must be the oracle's."""
    L = oracle._world_lib()
    w = ow.w
    arr3 = C.c_double * 3
    out = np.zeros(len(hits), rtw.SURFACE_DTYPE)
    for i, h in enumerate(hits):
        k = int(h["prim"])
        if k == 0 or k > w.n_prims:
            continue
        m = w.mats[int(w.prims[k - 1].mat)]
        mi = int(desc.prims[k - 1].mat)
        assert desc.mats[mi].kind == m.kind, (k, mi)
        out["kind"][i], out["mat"][i] = m.kind + 1, mi + 1
        if m.kind == oracle.RW_METAL:
            out["value"][i], out["fuzz"][i] = list(m.albedo), m.fuzz
        elif m.kind == oracle.RW_DIELECTRIC:
            out["value"][i], out["ir"][i] = (1.0, 1.0, 1.0), m.ir
        else:
            v = arr3()
            L.rw_texture_value(ow.ptr, m.tex, float(h["u"]), float(h["v"]), arr3(*[float(x) for x in h["p"]]), v)
            ti = int(desc.mats[mi].tex)
            assert desc.textures[ti].kind == w.textures[m.tex].kind, (k, mi, ti)
            out["value"][i], out["tex"][i], out["tex_kind"][i] = list(v), ti + 1, w.textures[m.tex].kind + 1
    return out


def oracle_tex(ow, prim):
    """The oracle's own texture index of the material of list entry prim - 1."""
    return int(ow.w.mats[int(ow.w.prims[int(prim) - 1].mat)].tex)


def texture_value(oracle, ow, tex, u, v, p):
    """rw_texture_value of the oracle's texture `tex` at (u, v, p) -> three floats."""
    out = (C.c_double * 3)()
    oracle._world_lib().rw_texture_value(ow.ptr, tex, float(u), float(v), (C.c_double * 3)(*[float(x) for x in p]), out)
    return list(out)


def guides_of(rtw, hits, surf, background):
    """The guide records the surface records define: {f32(normal), f32(t), f32(value), prim}; a miss
    {0, 0, 0, 0, f32(background), 0}.  (numpy's float64 -> float32 is the C cast: to nearest even.)"""
    g = np.zeros(len(hits), rtw.GUIDE_DTYPE)
    hit = surf["kind"] > 0
    with np.errstate(over="ignore", invalid="ignore"):
        g["normal"][hit] = hits["normal"][hit].astype(np.float32)
        g["depth"][hit] = hits["t"][hit].astype(np.float32)
        g["albedo"][hit] = surf["value"][hit].astype(np.float32)
    g["prim"][hit] = hits["prim"][hit]
    g["albedo"][~hit] = np.array(background, np.float64).astype(np.float32)
    return g


class Case:
    """One frame: the product's description, the oracle's world, the camera, the feature rays and the
    oracle's hit and surface records of them."""

    def __init__(self, rtw, oracle, W, name):
        sid, self.w, self.h = FRAMES[name]
        self.name, self.n = name, self.w * self.h
        if sid == "mixed":
            self.tables = mixed_bvh_world(W, W.earth_map(), *MIXED_SIZES["small"], GEN_SEED)
            self.desc, self._keep = _to_desc(W, *self.tables)
            self.oracle = oracle.TableWorld(*self.tables, background=SKY)
            m = MIXED_CAMERA
            self.cam = rtw.camera_init(m["look_from"], m["look_at"], (0, 1, 0), m["vfov"], self.w / self.h,
                                       m["aperture"], m["focus"], 0.0, 1.0)
            self.background = SKY
        else:
            img = W.earth_map() if sid in (4, 7) else None
            self.built = W.BuiltScene(sid, 42, img)
            self.desc = self.built.desc
            self.oracle = oracle.OracleWorld(sid, 42, img)
            self.cam = self.built.camera(self.w / self.h)
            self.background = tuple(self.built.background)
        self.rays = host_frame_rays(rtw, self.cam, self.w, self.h)
        self.ref_hits = oracle_hits(rtw, self.oracle, self.rays)
        self.ref_surf = oracle_surface(rtw, oracle, self.oracle, self.ref_hits, self.desc)
        for a in (self.rays, self.ref_hits, self.ref_surf):
            a.setflags(write=False)


_CASES = {}


def get_case(rtw, oracle, W, name):
    if name not in _CASES:
        _CASES[name] = Case(rtw, oracle, W, name)
    return _CASES[name]


def census(oracle, W, desc, hits, surf):
    """Records per class, from the oracle's records and the description alone."""
    c = {}

    def add(k, mask):
        c[k] = c.get(k, 0) + int(np.count_nonzero(mask))
    hit = hits["prim"] > 0
    add("miss", ~hit)
    idx = hits["prim"].astype(np.int64) - 1
    kind = np.array([desc.prims[int(i)].kind if i >= 0 else -1 for i in idx])
    xform = np.array([desc.prims[int(i)].xform if i >= 0 else -1 for i in idx])
    lam, light = surf["kind"] == oracle.RW_LAMBERT + 1, surf["kind"] == oracle.RW_LIGHT + 1
    solid = surf["tex_kind"] == oracle.RW_TEX_SOLID + 1
    add("solid", lam & solid & (kind == W.PRIM_SPHERE))
    add("solid_moving", lam & solid & (kind == W.PRIM_MOVING_SPHERE))
    add("checker", surf["tex_kind"] == oracle.RW_TEX_CHECKER + 1)
    add("noise", surf["tex_kind"] == oracle.RW_TEX_NOISE + 1)
    add("image", surf["tex_kind"] == oracle.RW_TEX_IMAGE + 1)
    add("metal", surf["kind"] == oracle.RW_METAL + 1)
    add("glass", surf["kind"] == oracle.RW_DIELECTRIC + 1)
    add("light", light)
    add("light_rect", light & (kind >= W.PRIM_XY_RECT))
    add("xform", hit & (xform >= 0))
    add("inside", hit & (hits["front"] == 0) & (kind <= W.PRIM_MOVING_SPHERE))
    add("back", hit & (hits["front"] == 0))
    for k, nm in RECT.items():
        add(nm + "_front", (kind == k) & (hits["front"] == 1))
        add(nm + "_back", (kind == k) & (hits["front"] == 0))
    return c


def check_census(oracle, W, case, hits=None, surf=None, required=None):
    c = census(oracle, W, case.desc, case.ref_hits if hits is None else hits, case.ref_surf if surf is None else surf)
    need = REQUIRED[case.name] if required is None else required
    short = {k: c.get(k, 0) for k in need if c.get(k, 0) < CENSUS_MIN}
    assert not short, (case.name, "classes with fewer than %d records" % CENSUS_MIN, short, c)
    return c


def bounce_rays(rtw, rays, hits):
    """From every hit of (rays, hits): the ray reflected about the record's normal and the ray continued
    straight on (into a sphere it met from outside: the next hit is from inside), both from p at the
    ray's time.  The CPU's statement of the bounce the GPU test builds in torch (that test hands the
    oracle the device's own ray bytes, so the two need not agree to the bit)."""
    hit = hits["prim"] > 0
    d, n, p = rays["dir"][hit], hits["normal"][hit], hits["p"][hit]
    dn = (d[:, 0] * n[:, 0] + d[:, 1] * n[:, 1]) + d[:, 2] * n[:, 2]
    refl = d - (2.0 * dn)[:, None] * n
    out = np.zeros(2 * len(d), rtw.RAY_DTYPE)
    out["origin"] = np.concatenate([p, p])
    out["dir"] = np.concatenate([refl, d])
    out["time"] = np.concatenate([rays["time"][hit]] * 2)
    out["t_min"], out["t_max"] = 0.001, np.inf
    return out


__all__ = ["FRAMES", "REQUIRED", "Case", "get_case", "census", "check_census", "oracle_surface", "oracle_tex", "texture_value",
           "guides_of", "host_frame_rays", "bounce_rays", "words"]
