"""General worlds through the C ABI (include/rtw_hip.h "general worlds"):
every scene of the reference's main.zig (1 cover, 2 two spheres, 3 two Perlin
spheres, 4 earth, 5 simple light, 6 Cornell box) and BASELINE.json
configs[4] (7: globe + 10k random spheres), rendered by the world kernel
(csrc/rtw_world.hip).  Plain ctypes marshalling; no CPU fallback.

Reference correspondence:
  build_scene     -> generate* scene builders   src/main.zig:123-290 (+ DefaultPrng, :300)
  scene_camera    -> Camera.init with the scene's settings  main.zig:316-376
  load_png        -> Image.fromFilePath (zigimg) of texture.zig:111 (RGBA8, non-interlaced PNG)
  DeviceWorld     -> the world upload + the render loop     main.zig:378-402
"""
from __future__ import annotations

import ctypes as C
import os
import struct
import zlib

import numpy as np

from . import (HIT_DTYPE, RAY_DTYPE, RTW_EINVAL, SURFACE_DTYPE, Camera, Params, QueryOpts, RtwError, Timer, _check,
               _surface, camera_init, lib)

PRIM_SPHERE, PRIM_MOVING_SPHERE, PRIM_XY_RECT, PRIM_XZ_RECT, PRIM_YZ_RECT = 0, 1, 2, 3, 4
PRIM_TRIANGLE = 5  # rtw_hip.h RTW_PRIM_TRIANGLE: a = v0[3], v1[3], v2[3] (not in the reference; csrc/rtw_tri.hpp)
XF_TRANSLATE, XF_ROTATE_Y = 0, 1
TEX_SOLID, TEX_CHECKER, TEX_NOISE, TEX_IMAGE = 0, 1, 2, 3
WMAT_LAMBERT, WMAT_METAL, WMAT_DIELECTRIC, WMAT_LIGHT = 0, 1, 2, 3
WORLD_LINEAR = 1
WORLD_DYNAMIC = 4  # rtw_hip.h RTW_WORLD_DYNAMIC: the world takes updates (update / update_device)
WORLD_DEBUG_BVH = 2  # rtw_hip.h RTW_WORLD_DEBUG_BVH: the BVH root's children to stderr (diagnostic)
SCENES = {1: "cover", 2: "two_spheres", 3: "two_perlin_spheres", 4: "earth", 5: "simple_light",
          6: "cornell_box", 7: "globe_10k"}


class Prim(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("mat", C.c_uint32), ("xform", C.c_int32), ("reserved", C.c_uint32),
                ("a", C.c_double * 9)]


class Xform(C.Structure):
    _fields_ = [("n", C.c_uint32), ("op", C.c_uint32 * 4), ("v", (C.c_double * 3) * 4)]


class Texture(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("perlin", C.c_uint32), ("image", C.c_uint32), ("reserved", C.c_uint32),
                ("color", C.c_double * 3), ("odd", C.c_double * 3), ("even", C.c_double * 3),
                ("scale", C.c_double)]


class WMaterial(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("tex", C.c_uint32), ("albedo", C.c_double * 3), ("fuzz", C.c_double),
                ("ir", C.c_double)]


class Perlin(C.Structure):
    _fields_ = [("ranvec", (C.c_double * 3) * 256), ("perm", (C.c_uint32 * 256) * 3)]


class Image(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("rgba", C.c_void_p)]


class WorldDesc(C.Structure):
    _fields_ = [("prims", C.POINTER(Prim)), ("n_prims", C.c_uint32),
                ("xforms", C.POINTER(Xform)), ("n_xforms", C.c_uint32),
                ("textures", C.POINTER(Texture)), ("n_textures", C.c_uint32),
                ("mats", C.POINTER(WMaterial)), ("n_mats", C.c_uint32),
                ("perlins", C.POINTER(Perlin)), ("n_perlins", C.c_uint32),
                ("images", C.POINTER(Image)), ("n_images", C.c_uint32)]


class SceneSettings(C.Structure):
    _fields_ = [("look_from", C.c_double * 3), ("look_at", C.c_double * 3), ("vfov", C.c_double),
                ("aperture", C.c_double), ("aspect", C.c_double), ("background", C.c_double * 3),
                ("width", C.c_uint32), ("height", C.c_uint32), ("spp", C.c_uint32), ("reserved", C.c_uint32)]


def _wlib():
    L = lib()
    if getattr(L, "_world_ready", False):
        return L
    P = C.POINTER
    L.rtw_build_scene.argtypes = [C.c_uint32, C.c_uint64, P(Image), P(C.c_void_p)]
    L.rtw_built_scene_desc.argtypes = [C.c_void_p, P(WorldDesc), P(SceneSettings), C.c_uint64 * 4]
    L.rtw_built_scene_free.argtypes = [C.c_void_p]
    L.rtw_world_create.argtypes = [P(WorldDesc), C.c_uint32, P(C.c_void_p)]
    L.rtw_world_destroy.argtypes = [C.c_void_p]
    L.rtw_world_bvh_info.argtypes = [C.c_void_p, C.c_uint32 * 4]
    L.rtw_world_workspace_bytes.restype = C.c_size_t
    L.rtw_world_workspace_bytes.argtypes = [C.c_void_p, P(Params)]
    L.rtw_world_render_device.argtypes = [C.c_void_p, P(Camera), P(Params), C.c_void_p, C.c_size_t, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p]
    L.rtw_world_render.argtypes = [P(Camera), P(WorldDesc), P(Params), C.c_void_p, C.c_void_p]
    L.rtw_world_render_counts.argtypes = [C.c_void_p, P(Camera), P(Params), C.c_void_p, C.c_size_t,
                                          C.c_uint64 * 4]
    L.rtw_world_render_counts_ex.argtypes = [C.c_void_p, P(Camera), P(Params), C.c_void_p, C.c_size_t,
                                             C.c_uint64 * 8]
    if hasattr(L, "rtw_world_launch_info"):  # (A/B timing may load an older build without it)
        L.rtw_world_launch_info.argtypes = [C.c_void_p, P(Params), C.c_uint32 * 6]
    if hasattr(L, "rtw_world_trace_tri_host"):
        L.rtw_world_trace_tri_host.argtypes = [P(WorldDesc), C.c_void_p, C.c_size_t, P(QueryOpts), C.c_void_p]
    L._world_ready = True
    return L


# ------------------------------------------------------------ images ----
def load_png(path: str) -> np.ndarray:
    """Decode an 8-bit, non-interlaced PNG to (H, W, 4) uint8 RGBA (grey,
    grey+alpha, RGB, palette are expanded; RGBA is taken as is, which is the
    only layout texture.zig:133-140's 4-byte stride reads correctly)."""
    data = open(path, "rb").read()
    if data[:8] != b"\x89PNG\r\n\x1a\n":
        raise ValueError(f"{path}: not a PNG")
    i, idat, plte, trns, hdr = 8, [], None, None, None
    while i < len(data):
        n = struct.unpack(">I", data[i:i + 4])[0]
        typ, body = data[i + 4:i + 8], data[i + 8:i + 8 + n]
        if typ == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", body)
        elif typ == b"PLTE":
            plte = np.frombuffer(body, np.uint8).reshape(-1, 3)
        elif typ == b"tRNS":
            trns = np.frombuffer(body, np.uint8)
        elif typ == b"IDAT":
            idat.append(body)
        elif typ == b"IEND":
            break
        i += 12 + n
    w, h, depth, ctype, _, _, interlace = hdr
    if depth != 8 or interlace != 0:
        raise ValueError(f"{path}: only 8-bit non-interlaced PNGs are supported")
    ch = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}[ctype]
    raw = np.frombuffer(zlib.decompress(b"".join(idat)), np.uint8)
    stride = w * ch
    out = np.zeros((h, stride), np.int32)
    prev = np.zeros(stride, np.int32)
    for y in range(h):
        f = raw[y * (stride + 1)]
        line = raw[y * (stride + 1) + 1:(y + 1) * (stride + 1)].astype(np.int32)
        if f == 0:
            cur = line
        elif f == 2:
            cur = (line + prev) & 255
        else:  # Sub / Average / Paeth need the running left neighbour
            cur = np.zeros(stride, np.int32)
            for x in range(stride):
                a = cur[x - ch] if x >= ch else 0
                b = prev[x]
                c = prev[x - ch] if x >= ch else 0
                if f == 1:
                    pred = a
                elif f == 3:
                    pred = (a + b) >> 1
                else:
                    p = a + b - c
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    pred = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
                cur[x] = (line[x] + pred) & 255
        out[y] = cur
        prev = cur
    px = out.astype(np.uint8).reshape(h, w, ch)
    if ctype == 6:
        return np.ascontiguousarray(px)
    rgba = np.full((h, w, 4), 255, np.uint8)
    if ctype == 2:
        rgba[..., :3] = px
    elif ctype == 0:
        rgba[..., :3] = px[..., :1]
    elif ctype == 4:
        rgba[..., :3] = px[..., :1]
        rgba[..., 3] = px[..., 1]
    else:
        rgba[..., :3] = plte[px[..., 0]]
        if trns is not None:
            a = np.full(len(plte), 255, np.uint8)
            a[:len(trns)] = trns
            rgba[..., 3] = a[px[..., 0]]
    return rgba


EARTH_PNG = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))),
                         "assets", "sekaichizu.png")


def earth_map(path: str | None = None) -> np.ndarray:
    """The reference's globe texture (assets/sekaichizu.png, 500 x 282 RGBA8,
    ocean = alpha 0; loaded by ImageTexture.init, texture.zig:107-119, for
    main.zig:226 and BASELINE configs[4]).  The repo carries the reference's
    asset file unchanged, with the reference's own note (assets/LICENSE), so
    the GPU box renders the real texture; RTW_EARTH_MAP names another PNG.
    Decoded by the library's PNG reader."""
    return load_png(path or os.environ.get("RTW_EARTH_MAP") or EARTH_PNG)


def synthetic_world_map(width: int = 500, height: int = 282) -> np.ndarray:
    """A deterministic map of the globe asset's size and format (500 x 282
    RGBA8, ocean = alpha 0): smooth 'continents' from a few sinusoids.  Used
    only by tests that want a texture independent of the asset file."""
    y, x = np.mgrid[0:height, 0:width].astype(np.float64)
    u, v = x / width * 2 * np.pi, y / height * np.pi
    f = np.sin(3 * u) * np.sin(2 * v) + 0.6 * np.sin(5 * u + 1.3) * np.cos(3 * v) + 0.4 * np.cos(7 * u - 2 * v)
    land = f > 0.35
    img = np.zeros((height, width, 4), np.uint8)
    img[..., 0] = np.clip(80 + 120 * np.sin(u + v) ** 2, 0, 255).astype(np.uint8)
    img[..., 1] = np.clip(150 + 80 * np.cos(2 * u) * np.sin(v), 0, 255).astype(np.uint8)
    img[..., 2] = np.clip(60 + 40 * np.sin(3 * v), 0, 255).astype(np.uint8)
    img[..., 3] = np.where(land, 255, 0).astype(np.uint8)
    return img


# ------------------------------------------------------------ scenes ----
class BuiltScene:
    """A scene built by the library's builders (rtw_build_scene): desc points
    into library-owned arrays until close()."""

    def __init__(self, scene_id: int, seed: int = 42, image: np.ndarray | None = None):
        L = _wlib()
        self._img = None
        img = None
        if image is not None:
            self._img = np.ascontiguousarray(image, np.uint8)
            img = Image(self._img.shape[1], self._img.shape[0], self._img.ctypes.data)
        self.h = C.c_void_p()
        _check(L.rtw_build_scene(scene_id, seed, C.byref(img) if img is not None else None, C.byref(self.h)))
        self.desc = WorldDesc()
        self.settings = SceneSettings()
        st = (C.c_uint64 * 4)()
        _check(L.rtw_built_scene_desc(self.h, C.byref(self.desc), C.byref(self.settings), st))
        self.rng_state = [int(x) for x in st]
        self.scene_id = scene_id

    def camera(self, aspect: float | None = None) -> Camera:
        s = self.settings
        return camera_init(tuple(s.look_from), tuple(s.look_at), (0, 1, 0), s.vfov,
                           aspect if aspect is not None else s.aspect, s.aperture, 10.0, 0.0, 1.0)

    @property
    def background(self):
        return tuple(self.settings.background)

    def table(self) -> dict:
        """Resolved plain-python dump (materials with their texture values
        inlined), comparable with oracle.OracleWorld.table()."""
        d = self.desc
        prims = [{"kind": p.kind, "mat": p.mat, "xform": p.xform, "a": list(p.a)}
                 for p in (d.prims[i] for i in range(d.n_prims))]
        xfs = [{"n": x.n, "op": list(x.op)[:x.n], "v": [list(x.v[k]) for k in range(x.n)]}
               for x in (d.xforms[i] for i in range(d.n_xforms))]
        texs = [{"kind": t.kind, "perlin": t.perlin, "image": t.image, "color": list(t.color), "odd": list(t.odd),
                 "even": list(t.even), "scale": t.scale} for t in (d.textures[i] for i in range(d.n_textures))]
        mats = [{"kind": m.kind, "tex": m.tex, "albedo": list(m.albedo), "fuzz": m.fuzz, "ir": m.ir}
                for m in (d.mats[i] for i in range(d.n_mats))]
        perl = [{"ranvec": [list(p.ranvec[k]) for k in range(256)], "perm": [list(p.perm[a]) for a in range(3)]}
                for p in (d.perlins[i] for i in range(d.n_perlins))]
        return {"prims": prims, "xforms": xfs, "textures": texs, "materials": mats, "perlins": perl}

    def close(self):
        if self.h:
            _wlib().rtw_built_scene_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def render_world(cam: Camera, desc: WorldDesc, params: Params, want_mean=False):
    """Synchronous host-buffer render of a world (rtw_world_render)."""
    rgb = np.zeros((params.row_count, params.width, 3), np.uint8)
    mean = np.zeros((params.row_count, params.width, 3), np.float32) if want_mean else None
    _check(_wlib().rtw_world_render(C.byref(cam), C.byref(desc), C.byref(params), rgb.ctypes.data,
                                    mean.ctypes.data if want_mean else None))
    return (rgb, mean) if want_mean else rgb


def refit_tables_host(desc: WorldDesc, flags: int, table_bytes: int, a=None, xv=None) -> dict:
    """rtw_world_refit_tables_host: what the tables of `desc` created with `flags` hold after an
    update with a ((n_prims, 9) float64) and xv ((n_xforms, 4, 3) float64 or None), computed on
    the host alone; a=None: as created.  table_bytes: DeviceWorld.table_bytes() of such a world.
    Same keys as DeviceWorld.read_tables()."""
    L = _wlib()
    cull, bounds = (C.c_float * 2)(), (C.c_double * 6)()
    a = None if a is None else np.ascontiguousarray(a, np.float64)
    xv = None if xv is None else np.ascontiguousarray(xv, np.float64)
    if a is not None and a.shape != (desc.n_prims, 9):
        raise ValueError(f"a must be ({desc.n_prims}, 9)")
    if xv is not None and xv.shape != (desc.n_xforms, 4, 3):
        raise ValueError(f"xv must be ({desc.n_xforms}, 4, 3)")
    blob = np.zeros(table_bytes, np.uint8)
    _check(L.rtw_world_refit_tables_host(C.byref(desc), flags, a.ctypes.data if a is not None else None,
                                         xv.ctypes.data if xv is not None else None, blob.ctypes.data, table_bytes,
                                         cull, bounds))
    return {"blob": blob, "cull": np.array(cull[:], np.float32), "bounds": np.array(bounds[:], np.float64)}


def rebuild_tables_host(desc: WorldDesc, flags: int, table_bytes: int, a, xv=None, then_a=None, then_xv=None) -> dict:
    """rtw_world_rebuild_tables_host: what the tables of `desc` created with `flags` hold after a
    rebuild with a / xv, computed on the host alone; then_a / then_xv: followed by an update with
    these (rtw_world_rebuild_refit_tables_host).  The keys of refit_tables_host, and "info": the
    four numbers of rtw_world_bvh_info."""
    L = _wlib()
    cull, bounds, info = (C.c_float * 2)(), (C.c_double * 6)(), (C.c_uint32 * 4)()

    def arr(x, shape, what):
        if x is None:
            return None
        x = np.ascontiguousarray(x, np.float64)
        if x.shape != shape:
            raise ValueError(f"{what} must be {shape}")
        return x
    a, then_a = arr(a, (desc.n_prims, 9), "a"), arr(then_a, (desc.n_prims, 9), "then_a")
    xv, then_xv = arr(xv, (desc.n_xforms, 4, 3), "xv"), arr(then_xv, (desc.n_xforms, 4, 3), "then_xv")
    if a is None:
        raise ValueError("a is required")

    def ptr(x):
        return x.ctypes.data if x is not None and x.size else None
    blob = np.zeros(table_bytes, np.uint8)
    if then_a is None:
        _check(L.rtw_world_rebuild_tables_host(C.byref(desc), flags, ptr(a), ptr(xv), blob.ctypes.data, table_bytes,
                                               cull, bounds, info))
    else:
        _check(L.rtw_world_rebuild_refit_tables_host(C.byref(desc), flags, ptr(a), ptr(xv), ptr(then_a), ptr(then_xv),
                                                     blob.ctypes.data, table_bytes, cull, bounds, info))
    return {"blob": blob, "cull": np.array(cull[:], np.float32), "bounds": np.array(bounds[:], np.float64),
            "info": {"nodes": info[0], "leaves": info[1], "max_depth": info[2], "max_leaf": info[3]}}


def desc_numbers(desc: WorldDesc):
    """The numbers an update replaces, out of a descriptor: a (n_prims, 9) and xv (n_xforms, 4, 3)."""
    a = np.array([list(desc.prims[i].a) for i in range(desc.n_prims)], np.float64).reshape(desc.n_prims, 9)
    xv = np.array([[list(desc.xforms[i].v[k]) for k in range(4)] for i in range(desc.n_xforms)],
                  np.float64).reshape(desc.n_xforms, 4, 3)
    return a, xv


def prev_points_host(desc: WorldDesc, hits, time: float, a_prev=None, xv_prev=None) -> np.ndarray:
    """rtw_world_prev_points_host (no GPU): hits (n,) HIT_DTYPE of the world `desc` describes -> (n, 3)
    float64, each hit's surface point under the numbers a_prev ((n_prims, 9)) / xv_prev ((n_xforms, 4, 3)),
    None = the descriptor's own."""
    h = np.ascontiguousarray(hits, HIT_DTYPE).reshape(-1)
    a = np.ascontiguousarray(a_prev, np.float64) if a_prev is not None else None
    xv = np.ascontiguousarray(xv_prev, np.float64) if xv_prev is not None else None
    if (a is not None and a.shape != (desc.n_prims, 9)) or (xv is not None and xv.shape != (desc.n_xforms, 4, 3)):
        raise ValueError("a_prev must be (n_prims, 9) and xv_prev (n_xforms, 4, 3)")
    out = np.zeros((h.size, 3), np.float64)
    _check(_wlib().rtw_world_prev_points_host(C.byref(desc), h.ctypes.data, h.size, float(time),
                                              a.ctypes.data if a is not None else None,
                                              xv.ctypes.data if xv is not None and xv.size else None, out.ctypes.data))
    return out


def mirror_rays_host(desc: WorldDesc, rays, hits):
    """rtw_world_mirror_rays_host (no GPU): rays (n,) RAY_DTYPE and their hits (n,) HIT_DTYPE of the world `desc`
    describes -> (rays2 (n,) RAY_DTYPE, is_mirror (n,) uint8): the reflected ray of every record that counts as a
    mirror (a front hit of a metal primitive), zero bytes for the others."""
    r = np.ascontiguousarray(rays, RAY_DTYPE).reshape(-1)
    h = np.ascontiguousarray(hits, HIT_DTYPE).reshape(-1)
    if r.size != h.size:
        raise ValueError("rays and hits must have the same length")
    r2, m = np.zeros(r.size, RAY_DTYPE), np.zeros(r.size, np.uint8)
    _check(_wlib().rtw_world_mirror_rays_host(C.byref(desc), r.ctypes.data, h.ctypes.data, r.size, r2.ctypes.data,
                                              m.ctypes.data))
    return r2, m


def mirror_points_host(desc: WorldDesc, rays, hits, hits2, cam_prev, a_prev=None, xv_prev=None, opts=None) -> np.ndarray:
    """rtw_world_mirror_points_host (no GPU): prev_points_host's result with each ray's own time, except that a
    mirror record gets the point of the mirror that showed the same reflected thing from cam_prev under the
    previous numbers; hits2 (n,) HIT_DTYPE are the hits of mirror_rays_host's rays.  -> (n, 3) float64."""
    r = np.ascontiguousarray(rays, RAY_DTYPE).reshape(-1)
    h = np.ascontiguousarray(hits, HIT_DTYPE).reshape(-1)
    h2 = np.ascontiguousarray(hits2, HIT_DTYPE).reshape(-1)
    if r.size != h.size or h2.size != h.size:
        raise ValueError("rays, hits and hits2 must have the same length")
    a = np.ascontiguousarray(a_prev, np.float64) if a_prev is not None else None
    xv = np.ascontiguousarray(xv_prev, np.float64) if xv_prev is not None else None
    if (a is not None and a.shape != (desc.n_prims, 9)) or (xv is not None and xv.shape != (desc.n_xforms, 4, 3)):
        raise ValueError("a_prev must be (n_prims, 9) and xv_prev (n_xforms, 4, 3)")
    out = np.zeros((h.size, 3), np.float64)
    _check(_wlib().rtw_world_mirror_points_host(C.byref(desc), r.ctypes.data, h.ctypes.data, h2.ctypes.data, h.size,
                                                C.byref(cam_prev), a.ctypes.data if a is not None else None,
                                                xv.ctypes.data if xv is not None and xv.size else None,
                                                C.byref(opts) if opts is not None else None, out.ctypes.data))
    return out


def mesh_prims(vertices, faces, mat: int, xform: int = -1) -> list:
    """The triangles of an indexed mesh as a list of Prim (PRIM_TRIANGLE): vertices (n, 3) float, faces (m, 3) int
    indices into them (the winding gives the normal: (v1 - v0) x (v2 - v0)), one material and transform chain for
    all.  Shared vertices keep their bits, which is what makes a closed mesh watertight (csrc/rtw_tri.hpp)."""
    v = np.ascontiguousarray(vertices, np.float64)
    f = np.ascontiguousarray(faces, np.int64)
    if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3:
        raise ValueError("vertices must be (n, 3) and faces (m, 3)")
    if f.size and (f.min() < 0 or f.max() >= len(v)):
        raise ValueError("a face index is out of range")
    out = []
    for tri in v[f].reshape(-1, 9):
        p = Prim()
        p.kind, p.mat, p.xform = PRIM_TRIANGLE, int(mat), int(xform)
        for k in range(9):
            p.a[k] = float(tri[k])
        out.append(p)
    return out


def load_obj(path: str):
    """A Wavefront OBJ's geometry: (vertices (n, 3) float64, faces (m, 3) int64).  `v` and `f` lines only (every
    other line is skipped); a polygon is fanned from its first vertex; an index may be negative (relative to the
    vertices read so far) and may carry /vt/vn parts, which are ignored."""
    verts, faces = [], []
    with open(path) as fh:
        for ln, line in enumerate(fh, 1):
            t = line.split("#", 1)[0].split()
            if not t:
                continue
            if t[0] == "v":
                if len(t) < 4:
                    raise ValueError(f"{path}:{ln}: a vertex needs three coordinates")
                verts.append([float(t[1]), float(t[2]), float(t[3])])
            elif t[0] == "f":
                idx = []
                for w in t[1:]:
                    i = int(w.split("/")[0])
                    i = i - 1 if i > 0 else len(verts) + i
                    if i < 0 or i >= len(verts) or int(w.split("/")[0]) == 0:
                        raise ValueError(f"{path}:{ln}: vertex index {w} out of range")
                    idx.append(i)
                if len(idx) < 3:
                    raise ValueError(f"{path}:{ln}: a face needs three vertices")
                for k in range(1, len(idx) - 1):
                    faces.append([idx[0], idx[k], idx[k + 1]])
    return np.array(verts, np.float64).reshape(-1, 3), np.array(faces, np.int64).reshape(-1, 3)


def trace_tri_host(desc: WorldDesc, rays, opts: QueryOpts | None = None) -> np.ndarray:
    """rtw_world_trace_tri_host (no GPU): rays (n,) RAY_DTYPE -> (n,) HIT_DTYPE, the closest hit of each ray over
    the TRIANGLES of `desc` only (the reference's sequential loop through csrc/rtw_tri.hpp); a miss is all zero."""
    r = np.ascontiguousarray(rays, RAY_DTYPE).reshape(-1)
    out = np.zeros(r.size, HIT_DTYPE)
    _check(_wlib().rtw_world_trace_tri_host(C.byref(desc), r.ctypes.data, r.size,
                                            C.byref(opts) if opts is not None else None, out.ctypes.data))
    return out


TRAVERSAL_NAMES = {1: "union", 2: "lane", 3: "linear"}  # rtw_world_traversal (rtw_hip.h)


class DeviceWorld:
    """A world resident in HBM of the current device (rtw_world_create)."""

    def __init__(self, desc: WorldDesc, linear: bool = False, debug_bvh: bool = False, dynamic: bool = False):
        self.h = C.c_void_p()
        flags = ((WORLD_LINEAR if linear else 0) | (WORLD_DEBUG_BVH if debug_bvh else 0) |
                 (WORLD_DYNAMIC if dynamic else 0))
        self.flags, self.n_prims, self.n_xforms = flags, int(desc.n_prims), int(desc.n_xforms)
        _check(_wlib().rtw_world_create(C.byref(desc), flags, C.byref(self.h)))

    def update(self, prims, xforms=None):
        """rtw_world_update: new numbers from HOST arrays shaped like the descriptor's — a
        WorldDesc (its prims and xforms are taken), or ctypes arrays of Prim and Xform (all of
        them, in list order); kinds, materials, transform indices and op lists must equal the
        world's.  The world must have been created with dynamic=True."""
        if isinstance(prims, WorldDesc):
            pp, n, xp, nx = prims.prims, prims.n_prims, prims.xforms, prims.n_xforms
        else:
            pp, n = prims, (len(prims) if prims is not None else 0)
            xp, nx = xforms, (len(xforms) if xforms is not None else 0)
        _check(_wlib().rtw_world_update(self.h, C.cast(pp, C.c_void_p) if n else None, n,
                                        C.cast(xp, C.c_void_p) if nx else None, nx))

    def update_device(self, a_ptr: int, xv_ptr: int | None = None, stream: int | None = None):
        """rtw_world_update_device: a_ptr = n_prims x 9 float64 in device memory (list order),
        xv_ptr = n_xforms x 4 x 3 float64 or None (the transforms keep their values).  Waits for
        the validation's readback, then enqueues the commit on `stream` and returns."""
        _check(_wlib().rtw_world_update_device(self.h, C.c_void_p(a_ptr) if a_ptr else None,
                                               C.c_void_p(xv_ptr) if xv_ptr else None,
                                               C.c_void_p(stream) if stream else None))

    def rebuild(self, prims, xforms=None):
        """rtw_world_rebuild: the arguments of update(); the world takes the numbers and gets a
        new tree built from them on the device (dynamic worlds whose BVH has leaves of one
        primitive: >= 512 primitives; others raise RTW_UNSUPPORTED)."""
        if isinstance(prims, WorldDesc):
            pp, n, xp, nx = prims.prims, prims.n_prims, prims.xforms, prims.n_xforms
        else:
            pp, n = prims, (len(prims) if prims is not None else 0)
            xp, nx = xforms, (len(xforms) if xforms is not None else 0)
        _check(_wlib().rtw_world_rebuild(self.h, C.cast(pp, C.c_void_p) if n else None, n,
                                         C.cast(xp, C.c_void_p) if nx else None, nx))

    def rebuild_device(self, a_ptr: int, xv_ptr: int | None = None, stream: int | None = None):
        """rtw_world_rebuild_device: the arguments of update_device().  Waits for one readback
        (validation, the new depth and the nodes per level), then enqueues the commit."""
        _check(_wlib().rtw_world_rebuild_device(self.h, C.c_void_p(a_ptr) if a_ptr else None,
                                                C.c_void_p(xv_ptr) if xv_ptr else None,
                                                C.c_void_p(stream) if stream else None))

    def bvh_cost(self, stream: int | None = None) -> float:
        """rtw_world_bvh_cost: sum over nodes of the two child boxes' half-areas over the root
        box's, from the node table as stored; waits for its 8-byte readback."""
        out = C.c_double(0.0)
        _check(_wlib().rtw_world_bvh_cost(self.h, C.c_void_p(stream) if stream else None, C.byref(out)))
        return float(out.value)

    def table_bytes(self) -> int:
        return int(_wlib().rtw_world_table_bytes(self.h))

    def read_tables(self) -> dict:
        """rtw_world_read_tables (diagnostic, synchronous): the device tables as bytes, the
        pretest's host scalars and the world box."""
        n = self.table_bytes()
        blob = np.zeros(n, np.uint8)
        cull, bounds = (C.c_float * 2)(), (C.c_double * 6)()
        _check(_wlib().rtw_world_read_tables(self.h, blob.ctypes.data, n, cull, bounds))
        return {"blob": blob, "cull": np.array(cull[:], np.float32), "bounds": np.array(bounds[:], np.float64)}

    def bvh_info(self) -> dict:
        info = (C.c_uint32 * 4)()
        _check(_wlib().rtw_world_bvh_info(self.h, info))
        return {"nodes": info[0], "leaves": info[1], "max_depth": info[2], "max_leaf": info[3]}

    def workspace_bytes(self, params: Params) -> int:
        """Device workspace of a render of this world (rtw_world_workspace_bytes:
        the common region + the tail dealing's per-lane rings)."""
        n = _wlib().rtw_world_workspace_bytes(self.h, C.byref(params))
        if n == 0:
            raise RtwError(RTW_EINVAL, lib().rtw_last_error().decode())
        return n

    def render_async(self, cam: Camera, params: Params, workspace_ptr: int, workspace_bytes_: int, rgb_ptr: int,
                     mean_ptr: int | None = None, stream: int | None = None, timer: Timer | None = None):
        _check(_wlib().rtw_world_render_device(self.h, C.byref(cam), C.byref(params), C.c_void_p(workspace_ptr),
                                               workspace_bytes_, C.c_void_p(rgb_ptr),
                                               C.c_void_p(mean_ptr) if mean_ptr else None,
                                               C.c_void_p(stream) if stream else None,
                                               timer.h if timer is not None else None))

    def guides(self, cam: Camera, params: Params, guides_ptr: int, stream: int | None = None):
        """The world's feature buffers (rtw_world_guides_device): row_count x W rtw_guide
        records (32 bytes each) into device memory, asynchronous on `stream`."""
        _check(_wlib().rtw_world_guides_device(self.h, C.byref(cam), C.byref(params), C.c_void_p(guides_ptr),
                                               C.c_void_p(stream) if stream else None))

    def launch_info(self, params: Params) -> dict:
        """rtw_world_launch_info: how a render with these params launches on the
        current device — the traversal that runs (after AUTO and the world's
        limits), kernel feature set, register budget, workgroups per CU, grid, LDS."""
        out = (C.c_uint32 * 6)()
        _check(_wlib().rtw_world_launch_info(self.h, C.byref(params), out))
        return {"traversal": TRAVERSAL_NAMES.get(int(out[0]), str(out[0])), "feature_set": int(out[1]),
                "waves": int(out[2]), "blocks_per_cu": int(out[3]), "grid": int(out[4]), "lds_bytes": int(out[5])}

    def trace(self, rays_ptr: int, n: int, hits_ptr: int, opts: QueryOpts | None = None, stream: int | None = None):
        """Closest hits of n rtw_ray records in device memory into n rtw_hit records
        (rtw_world_trace_device), asynchronous on `stream`; prim = list index + 1, a miss all zero."""
        _check(_wlib().rtw_world_trace_device(self.h, C.c_void_p(rays_ptr), n,
                                              C.byref(opts) if opts is not None else None, C.c_void_p(hits_ptr),
                                              C.c_void_p(stream) if stream else None))

    def occluded(self, rays_ptr: int, n: int, out_ptr: int, opts: QueryOpts | None = None,
                 stream: int | None = None):
        """One byte per ray, 1 where trace() would hit (rtw_world_occluded_device)."""
        _check(_wlib().rtw_world_occluded_device(self.h, C.c_void_p(rays_ptr), n,
                                                 C.byref(opts) if opts is not None else None, C.c_void_p(out_ptr),
                                                 C.c_void_p(stream) if stream else None))

    def trace_host(self, rays, opts: QueryOpts | None = None) -> np.ndarray:
        """rtw_world_trace: rays (n,) RAY_DTYPE on the host -> hits (n,) HIT_DTYPE, synchronous."""
        r = np.ascontiguousarray(rays, RAY_DTYPE)
        out = np.zeros(r.shape, HIT_DTYPE)
        _check(_wlib().rtw_world_trace(self.h, r.ctypes.data, r.size, C.byref(opts) if opts is not None else None,
                                       out.ctypes.data))
        return out

    def surface(self, hits_ptr: int, n: int, surf_ptr: int | None = None, guides_ptr: int | None = None,
                background=None, stream: int | None = None):
        """rtw_world_surface_device: for n rtw_hit records of this world in device memory (trace()'s), what
        each hit surface is — n rtw_surface records (SURFACE_DTYPE, 64 bytes: the material's kind and index,
        its texture's value at the hit, fuzz, ir) into surf_ptr and / or the n rtw_guide records of those rays
        into guides_ptr, at least one; asynchronous on `stream`.  `background` (three numbers, a miss's
        albedo) is needed with guides_ptr."""
        _surface(_wlib().rtw_world_surface_device, self.h, hits_ptr, n, surf_ptr, guides_ptr, background, stream)

    def surface_host(self, hits) -> np.ndarray:
        """rtw_world_surface: hits (n,) HIT_DTYPE on the host -> (n,) SURFACE_DTYPE, synchronous."""
        h = np.ascontiguousarray(hits, HIT_DTYPE)
        out = np.zeros(h.shape, SURFACE_DTYPE)
        _check(_wlib().rtw_world_surface(self.h, h.ctypes.data, h.size, out.ctypes.data))
        return out

    def prev_points_device(self, hits_ptr: int, n: int, time: float, out_ptr: int, a_prev_ptr: int | None = None,
                           xv_prev_ptr: int | None = None, stream: int | None = None):
        """rtw_world_prev_points_device: for n rtw_hit records of this world as it is now, the same surface
        points under the previous frame's numbers (device arrays shaped as update_device's, None = the
        current values) into n x 3 float64, asynchronous on `stream`."""
        _check(_wlib().rtw_world_prev_points_device(self.h, C.c_void_p(hits_ptr) if hits_ptr else None, n, float(time),
                                                    C.c_void_p(a_prev_ptr) if a_prev_ptr else None,
                                                    C.c_void_p(xv_prev_ptr) if xv_prev_ptr else None,
                                                    C.c_void_p(out_ptr) if out_ptr else None,
                                                    C.c_void_p(stream) if stream else None))

    def mirror_points_device(self, rays_ptr: int, hits_ptr: int, n: int, cam_prev, out_ptr: int,
                             a_prev_ptr: int | None = None, xv_prev_ptr: int | None = None, opts=None,
                             hits2_ptr: int | None = None, stream: int | None = None):
        """rtw_world_mirror_points_device: prev_points_device with each ray's own time, except that a mirror
        record (a front hit of a metal primitive) gets the point of the mirror that showed the same reflected
        thing from cam_prev under the previous numbers; one launch that walks the reflected rays itself.
        hits2_ptr (optional): n rtw_hit records of the reflected rays.  Asynchronous on `stream`."""
        _check(_wlib().rtw_world_mirror_points_device(self.h, C.c_void_p(rays_ptr) if rays_ptr else None,
                                                      C.c_void_p(hits_ptr) if hits_ptr else None, n,
                                                      C.byref(cam_prev) if cam_prev is not None else None,
                                                      C.c_void_p(a_prev_ptr) if a_prev_ptr else None,
                                                      C.c_void_p(xv_prev_ptr) if xv_prev_ptr else None,
                                                      C.byref(opts) if opts is not None else None,
                                                      C.c_void_p(out_ptr) if out_ptr else None,
                                                      C.c_void_p(hits2_ptr) if hits2_ptr else None,
                                                      C.c_void_p(stream) if stream else None))

    def query_info(self, opts: QueryOpts | None = None) -> dict:
        """rtw_world_query_info: the walk a query runs (after AUTO and the world's limits),
        its kernel feature set, the workgroups of a device-filling batch, LDS per workgroup."""
        out = (C.c_uint32 * 4)()
        _check(_wlib().rtw_world_query_info(self.h, C.byref(opts) if opts is not None else None, out))
        return {"traversal": TRAVERSAL_NAMES.get(int(out[0]), str(out[0])), "feature_set": int(out[1]),
                "grid": int(out[2]), "lds_bytes": int(out[3])}

    def counts(self, cam: Camera, params: Params, workspace_ptr: int, workspace_bytes_: int) -> dict:
        """rtw_world_render_counts_ex: the counts, the persistent kernel's wave
        iterations and whether tail dealing ran (the workspace held the rings),
        plus the traversal that ran (rtw_world_launch_info)."""
        out = (C.c_uint64 * 8)()
        _check(_wlib().rtw_world_render_counts_ex(self.h, C.byref(cam), C.byref(params),
                                                  C.c_void_p(workspace_ptr), workspace_bytes_, out))
        return {"samples": int(out[0]), "segments": int(out[1]), "node_visits": int(out[2]),
                "prim_tests": int(out[3]), "wave_iters": int(out[4]), "tail_dealing": bool(out[5]),
                "lane_interior_iters": int(out[6]), "lane_leaf_iters": int(out[7]),
                "traversal": self.launch_info(params)["traversal"] if hasattr(_wlib(), "rtw_world_launch_info")
                else None}

    def close(self):
        if self.h:
            _wlib().rtw_world_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


__all__ = ["BuiltScene", "DeviceWorld", "refit_tables_host", "rebuild_tables_host", "prev_points_host", "mirror_rays_host", "mirror_points_host", "desc_numbers", "render_world", "load_png", "earth_map", "synthetic_world_map", "RtwError", "SCENES"]
