"""Helpers of the denoiser's tests: the feature buffers restated
on the oracle (World.hit + rw_texture_value on the feature ray of rtw_hip.h),
and the unguided B3 blur in numpy."""
import ctypes as C

import numpy as np

T_MIN = 0.001


def feature_ray(cam, W, H, x, y):
    """Camera.getRay (main.zig:91-100) with its two draws at their means, in f64."""
    s = (x + 0.5) / (W - 1)
    t = ((H - 1 - y) + 0.5) / (H - 1)
    o = [cam.origin[k] for k in range(3)]
    d = [((cam.lower_left_corner[k] + cam.horizontal[k] * s) + cam.vertical[k] * t) - o[k] for k in range(3)]
    return o, d, cam.time0 + 0.5 * (cam.time1 - cam.time0)


def oracle_guides(oracle, world, cam, W, H, background, rows=None):
    """The guides of image rows `rows` (default: all) from the oracle, in f64:
    dict of normal (n, W, 3), depth (n, W), albedo (n, W, 3), prim (n, W) int."""
    L = oracle._world_lib()
    rows = list(range(H)) if rows is None else list(rows)
    n = len(rows)
    out = {"normal": np.zeros((n, W, 3)), "depth": np.zeros((n, W)), "albedo": np.zeros((n, W, 3)),
           "prim": np.zeros((n, W), np.int64)}
    out["albedo"][:] = background
    arr = C.c_double * 3
    w = world.w
    for q, y in enumerate(rows):
        for x in range(W):
            o, d, time = feature_ray(cam, W, H, x, y)
            h = world.hit(o, d, time, T_MIN, float("inf"))
            if h is None:
                continue
            m = w.mats[w.prims[h["prim"]].mat]
            if m.kind == oracle.RW_METAL:
                alb = list(m.albedo)
            elif m.kind == oracle.RW_DIELECTRIC:
                alb = [1.0, 1.0, 1.0]
            else:  # Lambert: the texture's value; Light: the emit texture's
                c = arr()
                L.rw_texture_value(world.ptr, m.tex, h["uv"][0], h["uv"][1], arr(*h["p"]), c)
                alb = list(c)
            out["normal"][q, x] = h["normal"]
            out["depth"][q, x] = h["t"]
            out["albedo"][q, x] = alb
            out["prim"][q, x] = h["prim"] + 1
    return out


def guides_record(rtw, g):
    """The f64 dict of oracle_guides as an array of rtw_guide records (f32 on store)."""
    r = np.zeros(g["prim"].shape, rtw.GUIDE_DTYPE)
    r["normal"], r["depth"], r["albedo"], r["prim"] = g["normal"], g["depth"], g["albedo"], g["prim"]
    return r


def b3_blur(img, levels=5):
    """The unguided a-trous B3-spline blur: every weight term but the spline's
    dropped, taps outside the image dropped, normalised.  img: (H, W, 3)."""
    k = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16])
    cur = np.asarray(img, np.float64)
    H, W = cur.shape[:2]
    for l in range(levels):
        s = 1 << l
        for axis, n in ((0, H), (1, W)):
            acc = np.zeros_like(cur)
            wsum = np.zeros((H, W, 1))
            for i, kw in zip(range(-2, 3), k):
                lo, hi = max(0, -i * s), min(n, n - i * s)  # destination range whose tap lies inside
                if lo >= hi:
                    continue
                dst = [slice(None)] * 3
                src = [slice(None)] * 3
                dst[axis], src[axis] = slice(lo, hi), slice(lo + i * s, hi + i * s)
                acc[tuple(dst)] += kw * cur[tuple(src)]
                wsum[tuple(dst[:2]) + (slice(None),)] += kw
            cur = acc / wsum
    return cur


def rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))


def luminance(img):
    return (0.2126 * img[..., 0] + 0.7152 * img[..., 1]) + 0.0722 * img[..., 2]
