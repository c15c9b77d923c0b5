"""Inputs of the dynamic-world tests (tests/test_refit_host.py on the CPU,
tests/test_gpu_world_update.py on the GPU): updated descriptions of the mixed
worlds of helpers.mixed_bvh_world, the numbers an update takes, and a
descriptor's dump for tests/native/refit_check.cpp."""
import copy
import struct

import numpy as np

from helpers import _rot


def displace(tables, seed=62, k_range=(3.0, 10.0)):
    """The tables with every geometry number an update may change moved far enough that a
    stale box would prune: every sphere's centre moves by 3-10 of its |radius| in the xz plane
    (spheres that share a centre at creation — the coincident pair, the hollow shell — move
    together); every RotateY op gets a new angle and every Translate op a
    new offset; the first two moving spheres get a new centre1.  The direction points towards the y axis
    within +-0.5 rad, so that the scene stays in the camera's view.  Kinds, materials, transform
    indices, op lists and counts stay.  Returns new tables (the input is not modified)."""
    rng = np.random.default_rng(seed)
    prims, xf = copy.deepcopy(tables[0]), copy.deepcopy(tables[1])
    per_centre, moved_c1, radii = {}, 0, {}
    for p in prims:
        if p["kind"] <= 1:
            radii.setdefault(tuple(p["a"][0:3]), []).append(abs(p["a"][6]))
    for p in prims:
        if p["kind"] > 1:
            continue
        a = p["a"]
        key = (a[0], a[1], a[2])
        if key not in per_centre:
            # one displacement per centre, 3 of its largest radius to 10 of its smallest; towards the
            # middle of the scene (+-0.5 rad), so that what the camera saw stays in view
            rmin, rmax = min(radii[key]), max(radii[key])
            th = np.arctan2(-a[2], -a[0]) + rng.uniform(-0.5, 0.5) if (a[0], a[2]) != (0.0, 0.0) else rng.uniform(0.0, 2.0 * np.pi)
            per_centre[key] = (rng.uniform(k_range[0] * rmax, k_range[1] * rmin), th)
        dist, th = per_centre[key]
        d = dist * np.array([np.cos(th), 0.0, np.sin(th)])
        for c in range(3):
            a[c] = float(a[c] + d[c])
            a[3 + c] = float(a[3 + c] + d[c])
        if p["kind"] == 1 and moved_c1 < 2:
            moved_c1 += 1
            for c in range(3):
                a[3 + c] = float(a[3 + c] + rng.uniform(-0.5, 0.5))
    for x in xf:
        x["v"] = [tuple(v) for v in x["v"]]
        for k in range(x["n"]):
            if x["op"][k] == 0:
                x["v"][k] = tuple(float(c + rng.uniform(-1.0, 1.0)) for c in x["v"][k])
            else:
                x["v"][k] = _rot(x["v"][k][2] + rng.uniform(-0.6, 0.6))
    return (prims, xf) + tuple(tables[2:])


def numbers(tables):
    """(a (n_prims, 9), xv (n_xforms, 4, 3)) float64 of tables in the dict form."""
    prims, xf = tables[0], tables[1]
    a = np.zeros((len(prims), 9))
    for i, p in enumerate(prims):
        a[i, :len(p["a"])] = p["a"]
    xv = np.zeros((len(xf), 4, 3))
    for i, x in enumerate(xf):
        for k in range(x["n"]):
            xv[i, k] = x["v"][k]
    return a, xv


def camera_outside_spheres(tables, look_from, margin=0.05):
    """The render / query input domain: the camera lies outside every sphere, at every shutter time."""
    o = np.array(look_from, float)
    for p in tables[0]:
        if p["kind"] > 1 or p["xform"] >= 0:
            continue
        a = np.array(p["a"], float)
        ends = [a[0:3]] if p["kind"] == 0 else [a[0:3] + (a[3:6] - a[0:3]) * ((s - a[7]) / (a[8] - a[7])) for s in (0, 1)]
        # (a segment's distance to the camera is at least the smaller end distance minus its length)
        dist = min(np.linalg.norm(o - e) for e in ends) - (np.linalg.norm(ends[-1] - ends[0]) if len(ends) > 1 else 0.0)
        if dist < abs(a[6]) * (1 + margin):
            return False
    return True


def truncated(W, desc, n_prims):
    """A descriptor of the first n_prims primitives of desc (it points into the same arrays)."""
    d = W.WorldDesc()
    for f, _ in W.WorldDesc._fields_:
        setattr(d, f, getattr(desc, f))
    d.n_prims = n_prims
    return d


def dump_desc(desc, flags, path):
    """The descriptor as tests/native/refit_check.cpp reads it: flags, then each array as a count
    and the C structs' bytes (images: width, height, pixels)."""
    import ctypes as C
    with open(path, "wb") as f:
        f.write(struct.pack("<I", flags))
        for arr, n in ((desc.prims, desc.n_prims), (desc.xforms, desc.n_xforms), (desc.textures, desc.n_textures),
                       (desc.mats, desc.n_mats), (desc.perlins, desc.n_perlins)):
            f.write(struct.pack("<I", n))
            if n:
                f.write(C.string_at(arr, n * C.sizeof(arr._type_)))
        f.write(struct.pack("<I", desc.n_images))
        for i in range(desc.n_images):
            im = desc.images[i]
            f.write(struct.pack("<II", im.width, im.height))
            f.write(C.string_at(im.rgba, im.width * im.height * 4))


def prims_with(W, desc, a):
    """A ctypes array of the descriptor's primitives with the numbers a ((n_prims, 9))."""
    import ctypes as C
    n = desc.n_prims
    arr = (W.Prim * max(1, n))()
    if n:
        C.memmove(arr, desc.prims, n * C.sizeof(W.Prim))
        np.frombuffer(arr, np.float64).reshape(-1, 11)[:n, 2:11] = a  # (16 bytes of header, then a[9])
    return arr


def xforms_with(W, desc, xv):
    """A ctypes array of the descriptor's transforms with the values xv ((n_xforms, 4, 3))."""
    import ctypes as C
    n = desc.n_xforms
    arr = (W.Xform * max(1, n))()
    if n:
        C.memmove(arr, desc.xforms, n * C.sizeof(W.Xform))
        np.frombuffer(arr, np.float64).reshape(-1, 15)[:n, 3:15] = np.asarray(xv).reshape(n, 12)  # (n, op[4], pad)
    return arr


def blob_nodes(desc, n_nodes, blob):
    """The BVH node records ((n_nodes, 16) uint32) of a world's table bytes: the tables lie in the order
    prim | xform | tex | mat | perlin | image | pixels | nodes | ..., each at a 256-byte aligned offset."""
    def al(b):
        return (b + 255) & ~255
    pix = sum(desc.images[i].width * desc.images[i].height * 4 for i in range(desc.n_images))
    o = (al(128 * (desc.n_prims + 1)) + al(128 * max(desc.n_xforms, 1)) + al(128 * max(desc.n_textures, 1)) +
         al(64 * max(desc.n_mats, 1)) + al((256 * 3 + 384) * 8 * max(desc.n_perlins, 1)) + al(16 * max(desc.n_images, 1)) +
         al(max(pix, 4)))
    return np.frombuffer(blob.tobytes()[o:o + 64 * n_nodes], np.uint32).reshape(n_nodes, 16)


def cull_bits(nodes):
    """How many leaf refs carry kCullBit."""
    refs = nodes[:, 12:14]
    return int((((refs & 0x80000000) != 0) & ((refs & 0x40000000) != 0)).sum())
