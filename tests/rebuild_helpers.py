"""Inputs of the rebuild tests (tests/test_rebuild_host.py on the CPU,
tests/test_gpu_world_rebuild.py on the GPU): three degenerate worlds of 600
spheres whose Morton keys collide — every centre equal, every centre on one
line (two extents of the centroid box are 0), and 300 coincident pairs — in the
dict form helpers._to_desc and oracle.TableWorld take, with the numbers of a
second placement of the same kind."""
import numpy as np

N_DEGENERATE = 600
DEGENERATE = ("same_centre", "on_a_line", "pairs")


def degenerate_world(W, kind, moved=False):
    """(prims, xforms, textures, materials, perlins, images) of one degenerate world, in view of
    helpers.MIXED_CAMERA.  moved: the second placement (same kinds, materials and counts).
      same_centre: 600 concentric spheres, radii 0.5 .. 3.5 (every centroid equal: one key);
      on_a_line:   600 spheres of radius 0.05 on the line x = -9 .. 9, y = 2, z = 0;
      pairs:       300 random centres, each held by two spheres (radius r, and 0.8 r)."""
    rng = np.random.default_rng({"same_centre": 11, "on_a_line": 12, "pairs": 13}[kind] + (100 if moved else 0))
    n = N_DEGENERATE
    if kind == "same_centre":
        c = np.tile(np.array([1.5, 2.0, -1.0]) if moved else np.array([0.0, 2.0, 0.0]), (n, 1))
        r = 0.5 + 3.0 * np.arange(n) / (n - 1)
    elif kind == "on_a_line":
        x = np.linspace(-9.0, 9.0, n)
        if moved:
            x = rng.permutation(x)
        c = np.stack([x, np.full(n, 2.0), np.zeros(n)], axis=1)
        r = np.full(n, 0.05)
    else:
        half = np.stack([rng.uniform(-8, 8, n // 2), rng.uniform(0.3, 4.0, n // 2), rng.uniform(-8, 4, n // 2)], axis=1)
        c = np.repeat(half, 2, axis=0)
        r = np.repeat(rng.uniform(0.1, 0.3, n // 2), 2) * np.tile([1.0, 0.8], n // 2)
    prims = [dict(kind=W.PRIM_SPHERE, mat=i % 3, xform=-1, cls="base",
                  a=[float(c[i, 0]), float(c[i, 1]), float(c[i, 2]), float(c[i, 0]), float(c[i, 1]), float(c[i, 2]),
                     float(r[i]), 0.0, 0.0]) for i in range(n)]
    tex = [dict(kind=W.TEX_SOLID, color=(0.7, 0.3, 0.3)), dict(kind=W.TEX_SOLID, color=(0.3, 0.6, 0.8))]
    mats = [dict(kind=W.WMAT_LAMBERT, tex=0), dict(kind=W.WMAT_METAL, albedo=(0.8, 0.8, 0.9), fuzz=0.1),
            dict(kind=W.WMAT_LAMBERT, tex=1)]
    return prims, [], tex, mats, [], []
