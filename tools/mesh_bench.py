#!/usr/bin/env python3
"""Triangle worlds next to the sphere world they were made from.

  python tools/mesh_bench.py [--rounds 3] [--spp 20] [--out FILE]

Sphere world: scene 7 (the globe with the real map + 10k spheres, as bench.py uses it).  Mesh world: the same
scene with the globe as a level-5 icosphere (20,480 triangles, a checker texture: an image texture on a triangle
reads barycentrics) and every other sphere of radius < 100 as the icosahedron inscribed in it (20 triangles each; a
moving sphere at its first centre), its material kept; the ground sphere (radius 1000) stays a sphere: ~220k
triangles, generated from the scene's seed alone.  Both worlds are DYNAMIC.
Reported, each figure of the mesh world next to the sphere world's of the same run:
  * render, 1200x675 x --spp: Msamples/s under the union walk and the per-lane walk (rtw_timer's HIP events around
    the kernel), and the register budget / feature set rtw_world_launch_info reports; for the mesh world also the
    4-wave budget (params.world_waves = 4), the alternative to its 3-wave default;
  * ray queries: the frame's feature rays (P) and one incoherent bounce per hit (S), closest hit under UNION and
    LANE, HIP events around back-to-back launches filling ~200 ms (query_bench.py's protocol);
  * rtw_world_update_device and rtw_world_rebuild_device of the world's own numbers from a device tensor, HIP
    events, and rtw_world_bvh_cost.
Protocol: one process, warm-up first, the variants alternate for --rounds rounds, median (min .. max); the shader
clock over the timed part is rtw_sclk_probe's.  A render, an update and a rebuild are timed one launch per sample
(each is milliseconds long, and an update or rebuild ends in its own readback); only the queries fill a time window.
(icosahedron / icosphere restate tests/tri_helpers.py's: the tool stands alone, it imports nothing from tests/.)"""
import argparse
import ctypes as C
import math
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "raytracinginoneweekend.zig_amd"))

PRIM_DT = np.dtype([("kind", np.uint32), ("mat", np.uint32), ("xform", np.int32), ("reserved", np.uint32), ("a", np.float64, 9)])


def icosahedron():
    t = (1.0 + math.sqrt(5.0)) / 2.0
    v = np.array([[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t],
                  [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]], float)
    f = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2],
                  [10, 7, 6], [7, 1, 8], [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11],
                  [6, 2, 10], [8, 6, 7], [9, 8, 1]])
    return v / np.linalg.norm(v[0]), f


def icosphere(level):
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


def mesh_desc(Wd, b):
    """scene 7's description with every sphere as a mesh; returns (desc, keep-alive list, triangle count)."""
    d = b.desc
    src = np.frombuffer((C.c_char * (d.n_prims * PRIM_DT.itemsize)).from_address(C.addressof(d.prims.contents)), PRIM_DT)
    tex_kind = [d.textures[i].kind for i in range(d.n_textures)]
    is_globe = np.array([d.mats[int(m)].kind in (Wd.WMAT_LAMBERT, Wd.WMAT_LIGHT) and tex_kind[d.mats[int(m)].tex] == Wd.TEX_IMAGE
                         for m in src["mat"]])
    big = src["a"][:, 6] >= 100.0
    assert (src["kind"] <= Wd.PRIM_MOVING_SPHERE).all() and is_globe.sum() == 1 and not (big & is_globe).any()
    # tables: the scene's, plus a checker texture and a Lambertian over it for the globe
    tex = (Wd.Texture * (d.n_textures + 1))(*[d.textures[i] for i in range(d.n_textures)])
    tex[d.n_textures].kind = Wd.TEX_CHECKER
    tex[d.n_textures].odd[:], tex[d.n_textures].even[:] = (0.2, 0.3, 0.1), (0.9, 0.9, 0.9)
    mats = (Wd.WMaterial * (d.n_mats + 1))(*[d.mats[i] for i in range(d.n_mats)])
    mats[d.n_mats].kind, mats[d.n_mats].tex = Wd.WMAT_LAMBERT, d.n_textures
    iv, if_ = icosahedron()
    gv, gf = icosphere(5)
    small = src[~is_globe & ~big]
    tri_small = (small["a"][:, None, None, :3] + small["a"][:, None, None, 6:7] * iv[if_][None]).reshape(-1, 9)
    g = src[is_globe][0]
    tri_globe = (g["a"][:3] + g["a"][6] * gv[gf]).reshape(-1, 9)
    nb, ng = int(big.sum()), len(tri_globe)
    n = nb + ng + len(tri_small)
    out = np.zeros(n, PRIM_DT)
    out["kind"], out["xform"] = Wd.PRIM_TRIANGLE, -1
    out[:nb] = src[big]
    out["a"][nb:nb + ng], out["mat"][nb:nb + ng] = tri_globe, d.n_mats
    out["a"][nb + ng:], out["mat"][nb + ng:] = tri_small, np.repeat(small["mat"], 20)
    md = Wd.WorldDesc()
    md.prims, md.n_prims = C.cast(out.ctypes.data, C.POINTER(Wd.Prim)), n
    md.textures, md.n_textures = C.cast(tex, C.POINTER(Wd.Texture)), d.n_textures + 1
    md.mats, md.n_mats = C.cast(mats, C.POINTER(Wd.WMaterial)), d.n_mats + 1
    md.images, md.n_images = d.images, d.n_images
    return md, [out, tex, mats], n - nb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--spp", type=int, default=20)
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import rtw_amd as R
    from rtw_amd import world as Wd
    from rtw_amd.device import TorchTracer, rebuild_world, update_world
    if not torch.cuda.is_available():
        raise SystemExit("mesh_bench needs a GPU (there is no CPU path)")
    dev = torch.device("cuda", 0)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def med(x):
        return f"{statistics.median(x):.4f} (min {min(x):.4f} .. max {max(x):.4f})"

    W, H, spp = 1200, 675, args.spp
    b = Wd.BuiltScene(7, 42, image=Wd.earth_map())
    mdesc, keep, n_tri = mesh_desc(Wd, b)
    cam = b.camera(W / H)
    worlds = {"spheres": (b.desc, Wd.DeviceWorld(b.desc, dynamic=True)), "mesh": (mdesc, Wd.DeviceWorld(mdesc, dynamic=True))}
    say(f"device: {torch.cuda.get_device_name(0)}")
    for name, (desc, dw) in worlds.items():
        say(f"{name}: {desc.n_prims} primitives, BVH {dw.bvh_info()}")
    stream = torch.cuda.current_stream(dev).cuda_stream
    side = torch.cuda.Stream()
    clk = R.SclkProbe(side.cuda_stream, 60000.0)

    # ---- render
    rgb = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
    variants = {}
    for name, (desc, dw) in worlds.items():
        for trav in ("union", "lane"):
            for waves in ((0, 4) if name == "mesh" else (0,)):
                p = R.make_params(W, H, spp, background=b.background, world_traversal=trav, world_waves=waves)
                need = dw.workspace_bytes(p)
                ws = torch.empty(need + 256, dtype=torch.uint8, device=dev)
                variants[f"{name} {trav} waves={waves or 'default'}"] = (dw, p, ws, need, dw.launch_info(p))
    times = {k: [] for k in variants}
    for rnd in range(args.rounds + 1):  # (round 0: warm-up)
        for k, (dw, p, ws, need, li) in variants.items():
            tm = R.Timer()
            dw.render_async(cam, p, (ws.data_ptr() + 255) & ~255, need, rgb.data_ptr(), None, stream, tm)
            torch.cuda.synchronize()
            if rnd:
                times[k].append(tm.elapsed_ms())
            tm.close()
    say(f"render {W}x{H}x{spp} (kernel ms by HIP events; {args.rounds} alternating rounds after one warm-up)")
    for k, (dw, p, ws, need, li) in variants.items():
        m = statistics.median(times[k])
        say(f"  {k:<28} {W * H * spp / m / 1e3:9.2f} Msamples/s  {med(times[k])} ms  ran {li['traversal']}, feature set "
            f"{li['feature_set']}, budget {li['waves']} waves")

    # ---- queries
    def time_launches(fn, k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(k):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / k

    f64 = dict(dtype=torch.float64, device=dev)
    s = (torch.arange(W, **f64) + 0.5) / (W - 1)
    t = ((H - 1 - torch.arange(H, **f64)) + 0.5) / (H - 1)
    v = {n: torch.tensor(list(getattr(cam, n)), **f64) for n in ("origin", "horizontal", "vertical", "lower_left_corner")}
    d = ((v["lower_left_corner"] + v["horizontal"] * s[None, :, None]) + v["vertical"] * t[:, None, None]) - v["origin"]
    o = v["origin"].expand(H, W, 3).reshape(-1, 3).contiguous()
    d = d.reshape(-1, 3).contiguous()
    qv = {}
    for name, (desc, dw) in worlds.items():
        tr = TorchTracer(dw)
        P = tr.pack(o, d, time=0.5)
        hit = tr.trace(o, d, time=0.5)
        torch.cuda.synchronize()
        m = hit["prim"] >= 0
        g = torch.Generator(device=dev)
        g.manual_seed(1235)
        u = torch.randn((int(m.sum()), 3), generator=g, dtype=torch.float64, device=dev)
        S = tr.pack(hit["p"][m].contiguous(), hit["normal"][m] + u / u.norm(dim=1, keepdim=True), time=0.5)
        rec = torch.empty((P.shape[0], 10), dtype=torch.float64, device=dev)
        for label, rays in (("P", P), ("S", S)):
            for trav in ("union", "lane"):
                opts = R.QueryOpts(R.WORLD_TRAVERSAL[trav], 0)
                qi = dw.query_info(opts)
                qv[f"{name} {label} {trav}"] = (lambda dw=dw, rays=rays, opts=opts: dw.trace(rays.data_ptr(), rays.shape[0], rec.data_ptr(), opts, stream),
                                                rays.shape[0], qi, rec)
    counts, qt = {}, {k: [] for k in qv}
    for k, (fn, n, qi, _) in qv.items():
        time_launches(fn, 2)
        counts[k] = max(1, min(2000, math.ceil(args.window_ms / max(time_launches(fn, 1), 1e-3))))
    for _ in range(args.rounds):
        for k, (fn, n, qi, _) in qv.items():
            qt[k].append(time_launches(fn, counts[k]))
    say("closest-hit queries: (P) the frame's feature rays, (S) one bounce per hit")
    for k, (fn, n, qi, _) in qv.items():
        m = statistics.median(qt[k])
        say(f"  {k:<22} {n / m / 1e3:10.1f} Mrays/s  {med(qt[k])} ms/launch  {n} rays, {counts[k]} launches x {args.rounds} rounds, "
            f"ran {qi['traversal']}, feature set {qi['feature_set']}")

    # ---- update, rebuild
    say("update / rebuild of the world's own numbers from a device tensor (ms by HIP events around ONE call per sample, "
        f"{args.rounds} samples after one warm-up; each call waits for its readback)")
    for name, (desc, dw) in worlds.items():
        a, _ = (np.frombuffer((C.c_char * (desc.n_prims * PRIM_DT.itemsize)).from_address(C.addressof(desc.prims.contents)), PRIM_DT)["a"].copy(), None)
        ta = torch.from_numpy(a).to(dev)
        res = {"update": [], "rebuild": []}
        for rnd in range(args.rounds + 1):
            for what, fn in (("update", update_world), ("rebuild", rebuild_world)):
                ms = time_launches(lambda: fn(dw, ta), 1)
                if rnd:
                    res[what].append(ms)
        say(f"  {name:<8} update {med(res['update'])} ms   rebuild {med(res['rebuild'])} ms   tree cost after the rebuild {dw.bvh_cost():.2f}")
    torch.cuda.synchronize()
    say(f"shader clock over the timed part: {clk.read():.1f} MHz")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    for _, dw in worlds.values():
        dw.close()


if __name__ == "__main__":
    main()
