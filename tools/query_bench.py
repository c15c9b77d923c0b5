#!/usr/bin/env python3
"""Throughput of the ray queries (rtw_world_trace_device / rtw_world_occluded_device,
DESIGN.md §15) in Mrays/s, and the numbers behind the AUTO traversal rule.

  python tools/query_bench.py [--rounds 3] [--window-ms 300] [--out FILE] [--scene-api]

Worlds: scene 7 (the globe with the real map, as bench.py uses it; 1200x675),
scene 6 (the Cornell box, the linear loop; 600x600) and scene 1 as a world
(1200x800: a BVH of a few dozen nodes, the small end of the AUTO rule).  Ray batches, built once
and kept on the device:
  (P) the frame's feature rays (rtw_pixel_ray's definition, evaluated with torch);
  (S) one incoherent bounce per hit of (P): origin p, direction normal + unit
      vector from a seeded generator.
Timing: HIP events around enough back-to-back launches of one variant to fill
--window-ms, after a warm-up; the variants alternate in one process for
--rounds rounds; the median and the spread (min .. max) of the rounds are
reported.  On (P) the guides kernel (rtw_world_guides_device) of the same frame
is timed the same way: before the queries it was the only first-hit facility,
so its time is the baseline and the ratio is printed.  AUTO follows whichever
of UNION / LANE is faster on (S); the verdict line says whether the two lie
within the measured spread.

--scene-api measures the scene entries instead (rtw_scene_trace_device / rtw_scene_occluded_device /
rtw_scene_guides_device: scene_query_kernel and scene_guides_kernel over the packed sphere table) on
cover_scene(42) at 1200x800 with the same (P) and (S) batches, and ends with one line
"scene_api_ms closest_P=.. occlusion_P=.. closest_S=.. occlusion_S=.. guides=.." of the medians, for
A/B runs of two libraries (RTW_LIB_PATH), each in a process of its own."""
import argparse
import math
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "raytracinginoneweekend.zig_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--max-launches", type=int, default=4000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--scene-api", action="store_true")
    args = ap.parse_args()
    import torch
    import rtw_amd as R
    from rtw_amd import world as Wd
    from rtw_amd.device import TorchTracer
    if not torch.cuda.is_available():
        raise SystemExit("query_bench needs a GPU (there is no CPU path)")
    dev = torch.device("cuda", 0)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def feature_rays(cam, W, H):
        """(P): Camera.getRay with its draws at their means, for every pixel, rows top first."""
        f64 = dict(dtype=torch.float64, device=dev)
        s = (torch.arange(W, **f64) + 0.5) / (W - 1)
        t = ((H - 1 - torch.arange(H, **f64)) + 0.5) / (H - 1)
        v = {n: torch.tensor(list(getattr(cam, n)), **f64) for n in ("origin", "horizontal", "vertical", "lower_left_corner")}
        d = ((v["lower_left_corner"] + v["horizontal"] * s[None, :, None]) + v["vertical"] * t[:, None, None]) - v["origin"]
        o = v["origin"].expand(H, W, 3)
        return o.reshape(-1, 3).contiguous(), d.reshape(-1, 3).contiguous(), cam.time0 + 0.5 * (cam.time1 - cam.time0)

    def time_launches(fn, k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(k):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / k

    def bench(variants):
        """variants: {name: (launch, rays per launch)} -> {name: [ms per launch, one per round]}"""
        counts, out = {}, {n: [] for n in variants}
        for name, (fn, _) in variants.items():  # warm-up, and the launches that fill the window
            time_launches(fn, 2)
            one = time_launches(fn, 1)
            counts[name] = max(1, min(args.max_launches, math.ceil(args.window_ms / max(one, 1e-3))))
        for _ in range(args.rounds):
            for name, (fn, _) in variants.items():
                out[name].append(time_launches(fn, counts[name]))
        return out, counts

    def report(title, variants, res, counts):
        say(title)
        for name, (_, n) in variants.items():
            ms = res[name]
            med = statistics.median(ms)
            say(f"  {name:<28} {n / med / 1e3:10.1f} Mrays/s   {med:9.4f} ms/launch  (min {min(ms):.4f} .. max {max(ms):.4f}, "
                f"{counts[name]} launches x {len(ms)} rounds)")

    say(f"device: {torch.cuda.get_device_name(0)}")
    if args.scene_api:
        W, H = 1200, 800
        sph, mats, _ = R.cover_scene(42)
        sc = R.DeviceScene(sph, mats)
        cam = R.cover_camera(W / H)
        tr = TorchTracer(sc)
        o, d, time = feature_rays(cam, W, H)
        P = tr.pack(o, d, time=time)
        hit = tr.trace(o, d, time=time)
        torch.cuda.synchronize()
        m = hit["prim"] >= 0
        g = torch.Generator(device=dev)
        g.manual_seed(1235)
        u = torch.randn((int(m.sum()), 3), generator=g, dtype=torch.float64, device=dev)
        u = u / u.norm(dim=1, keepdim=True)
        S = tr.pack(hit["p"][m].contiguous(), hit["normal"][m] + u, time=time)
        say(f"scene API, cover_scene(42) ({len(sph)} spheres), {W}x{H}: (P) {P.shape[0]} rays, {int(m.sum())} hit; (S) {S.shape[0]} rays"
            f"; library {R.LIB_PATH}")
        stream = torch.cuda.current_stream(dev).cuda_stream
        rec = torch.empty((P.shape[0], 10), dtype=torch.float64, device=dev)
        occ = torch.empty((P.shape[0],), dtype=torch.uint8, device=dev)
        guides = torch.empty((H, W, 32), dtype=torch.uint8, device=dev)
        params = R.make_params(W, H, 1)
        variants = {}
        for label, rays in (("P", P), ("S", S)):
            n = rays.shape[0]
            variants[f"closest_{label}"] = (lambda rays=rays, n=n: sc.trace(rays.data_ptr(), n, rec.data_ptr(), stream), n)
            variants[f"occlusion_{label}"] = (lambda rays=rays, n=n: sc.occluded(rays.data_ptr(), n, occ.data_ptr(), stream), n)
        variants["guides"] = (lambda: sc.guides(cam, params, guides.data_ptr(), stream), P.shape[0])
        res, counts = bench(variants)
        report("  scene entries", variants, res, counts)
        say("scene_api_ms " + " ".join(f"{k}={statistics.median(v):.5f}" for k, v in res.items()))
        sc.close()
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    for sid, W, H in ((7, 1200, 675), (6, 600, 600), (1, 1200, 800)):
        img = Wd.earth_map() if sid == 7 else None
        built = Wd.BuiltScene(sid, 42, img)
        world = Wd.DeviceWorld(built.desc)
        cam = built.camera(W / H)
        tr = TorchTracer(world)
        o, d, time = feature_rays(cam, W, H)
        P = tr.pack(o, d, time=time)
        hit = tr.trace(o, d, time=time)
        torch.cuda.synchronize()
        m = hit["prim"] >= 0
        g = torch.Generator(device=dev)
        g.manual_seed(1234 + sid)
        u = torch.randn((int(m.sum()), 3), generator=g, dtype=torch.float64, device=dev)
        u = u / u.norm(dim=1, keepdim=True)
        S = tr.pack(hit["p"][m].contiguous(), hit["normal"][m] + u, time=time)
        info = {k: world.query_info(R.query_opts(k)) for k in ("auto", "union", "lane")}
        say()
        say(f"scene {sid} ({built.desc.n_prims} primitives, BVH {world.bvh_info()}), {W}x{H}: (P) {P.shape[0]} rays, "
            f"{int(m.sum())} hit; (S) {S.shape[0]} rays")
        say("  walks: " + ", ".join(f"{k} -> {v['traversal']} (feature set {v['feature_set']}, grid {v['grid']}, "
                                    f"LDS {v['lds_bytes']} B)" for k, v in info.items()))
        walks = ["auto"] if info["lane"]["traversal"] == info["union"]["traversal"] else ["union", "lane"]
        stream = torch.cuda.current_stream(dev).cuda_stream
        rec = torch.empty((P.shape[0], 10), dtype=torch.float64, device=dev)
        occ = torch.empty((P.shape[0],), dtype=torch.uint8, device=dev)
        guides = torch.empty((H, W, 32), dtype=torch.uint8, device=dev)
        params = R.make_params(W, H, 1, background=built.background)
        for label, rays in (("P", P), ("S", S)):
            n = rays.shape[0]
            variants = {}
            for wk in walks:
                opts = R.query_opts(wk)
                variants[f"closest   {info[wk]['traversal']}"] = (
                    lambda opts=opts, rays=rays, n=n: world.trace(rays.data_ptr(), n, rec.data_ptr(), opts, stream), n)
                variants[f"occlusion {info[wk]['traversal']}"] = (
                    lambda opts=opts, rays=rays, n=n: world.occluded(rays.data_ptr(), n, occ.data_ptr(), opts, stream), n)
            if label == "P":
                variants["guides kernel (baseline)"] = (lambda: world.guides(cam, params, guides.data_ptr(), stream), n)
            res, counts = bench(variants)
            report(f"  ({label})", variants, res, counts)
            med = {k: statistics.median(v) for k, v in res.items()}
            if label == "P":
                default = f"closest   {info['auto']['traversal']}"
                say(f"  default query of (P) vs the guides kernel: {med[default]:.4f} ms vs "
                    f"{med['guides kernel (baseline)']:.4f} ms, ratio {med['guides kernel (baseline)'] / med[default]:.1f}x")
            if label == "S" and len(walks) == 2:
                a, b = res["closest   union"], res["closest   lane"]
                apart = max(a) < min(b) or max(b) < min(a)
                faster = "union" if med["closest   union"] < med["closest   lane"] else "lane"
                say(f"  AUTO on (S): union {med['closest   union']:.4f} ms, lane {med['closest   lane']:.4f} ms -> "
                    + (f"{faster} (the rounds do not overlap)" if apart else
                       "within the measured spread: AUTO keeps rtw_params.world_traversal's rule"))
        world.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
