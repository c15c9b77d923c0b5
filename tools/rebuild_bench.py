#!/usr/bin/env python3
"""Cost and worth of a device rebuild (rtw_world_rebuild / rtw_world_rebuild_device,
DESIGN.md §17) on the globe + 10k spheres (scene 7, the real map).

  python tools/rebuild_bench.py [--repeats 5] [--spp 100] [--out FILE]
  python tools/rebuild_bench.py --only-rebuilds N      (for a kernel trace: N device rebuilds, nothing else)

The method of tools/update_bench.py: alternating rounds in one process after a
warm-up round, median (min .. max), the shader clock (rtw_sclk_probe) noted.
  * host wall time incl. a synchronise of rebuild (host arrays), rebuild (device
    arrays), update (device arrays) and rtw_world_create + destroy of the same
    description;
  * render of configs[4] (1200x675) after every small sphere moved by k = 0, 0.5,
    2, 4, 8 of its radii on three trees — the created tree refitted, the device-
    rebuilt tree, a freshly created (SAH) tree: HIP-event kernel time, node
    visits, rtw_world_bvh_cost, and whether the three images are identical.
Per-stage kernel times and launch counts come from a kernel trace of
--only-rebuilds (the stage of a kernel is its name: wu_* validation and commit,
rb_* the rebuild's own, rocprim::* the sort)."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "raytracinginoneweekend.zig_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--spp", type=int, default=100)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only-rebuilds", type=int, default=0)
    args = ap.parse_args()
    import numpy as np
    import torch

    import rtw_amd as R
    from rtw_amd import world as Wd
    from rtw_amd.device import rebuild_world, update_world
    from update_helpers import prims_with, truncated, xforms_with
    if not torch.cuda.is_available():
        raise SystemExit("rebuild_bench needs a GPU (there is no CPU path)")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def fmt(v):
        return f"median {statistics.median(v):9.3f}  ({min(v):.3f} .. {max(v):.3f})"

    def sync():
        torch.cuda.current_stream().synchronize()

    def wall(f):
        sync()
        t0 = time.perf_counter()
        f()
        sync()
        return (time.perf_counter() - t0) * 1e3

    def moved(a0, radii, seed=11):
        rng = np.random.default_rng(seed)
        small = np.abs(a0[:, 6]) < 100
        th = rng.uniform(0, 2 * np.pi, len(a0))
        a = a0.copy()
        for c, f in ((0, np.cos(th)), (2, np.sin(th))):
            step = radii * np.abs(a0[:, 6]) * f
            a[small, c] += step[small]
            a[small, 3 + c] += step[small]
        return a

    b = Wd.BuiltScene(7, 42, image=Wd.earth_map())
    a0, xv0 = Wd.desc_numbers(b.desc)

    def desc_with(a):
        d = truncated(Wd, b.desc, b.desc.n_prims)
        keep = (prims_with(Wd, b.desc, a), xforms_with(Wd, b.desc, xv0))
        d.prims, d.xforms = C.cast(keep[0], C.POINTER(Wd.Prim)), C.cast(keep[1], C.POINTER(Wd.Xform))
        return d, keep
    a1 = moved(a0, 0.5)
    d1, keep1 = desc_with(a1)
    ta = torch.from_numpy(a1).cuda()
    dyn = Wd.DeviceWorld(b.desc, dynamic=True)
    if args.only_rebuilds:
        for _ in range(args.only_rebuilds):
            rebuild_world(dyn, ta, None)
        sync()
        dyn.close()
        return
    t = {k: [] for k in ("rebuild_host", "rebuild_dev", "update_dev", "create")}
    for r in range(args.repeats + 1):
        row = (wall(lambda: dyn.rebuild(d1)), wall(lambda: rebuild_world(dyn, ta, None)),
               wall(lambda: update_world(dyn, ta, None)), wall(lambda: Wd.DeviceWorld(d1).close()))
        if r:  # (round 0 warms up: code objects, the rebuild allocation)
            for k, v in zip(t, row):
                t[k].append(v)
    info = dyn.bvh_info()
    say(f"# globe + 10k spheres (scene 7): {b.desc.n_prims} primitives, BVH {info['nodes']} nodes, rebuilt depth {info['max_depth']}; "
        f"{args.repeats} alternating rounds after one warm-up, host wall ms incl. synchronise")
    say(f"rebuild, host arrays    : {fmt(t['rebuild_host'])}")
    say(f"rebuild, device arrays  : {fmt(t['rebuild_dev'])}")
    say(f"update, device arrays   : {fmt(t['update_dev'])}")
    say(f"rtw_world_create+destroy: {fmt(t['create'])}")
    say(f"create / rebuild (device arrays) {statistics.median(t['create']) / statistics.median(t['rebuild_dev']):.1f}x, "
        f"rebuild / update (device arrays) {statistics.median(t['rebuild_dev']) / statistics.median(t['update_dev']):.1f}x")
    dyn.close()

    s = b.settings
    cam = b.camera()
    p = R.make_params(s.width, s.height, args.spp, 50, 42, background=b.background)
    refit, rebuilt = Wd.DeviceWorld(b.desc, dynamic=True), Wd.DeviceWorld(b.desc, dynamic=True)
    need = refit.workspace_bytes(p)
    ws = torch.empty(need + 256, dtype=torch.uint8, device="cuda:0")
    ptr = (ws.data_ptr() + 255) & ~255
    rgb = [torch.empty((s.height, s.width, 3), dtype=torch.uint8, device="cuda:0") for _ in range(3)]

    def frame(dw, out):
        tm = R.Timer()
        dw.render_async(cam, p, ptr, need, out.data_ptr(), None, torch.cuda.current_stream().cuda_stream, tm)
        sync()
        ms = tm.elapsed_ms()
        tm.close()
        return ms
    say(f"# render of {s.width}x{s.height}x{args.spp} (configs[4]) after every small sphere moved by k radii, on the created tree refitted, "
        f"the device-rebuilt tree and a freshly created (SAH) tree; kernel ms, {args.repeats} alternating repeats after a warm-up")
    ks = (0.0, 0.5, 2.0, 4.0, 8.0)  # (4: between the two rows where the rebuilt tree starts to win)
    frame(refit, rgb[0])
    est = frame(refit, rgb[0])
    clk_stream = torch.cuda.Stream()
    clk = R.SclkProbe(clk_stream.cuda_stream, max(1.0, 0.8 * est * 3 * (args.repeats + 1) * len(ks)))
    rows, held = [], []
    for k in ks:
        a = moved(a0, k)
        d, keep = desc_with(a)
        tk = torch.from_numpy(a).cuda()
        update_world(refit, tk, None)
        rebuild_world(rebuilt, tk, None)
        fresh = Wd.DeviceWorld(d)
        tt = ([], [], [])
        for r in range(args.repeats + 1):
            x = [frame(w, o) for w, o in zip((refit, rebuilt, fresh), rgb)]
            if r:
                for v, y in zip(tt, x):
                    v.append(y)
        rows.append((k, tt, bool(torch.equal(rgb[0], rgb[1]) and torch.equal(rgb[0], rgb[2]))))
        held.append(fresh)  # (freeing device memory waits for the whole device, the probe's wave included)
    mhz = clk.read()
    for w in held:
        w.close()
    for k, tt, same in rows:  # (counts and costs wait for the whole device: after the probe)
        a = moved(a0, k)
        d, keep = desc_with(a)
        tk = torch.from_numpy(a).cuda()
        update_world(refit, tk, None)
        rebuild_world(rebuilt, tk, None)
        fresh = Wd.DeviceWorld(d)
        trees = (("refitted", refit), ("rebuilt", rebuilt), ("created", fresh))
        visits = {n: w.counts(cam, p, ptr, need)["node_visits"] for n, w in trees}
        cost = {n: w.bvh_cost() for n, w in trees}
        say(f"k = {k:4.1f}: images identical: {same}   depth rebuilt {rebuilt.bvh_info()['max_depth']} created {fresh.bvh_info()['max_depth']}")
        for (n, w), v in zip(trees, tt):
            say(f"    {n:9s} {fmt(v)}   / created {statistics.median(v) / statistics.median(tt[2]):.3f}   "
                f"node visits {visits[n] / visits['created']:.3f}x   bvh_cost {cost[n]:.4f} ({cost[n] / cost['created']:.3f}x created)")
        say(f"    refitted / rebuilt: time {statistics.median(tt[0]) / statistics.median(tt[1]):.3f}   bvh_cost {cost['refitted'] / cost['rebuilt']:.3f}")
        fresh.close()
    say(f"shader clock over the timed renders: {mhz:.1f} MHz")
    refit.close(), rebuilt.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
