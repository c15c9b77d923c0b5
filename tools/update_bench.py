#!/usr/bin/env python3
"""Cost of a dynamic world's update (rtw_world_update / rtw_world_update_device,
DESIGN.md §16) next to the only way to move a world without it: rtw_world_create
of the updated description.

  python tools/update_bench.py [--repeats 5] [--spp 100] [--out FILE]

On the globe + 10k spheres (scene 7, the real map, BASELINE configs[4]:
1200x675) and on the Cornell box (scene 6, no BVH):
  * update, host-array entry (copy of the arrays, validation, readback, commit);
  * update, device-array entry from a torch tensor (no host round trip);
  * rtw_world_create + rtw_world_destroy of the same description (host validation,
    SAH build, pack, hipMalloc, upload);
each as host wall time around the call and a device synchronise, the three
alternating in one process for --repeats rounds after a warm-up round; median
(min .. max).  On the globe, for displacements of every small sphere by 0, 0.1,
0.5, 2 and 8 of its radii (a seeded direction in the xz plane): the render time
of the frame on the refitted tree next to that on a freshly built tree of the
same description (HIP-event kernel time, alternating, the same repeats), the
images compared byte for byte, and the node visits of both.  The shader clock is
rtw_sclk_probe over the timed renders."""
import argparse
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
    args = ap.parse_args()
    import ctypes as C

    import numpy as np
    import torch

    import rtw_amd as R
    from rtw_amd import world as Wd
    from rtw_amd.device import update_world
    from update_helpers import prims_with, truncated, xforms_with
    if not torch.cuda.is_available():
        raise SystemExit("update_bench needs a GPU (there is no CPU path)")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def fmt(v):
        return f"median {statistics.median(v):9.3f}  ({min(v):.3f} .. {max(v):.3f})"

    def sync():  # (the render stream alone: a device-wide wait would wait for the clock probe's wave too)
        torch.cuda.current_stream().synchronize()

    def wall(f):
        sync()
        t0 = time.perf_counter()
        r = f()
        sync()
        return (time.perf_counter() - t0) * 1e3, r

    def desc_with(b, a, xv):
        d = truncated(Wd, b.desc, b.desc.n_prims)
        keep = (prims_with(Wd, b.desc, a), xforms_with(Wd, b.desc, xv))
        d.prims, d.xforms = C.cast(keep[0], C.POINTER(Wd.Prim)), C.cast(keep[1], C.POINTER(Wd.Xform))
        return d, keep

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

    clk_stream = torch.cuda.Stream()
    for scene, label in ((7, "globe + 10k spheres (scene 7)"), (6, "Cornell box (scene 6, no BVH)")):
        b = Wd.BuiltScene(scene, 42, image=Wd.earth_map() if scene == 7 else None)
        a0, xv0 = Wd.desc_numbers(b.desc)
        a1 = moved(a0, 0.5) if scene == 7 else a0
        xv1 = xv0.copy()
        if scene == 6:  # the inner boxes turn by 0.2 rad
            for i in range(b.desc.n_xforms):
                for k in range(b.desc.xforms[i].n):
                    if b.desc.xforms[i].op[k] == Wd.XF_ROTATE_Y:
                        t = xv0[i, k, 2] + 0.2
                        xv1[i, k] = (np.sin(t), np.cos(t), t)
        d1, keep1 = desc_with(b, a1, xv1)
        dyn = Wd.DeviceWorld(b.desc, dynamic=True)
        ta = torch.from_numpy(a1).cuda()
        tx = torch.from_numpy(xv1).cuda() if len(xv1) else None
        t_host, t_dev, t_create = [], [], []
        for r in range(args.repeats + 1):
            th_, _ = wall(lambda: dyn.update(d1))
            td_, _ = wall(lambda: update_world(dyn, ta, tx))
            tc_, _ = wall(lambda: Wd.DeviceWorld(d1).close())
            if r:  # (round 0 warms up: code objects, allocator)
                t_host.append(th_), t_dev.append(td_), t_create.append(tc_)
        info = dyn.bvh_info()
        say(f"# {label}: {b.desc.n_prims} primitives, {b.desc.n_xforms} transforms, BVH {info['nodes']} nodes, depth {info['max_depth']}; "
            f"{args.repeats} alternating rounds after one warm-up, host wall ms incl. synchronise")
        say(f"update, host arrays     : {fmt(t_host)}")
        say(f"update, device arrays   : {fmt(t_dev)}")
        say(f"rtw_world_create+destroy: {fmt(t_create)}")
        say(f"create / update: host arrays {statistics.median(t_create) / statistics.median(t_host):.1f}x, "
            f"device arrays {statistics.median(t_create) / statistics.median(t_dev):.1f}x")
        if scene != 7:
            dyn.close()
            continue
        s = b.settings
        cam = b.camera()
        p = R.make_params(s.width, s.height, args.spp, 50, 42, background=b.background)
        need = dyn.workspace_bytes(p)
        ws = torch.empty(need + 256, dtype=torch.uint8, device="cuda:0")
        ptr = (ws.data_ptr() + 255) & ~255
        rgb = [torch.empty((s.height, s.width, 3), dtype=torch.uint8, device="cuda:0") for _ in range(2)]

        def frame(dw, out):
            tm = R.Timer()
            dw.render_async(cam, p, ptr, need, out.data_ptr(), None, torch.cuda.current_stream().cuda_stream, tm)
            sync()
            ms = tm.elapsed_ms()
            tm.close()
            return ms
        say(f"# render of {s.width}x{s.height}x{args.spp} (configs[4]) after every small sphere moved by k radii: refitted tree vs "
            f"a freshly built one, kernel ms, {args.repeats} alternating repeats after a warm-up")
        ks = (0.0, 0.1, 0.5, 2.0, 8.0)
        frame(dyn, rgb[0])
        est = frame(dyn, rgb[0])
        clk = R.SclkProbe(clk_stream.cuda_stream, max(1.0, 0.8 * est * 2 * (args.repeats + 1) * len(ks)))
        rows, held = [], []
        for k in ks:
            a = moved(a0, k)
            d, keep = desc_with(b, a, xv0)
            update_world(dyn, torch.from_numpy(a).cuda(), None)
            fresh = Wd.DeviceWorld(d)
            t_ref, t_new = [], []
            for r in range(args.repeats + 1):
                x, y = frame(dyn, rgb[0]), frame(fresh, rgb[1])
                if r:
                    t_ref.append(x), t_new.append(y)
            rows.append((k, t_ref, t_new, bool(torch.equal(rgb[0], rgb[1]))))
            held.append(fresh)  # (freeing device memory waits for the whole device, the probe's wave included)
        mhz = clk.read()
        for w in held:
            w.close()
        for k, t_ref, t_new, same in rows:  # (the counts pass waits for the whole device: after the probe)
            a = moved(a0, k)
            d, keep = desc_with(b, a, xv0)
            update_world(dyn, torch.from_numpy(a).cuda(), None)
            fresh = Wd.DeviceWorld(d)
            cr, cf = dyn.counts(cam, p, ptr, need), fresh.counts(cam, p, ptr, need)
            say(f"k = {k:4.1f}: refit {fmt(t_ref)}   rebuilt {fmt(t_new)}   refit / rebuilt {statistics.median(t_ref) / statistics.median(t_new):.3f}   "
                f"node visits {cr['node_visits'] / cf['node_visits']:.3f}x   images identical: {same}")
            fresh.close()
        say(f"shader clock over the timed renders: {mhz:.1f} MHz")
        dyn.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
