#!/usr/bin/env python3
"""Cost of the surface queries (rtw_hip.h "surface queries"): one
rtw_world_surface_device launch over the first hits of a frame's feature rays
(coherent records: neighbouring lanes read neighbouring table entries) and over
the hits of one bounce off them (incoherent: every lane its own primitive,
material and texel), with guides only and with both outputs.

  python tools/surface_bench.py [--frames 7:1200x675,1:600x400] [--repeats 7] [--inner 20] [--out FILE]

Per form: HIP events around `inner` back-to-back launches (a single launch is a
few tens of microseconds: mostly the launch itself), the forms alternating in one
process after a warm-up round, median (min .. max) of the per-launch time over the
rounds; beside it the traffic floor at the project's measured 6.29 TB/s copy rate —
80 B read + 32 B written per record for guides only, + 64 B for both outputs (the
tables stay in cache and are left out).  The outputs are compared with
rtw_world_guides_device's buffer before anything is timed.  The shader clock
(rtw_sclk_probe) over the timed window is noted."""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "raytracinginoneweekend.zig_amd"))

COPY_RATE = 6.29e12  # bytes/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="7:1200x675,1:600x400", help="scene:WxH, comma separated")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20, help="launches per timed window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import rtw_amd as R
    from rtw_amd import world as Wd
    if not torch.cuda.is_available():
        raise SystemExit("surface_bench needs a GPU (there is no CPU path)")
    dev = "cuda:0"
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def stream():
        return torch.cuda.current_stream().cuda_stream

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.inner):
            f()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / args.inner

    for spec in args.frames.split(","):
        sid, size = spec.split(":")
        sid, (W, H) = int(sid), (int(x) for x in size.split("x"))
        b = Wd.BuiltScene(sid, 42, image=Wd.earth_map() if sid in (4, 7) else None)
        cam = b.camera(W / H)
        dw = Wd.DeviceWorld(b.desc)
        n = W * H
        rays = torch.empty((n, 9), dtype=torch.float64, device=dev)
        hits = torch.empty((n, 10), dtype=torch.float64, device=dev)
        R.pixel_rays_device(cam, W, H, rays.data_ptr(), stream())
        dw.trace(rays.data_ptr(), n, hits.data_ptr(), None, stream())
        # one bounce: reflected about the normal, from p
        hit = hits.view(torch.int32)[:, 18] != 0
        d, nrm = rays[hit, 3:6], hits[hit, 4:7]
        m = int(hit.sum())
        rays2 = torch.empty((m, 9), dtype=torch.float64, device=dev)
        rays2[:, 0:3], rays2[:, 3:6] = hits[hit, 1:4], d - 2.0 * (d * nrm).sum(dim=1, keepdim=True) * nrm
        rays2[:, 6], rays2[:, 7], rays2[:, 8] = rays[hit, 6], 0.001, float("inf")
        hits2 = torch.empty((m, 10), dtype=torch.float64, device=dev)
        dw.trace(rays2.data_ptr(), m, hits2.data_ptr(), None, stream())
        surf = torch.empty((n, 64), dtype=torch.uint8, device=dev)
        guides = torch.empty((n, 32), dtype=torch.uint8, device=dev)
        # what is timed is right: the guides are the guide kernel's
        ref = torch.empty((n, 32), dtype=torch.uint8, device=dev)
        dw.guides(cam, R.make_params(W, H, 1, background=b.background), ref.data_ptr(), stream())
        dw.surface(hits.data_ptr(), n, surf.data_ptr(), guides.data_ptr(), b.background, stream())
        torch.cuda.synchronize()
        if not torch.equal(ref, guides):
            raise SystemExit(f"scene {sid}: the guides differ from rtw_world_guides_device's")
        hit2 = float((hits2.view(torch.int32)[:, 18] != 0).float().mean())

        def form(h, k, both):
            return lambda: dw.surface(h.data_ptr(), k, surf.data_ptr() if both else None, guides.data_ptr(), b.background, stream())
        forms = {"frame hits, guides only": (form(hits, n, False), n, 112), "frame hits, both outputs": (form(hits, n, True), n, 176),
                 "bounce hits, guides only": (form(hits2, m, False), m, 112), "bounce hits, both outputs": (form(hits2, m, True), m, 176)}
        t = {k: [] for k in forms}
        est = sum(timed(f) for f, _, _ in forms.values()) * args.inner
        clk_stream = torch.cuda.Stream()
        clk = R.SclkProbe(clk_stream.cuda_stream, max(1.0, 1.5 * est * (args.repeats + 1)))
        for r in range(args.repeats + 1):
            for k, (f, _, _) in forms.items():
                ms = timed(f)
                if r:  # (round 0 warms up)
                    t[k].append(ms)
        mhz = clk.read()
        info = dw.query_info()
        say(f"# scene {sid}: {b.desc.n_prims} primitives ({b.desc.n_textures} textures, {b.desc.n_mats} materials), {W}x{H} = {n} "
            f"feature-ray records ({float(hit.float().mean()) * 100:.1f} % hits), {m} bounce records ({hit2 * 100:.1f} % hits); "
            f"trace walk {info['traversal']}; {args.repeats} alternating rounds of {args.inner} launches after one warm-up, "
            f"HIP-event ms per launch; shader clock {mhz:.1f} MHz")
        for k, v in t.items():
            _, cnt, bytes_ = forms[k]
            floor = bytes_ * cnt / COPY_RATE * 1e3
            med = statistics.median(v)
            say(f"  {k:28s} median {med:8.4f}  ({min(v):.4f} .. {max(v):.4f})   {cnt / med / 1e6:8.1f} G records/s   "
                f"floor {floor:.4f} ms ({bytes_} B/record at 6.29 TB/s): x{med / floor:.1f}")
        dw.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
