#!/usr/bin/env python3
"""What adaptive sampling (rtw_accum_set_adaptive) is worth in
time: the configs[1] frame (1200x675x500, f64 megakernel) rendered, alternating
in one process,
  (a) one-shot,
  (b) as uniform passes of --pass-spp samples,
  (c) as adaptive passes of --pass-spp samples, with the per-pixel budget `tol`
      set to the frame noise (b) reaches at the full spp.

  python tools/adaptive_bench.py [--repeats 5] [--warmup 1] [--pass-spp 100] [--out FILE]

Frame times are host clocks around work that ends in a device synchronise; (c)
includes its per-pass readback of the active-tile count.  The shader clock is
rtw_sclk_probe over the whole timed loop.  Per pass of (c): the active pixels
and tiles the pass rendered."""
import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "raytracinginoneweekend.zig_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1200)
    ap.add_argument("--spp", type=int, default=500)
    ap.add_argument("--pass-spp", type=int, default=100)
    ap.add_argument("--min-spp", type=int, default=0)
    ap.add_argument("--tol", type=float, default=0.0, help="the budget; default: the noise of (b) at the full spp")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import rtw_amd as R
    from rtw_amd.device import TorchAccumulator, TorchRenderer
    if not torch.cuda.is_available():
        raise SystemExit("adaptive_bench needs a GPU (there is no CPU path)")
    W = args.width
    H = R.image_height(W, 16 / 9)
    npix = W * H
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    sph, mats, _ = R.cover_scene(42)
    cam = R.cover_camera(16 / 9)
    p = R.make_params(W, H, args.spp)
    rend = TorchRenderer(sph, mats, 0)
    rgb = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda:0")
    ws = [None]

    def one_shot():
        rend.render(cam, p, out=rgb)

    def frame(tol, trace=None):
        """A frame in passes; tol > 0: adaptive.  Returns the accumulator (open)."""
        ta = TorchAccumulator(rend.scene, p, workspace=ws[0])  # (the frames share one workspace)
        if tol > 0:
            ta.set_adaptive(tol, args.min_spp)
        while ta.samples() < args.spp:
            if tol > 0:
                act = ta.active()
                if act[0] == 0:
                    break
                if trace is not None:
                    trace.append(act)
            ta.render_pass(cam, min(args.pass_spp, args.spp - ta.samples()))
        ws[0] = ta.workspace(args.pass_spp)
        return ta

    # the budget: what uniform sampling reaches with every sample
    ta = frame(0.0)
    torch.cuda.synchronize()
    noise_b = ta.noise()
    ta.close()
    tol = args.tol or noise_b
    for _ in range(max(1, args.warmup)):
        one_shot()
        torch.cuda.synchronize()
        frame(0.0).close()
        frame(tol).close()
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    one_shot()
    torch.cuda.synchronize()
    est = time.perf_counter() - t0
    side = torch.cuda.Stream()
    clk = R.SclkProbe(side.cuda_stream, max(1.0, 0.9 * 3.5 * est * 1e3 * args.repeats))
    t_a, t_b, t_c = [], [], []
    trace, noise_c, mean_spp, counts = [], None, None, None
    for r in range(args.repeats):
        a = time.perf_counter()
        one_shot()
        torch.cuda.synchronize()
        t_a.append((time.perf_counter() - a) * 1e3)
        a = time.perf_counter()
        tb = frame(0.0)
        torch.cuda.synchronize()
        t_b.append((time.perf_counter() - a) * 1e3)
        tb.close()
        tr = []
        a = time.perf_counter()
        tc = frame(tol, tr)
        torch.cuda.synchronize()
        t_c.append((time.perf_counter() - a) * 1e3)
        if r == args.repeats - 1:
            trace, noise_c, counts = tr, tc.noise(), tc.counts()
            mean_spp = float(counts.mean())
            left = tc.active()
        tc.close()
    mhz = clk.read()
    med = statistics.median
    say(f"# {W}x{H}x{args.spp} f64 megakernel; (a) one-shot, (b) uniform passes of {args.pass_spp}, (c) adaptive passes of "
        f"{args.pass_spp} with tol = {tol:.6g}; {args.repeats} alternating repeats after {args.warmup} warm-up(s), one process")
    say(f"shader clock over the timed loop: {mhz:.1f} MHz")
    for name, t in (("(a) one-shot", t_a), ("(b) uniform ", t_b), ("(c) adaptive", t_c)):
        say(f"{name} frame ms: median {med(t):.3f}  min {min(t):.3f}  max {max(t):.3f}")
    say(f"(c) / (b): {med(t_c) / med(t_b):.4f}   (c) / (a): {med(t_c) / med(t_a):.4f}   (b) / (a): {med(t_b) / med(t_a):.4f}")
    say(f"mean samples per pixel: (a) {args.spp}  (b) {args.spp}  (c) {mean_spp:.2f}")
    say(f"final rtw_accum_noise: (b) {noise_b:.6g}  (c) {noise_c:.6g}   ((a) is (b)'s frame: the same bytes)")
    n_tiles = ((W + 7) // 8) * ((H + 7) // 8)
    for i, (px, tl) in enumerate(trace):
        say(f"(c) pass {i + 1}: {px} active pixels ({px / npix:.1%}) in {tl} of {n_tiles} tiles")
    say(f"(c) after the last pass: {left[0]} active pixels in {left[1]} tiles; passes run: {len(trace)}")
    vals = sorted(set(counts.ravel().tolist()))
    say("(c) pixels per sample count: " + "  ".join(f"{v}: {int((counts == v).sum())}" for v in vals))
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
