#!/usr/bin/env python3
"""Cost of progressive rendering (rtw_accum_*): the configs[1] frame
(1200x675x500, f64 megakernel) rendered one-shot and as passes of 20 samples
with a resolve after every pass, alternating in one process.

  python tools/accum_bench.py [--repeats 5] [--warmup 2] [--out FILE]
  python tools/accum_bench.py --passes-only      # one progressive frame: the run to put under
                                                 # rocprofv3 --kernel-trace --stats
  python tools/accum_bench.py --kernel-stats CSV # add the fold kernel's bytes/s from that run's
                                                 # kernel stats (no GPU needed for this part)

Frame times are host clocks around work that ends in a device synchronise;
the trace-kernel shares are HIP events (rtw_timer) around each trace launch;
the shader clock is rtw_sclk_probe over the whole timed loop.  The fold
kernel's time comes from a kernel trace of a separate run, its bytes from the
shapes: per pixel 24 B per chunk read, the 24 B sum and the 16 B statistic
read and written.  Compared with the float4-copy rate MI355X reaches, 6.29 TB/s."""
import argparse
import csv
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "raytracinginoneweekend.zig_amd"))
COPY_TBS = 6.29  # measured float4 copy, MI355X


def fold_bytes(npix, n_chunks):
    return npix * (24 * n_chunks + 2 * 24 + 2 * 16)


def kernel_avg_ns(path, name):
    """Average duration (ns) and call count of the kernel whose name contains `name` in a rocprofv3 kernel_stats CSV."""
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            if name in row.get("Name", ""):
                return float(row["AverageNs"]), int(row["Calls"])
    raise SystemExit(f"{path}: no kernel named *{name}*")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1200)
    ap.add_argument("--spp", type=int, default=500)
    ap.add_argument("--pass-spp", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--passes-only", action="store_true")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import rtw_amd as R
    W = args.width
    H = R.image_height(W, 16 / 9)
    npix = W * H
    n_pass = -(-args.spp // args.pass_spp)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    if args.kernel_stats:
        chunks = args.pass_spp // R.DEFAULT_CHUNK
        ns, calls = kernel_avg_ns(args.kernel_stats, "accum_fold_kernel")
        b = fold_bytes(npix, chunks)
        say(f"accum_fold_kernel: {calls} calls, average {ns / 1e3:.2f} us; {b / 1e6:.2f} MB per call "
            f"({W}x{H}, {chunks} chunk(s) per pass) = {b / ns / 1e3:.3f} TB/s = {b / ns / 1e3 / COPY_TBS:.1%} of the "
            f"{COPY_TBS} TB/s float4 copy")
        for k in ("accum_resolve_kernel", "trace_kernel"):
            try:
                ns, calls = kernel_avg_ns(args.kernel_stats, k)
                say(f"{k}: {calls} calls, average {ns / 1e3:.2f} us")
            except SystemExit:
                pass
    else:
        import torch
        from rtw_amd.device import TorchAccumulator, TorchRenderer
        if not torch.cuda.is_available():
            raise SystemExit("accum_bench needs a GPU (there is no CPU path)")
        sph, mats, _ = R.cover_scene(42)
        cam = R.cover_camera(16 / 9)
        p = R.make_params(W, H, args.spp)
        rend = TorchRenderer(sph, mats, 0)
        rgb = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda:0")

        def one_shot(timer=None):
            rend.render(cam, p, out=rgb, timer=timer)

        def new_frame():
            # a fresh accumulator (device allocation + zeroing: outside the timed window, timed on its own)
            a = time.perf_counter()
            ta = TorchAccumulator(rend.scene, p)
            ta._ws = prog_ws[0]
            torch.cuda.synchronize()
            t_create.append((time.perf_counter() - a) * 1e3)
            return ta

        def progressive(ta=None, timers=None):
            ta = ta or new_frame()
            for i in range(n_pass):
                n = min(args.pass_spp, args.spp - ta.samples())
                ta.render_pass(cam, n, timers[i] if timers else None)
            prog_ws[0] = ta._ws
            return ta

        prog_ws, t_create = [None], []
        if args.passes_only:
            ta = progressive()
            torch.cuda.synchronize()
            ta = progressive()
            torch.cuda.synchronize()
            print(f"ran 2 progressive frames of {n_pass} passes", flush=True)
            return
        for _ in range(max(1, args.warmup)):
            one_shot()
            torch.cuda.synchronize()
            ta = progressive()
            torch.cuda.synchronize()
        # the same bytes, checked where they are timed
        one_shot()
        torch.cuda.synchronize()
        same = bool(torch.equal(rgb, ta.rgb))
        t0 = time.perf_counter()
        one_shot()
        torch.cuda.synchronize()
        est = time.perf_counter() - t0
        side = torch.cuda.Stream()
        clk = R.SclkProbe(side.cuda_stream, max(1.0, 0.9 * 2.1 * est * 1e3 * args.repeats))
        t_one, t_prog, k_one, k_prog = [], [], [], []
        for _ in range(args.repeats):
            tm = R.Timer()
            a = time.perf_counter()
            one_shot(tm)
            torch.cuda.synchronize()
            t_one.append((time.perf_counter() - a) * 1e3)
            k_one.append(tm.elapsed_ms())
            tm.close()
            tms = [R.Timer() for _ in range(n_pass)]
            ta = new_frame()
            a = time.perf_counter()
            progressive(ta, tms)
            torch.cuda.synchronize()
            t_prog.append((time.perf_counter() - a) * 1e3)
            k_prog.append(sum(t.elapsed_ms() for t in tms))
            for t in tms:
                t.close()
            ta.close()
        mhz = clk.read()
        m1, mp = statistics.median(t_one), statistics.median(t_prog)
        say(f"# {W}x{H}x{args.spp} f64 megakernel; one-shot vs {n_pass} passes of {args.pass_spp} samples with a "
            f"resolve per pass; {args.repeats} alternating repeats after {args.warmup} warm-ups, one process")
        say(f"images identical: {same}")
        say(f"shader clock over the timed loop: {mhz:.1f} MHz")
        say(f"one-shot frame ms    : median {m1:.3f}  min {min(t_one):.3f}  max {max(t_one):.3f}  "
            f"(trace kernel {statistics.median(k_one):.3f})")
        say(f"progressive frame ms : median {mp:.3f}  min {min(t_prog):.3f}  max {max(t_prog):.3f}  "
            f"(trace kernels {statistics.median(k_prog):.3f})")
        say(f"progressive / one-shot: {mp / m1:.4f}; overhead per pass {(mp - m1) / n_pass * 1e3:.1f} us "
            f"({(mp - m1):.3f} ms per frame), of which trace kernels "
            f"{(statistics.median(k_prog) - statistics.median(k_one)) / n_pass * 1e3:.1f} us per pass")
        say(f"accumulator creation (allocation + zeroing, per frame, not in the times above): "
            f"median {statistics.median(t_create):.3f} ms")
        say(f"workspace: one-shot {R.workspace_bytes(p) / 1e6:.1f} MB; pass {ta.acc.workspace_bytes(args.pass_spp) / 1e6:.1f} MB "
            f"+ accumulator {npix * 40 / 1e6:.1f} MB")
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
