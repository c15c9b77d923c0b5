#!/usr/bin/env python3
"""Cost and quality of the feature-guided denoiser (rtw_accum_denoise_device,
DESIGN.md §14) on the configs[1] frame: 1200x675, cover scene, one 20-sample
pass accumulated.

  python tools/denoise_bench.py [--repeats 20] [--warmup 3] [--out FILE] [--no-quality]
  python tools/denoise_bench.py --quality-only --chunk 10   # the quality figures with two chunks in the pass
  python tools/denoise_bench.py --quality-only --spatial    # ... of the single-chunk pass with RTW_DENOISE_SPATIAL_VAR

Times are HIP events around the calls on one stream, alternating the variants
in one process after a warm-up: the resolve alone, the variance alone, and the
denoise entry with 1..5 levels in the product's forms and with every level in
the direct form (RTW_DENOISE_DIRECT), and the spatial variance estimate
(rtw_denoise_spatial_variance_device, §14.6) over the all-unknown map in its
tiled and direct forms, with and without guides.  A level's time is the difference of
consecutive level counts; levels 1 and 2 (tap spacing 1 and 2) are the ones the
product runs through LDS tiles, so their two columns are the A/B of the forms.
Each level is compared with its traffic floor, 48 B read + 16 B written per
pixel at the 6.29 TB/s float4 copy rate (profiles/r07/accum.txt), and the total
with the 5.29 ms trace time of a 20-sample pass from the same file.  The shader
clock is rtw_sclk_probe over the whole timed loop.  Guide passes: the cover
scene and the globe (scene 7), timed the same way.  Quality: RMSE against the
500-spp frame of the 20-spp input, of the unguided 5-level B3 blur of it, and
of the denoised image."""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "raytracinginoneweekend.zig_amd"))
COPY_TBS = 6.29      # measured float4 copy, MI355X (profiles/r07/accum.txt)
PASS_TRACE_MS = 5.29  # trace time of a 20-sample pass (profiles/r07/accum.txt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1200)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ref-spp", type=int, default=500)
    ap.add_argument("--no-quality", action="store_true")
    ap.add_argument("--quality-only", action="store_true", help="skip the timings")
    ap.add_argument("--chunk", type=int, default=0,
                    help="params.chunk of the accumulated pass (0 = the default, 20: one chunk in the 20-sample pass, so "
                         "its variance is unknown and the colour term is dropped; 10 or 5 give 2 or 4 chunks)")
    ap.add_argument("--spatial", action="store_true",
                    help="quality: add the line of the denoise entry with RTW_DENOISE_SPATIAL_VAR (§14.6)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import rtw_amd as R
    from rtw_amd import world as Wd
    from rtw_amd.device import TorchAccumulator, TorchRenderer
    if not torch.cuda.is_available():
        raise SystemExit("denoise_bench needs a GPU (there is no CPU path)")
    W = args.width
    H = R.image_height(W, 16 / 9)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    sph, mats, _ = R.cover_scene(42)
    cam = R.cover_camera(16 / 9)
    rend = TorchRenderer(sph, mats, 0)
    p = R.make_params(W, H, 20, chunk=args.chunk)
    ta = TorchAccumulator(rend.scene, p)
    ta.render_pass(cam, 20)
    guides = ta.guides(cam)
    stream = torch.cuda.current_stream().cuda_stream
    var = torch.empty((H, W), dtype=torch.float32, device="cuda:0")
    need = ta.acc.denoise_workspace_bytes()
    ws = torch.empty(need + 256, dtype=torch.uint8, device="cuda:0")
    ptr = (ws.data_ptr() + 255) & ~255
    rgb = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda:0")
    mean = torch.empty((H, W, 3), dtype=torch.float32, device="cuda:0")

    def denoise(levels, flags=0):
        ta.acc.denoise(guides.data_ptr(), ptr, need, rgb.data_ptr(), mean.data_ptr(),
                       R.denoise_opts(levels=levels, flags=flags), stream)

    if not args.quality_only:
        timings(args, R, Wd, torch, ta, rend, cam, p, guides, var, rgb, mean, stream, denoise, say, W, H)
    if not args.no_quality:
        quality(args, R, np, torch, ta, rend, cam, rgb, mean, stream, denoise, say, W, H)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


def timings(args, R, Wd, torch, ta, rend, cam, p, guides, var, rgb, mean, stream, denoise, say, W, H):
    npix = W * H
    b7 = Wd.BuiltScene(7, 42, image=Wd.earth_map())
    dw7 = Wd.DeviceWorld(b7.desc)
    cam7 = b7.camera(16 / 9)
    p7 = R.make_params(W, H, 1, background=b7.background)
    g7 = torch.empty((H, W, 32), dtype=torch.uint8, device="cuda:0")
    variants = {"resolve": lambda: ta.acc.resolve(rgb.data_ptr(), mean.data_ptr(), stream),
                "variance": lambda: ta.acc.variance(var.data_ptr(), stream),
                "guides cover scene": lambda: rend.scene.guides(cam, p, guides.data_ptr(), stream),
                "guides globe (scene 7)": lambda: dw7.guides(cam7, p7, g7.data_ptr(), stream)}
    ta.acc.resolve(rgb.data_ptr(), mean.data_ptr(), stream)  # (the estimate's input: the resolved mean, no variance)
    est = torch.empty((H, W), dtype=torch.float32, device="cuda:0")

    def spatial(g, flags):
        R.spatial_variance_device(mean.data_ptr(), None, g, W, H, R.denoise_opts(flags=flags), est.data_ptr(), stream)
    variants["spatial variance tiled"] = lambda: spatial(guides.data_ptr(), 0)
    variants["spatial variance direct"] = lambda: spatial(guides.data_ptr(), R.DENOISE_DIRECT)
    variants["spatial variance tiled, no guides"] = lambda: spatial(None, 0)
    variants["spatial variance direct, no guides"] = lambda: spatial(None, R.DENOISE_DIRECT)
    variants["denoise 5 levels spatial"] = lambda: denoise(5, R.DENOISE_SPATIAL_VAR)
    for k in range(1, 6):
        variants[f"denoise {k} levels"] = (lambda k=k: denoise(k))
        variants[f"denoise {k} levels direct"] = (lambda k=k: denoise(k, R.DENOISE_DIRECT))
    for _ in range(max(1, args.warmup)):
        for f in variants.values():
            f()
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for f in variants.values():
        f()
    ev1.record()
    torch.cuda.synchronize()
    est_ms = ev0.elapsed_time(ev1)
    side = torch.cuda.Stream()
    clk = R.SclkProbe(side.cuda_stream, max(1.0, 0.9 * est_ms * args.repeats))
    times = {k: [] for k in variants}
    for _ in range(args.repeats):  # alternating: every variant once per repeat
        for k, f in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
    mhz = clk.read()
    med = {k: statistics.median(v) for k, v in times.items()}
    say(f"# denoiser on {W}x{H} (cover scene, 20 samples accumulated, f64 megakernel); HIP events, "
        f"{args.repeats} alternating repeats after {args.warmup} warm-ups, one process")
    say(f"shader clock over the timed loop: {mhz:.1f} MHz")
    for k in variants:
        say(f"{k:34s}: median {med[k] * 1e3:9.1f} us  min {min(times[k]) * 1e3:9.1f}  max {max(times[k]) * 1e3:9.1f}")
    floor_us = npix * 64 / (COPY_TBS * 1e12) * 1e6
    say(f"traffic floor of a level: {npix * 64 / 1e6:.1f} MB (48 B read + 16 B written per pixel) at {COPY_TBS} TB/s "
        f"= {floor_us:.1f} us")
    base = med["resolve"] + med["variance"]
    prev = {"": base, " direct": base}
    for k in range(1, 6):
        row = []
        for form in ("", " direct"):
            t = med[f"denoise {k} levels{form}"]
            row.append(t - prev[form])
            prev[form] = t
        form_name = "LDS tiles" if k <= 2 else "direct (the product's form too)"
        say(f"level {k} (tap spacing {1 << (k - 1):2d}): product form [{form_name}] {row[0] * 1e3:7.1f} us = "
            f"{row[0] * 1e3 / floor_us:5.1f} x floor;  direct form {row[1] * 1e3:7.1f} us = {row[1] * 1e3 / floor_us:5.1f} x floor")
    total = med["denoise 5 levels"]
    say(f"total (resolve + variance + 5 levels): {total:.3f} ms = {total / PASS_TRACE_MS:.1%} of the {PASS_TRACE_MS} ms "
        f"trace time of a 20-sample pass; all-direct {med['denoise 5 levels direct']:.3f} ms")
    level = (med["denoise 5 levels"] - base) / 5
    ts, td = med["spatial variance tiled"], med["spatial variance direct"]
    say(f"spatial variance estimate (7x7, every pixel unknown): tiled {ts * 1e3:.1f} us = {ts / level:.2f} mean levels, "
        f"direct {td * 1e3:.1f} us = {td / level:.2f} mean levels (a mean level: {level * 1e3:.1f} us); the flagged "
        f"5-level entry {med['denoise 5 levels spatial']:.3f} ms = unflagged + {(med['denoise 5 levels spatial'] - total) * 1e3:.1f} us")


def quality(args, R, np, torch, ta, rend, cam, rgb, mean, stream, denoise, say, W, H):
    ref = torch.empty((H, W, 3), dtype=torch.float32, device="cuda:0")
    rend.render(cam, R.make_params(W, H, args.ref_spp), out=rgb, mean=ref)
    ta.acc.resolve(rgb.data_ptr(), mean.data_ptr(), stream)
    noisy = mean.cpu().numpy().astype(np.float64)
    denoise(5)
    torch.cuda.synchronize()
    den = mean.cpu().numpy().astype(np.float64)
    refh = ref.cpu().numpy().astype(np.float64)
    blur = R.denoise_host(noisy.astype(np.float32), None, None)[1].astype(np.float64)  # no variance, no guides

    def rmse(a):
        return float(np.sqrt(np.mean((a - refh) ** 2)))
    e_in, e_blur, e_den = rmse(noisy), rmse(blur), rmse(den)
    m = 20 // (args.chunk or R.DEFAULT_CHUNK)
    say(f"quality, chunk {args.chunk or R.DEFAULT_CHUNK} ({m} full chunk(s): variance {'known' if m >= 2 else 'unknown, no colour term'}), "
        f"against the {args.ref_spp}-spp frame (RMSE of the linear mean): input 20 spp {e_in:.5f}, unguided "
        f"5-level B3 blur {e_blur:.5f}, denoised {e_den:.5f} = {e_den / e_in:.3f} x input, {e_den / e_blur:.3f} x blur")
    if args.spatial:
        denoise(5, R.DENOISE_SPATIAL_VAR)
        torch.cuda.synchronize()
        e_sp = rmse(mean.cpu().numpy().astype(np.float64))
        say(f"quality with RTW_DENOISE_SPATIAL_VAR (variances below two chunks estimated from the image): denoised "
            f"{e_sp:.5f} = {e_sp / e_in:.3f} x input, {e_sp / e_den:.3f} x the unflagged call")


if __name__ == "__main__":
    main()
