#!/usr/bin/env python3
"""Cost and worth of temporal accumulation (rtw_hip.h "temporal accumulation",
DESIGN.md §18) on turntables of scene 1 (configs[1]'s scene as a world) and of
the globe + 10k spheres (scene 7, the real map).

  python tools/temporal_bench.py --mode time    [--repeats 7] [--out FILE]
  python tools/temporal_bench.py --mode quality [--frames 16] [--spp 20] [--ref-spp 500] [--width W] [--out FILE]
                                                [--degrees 1,5,0] [--max-history M]
  either mode: [--clamp-gamma G[,G...]] [--clamp-radius R[,R...]]   
               [--mirror]                                           

time: at the scene's own size (1200x675), HIP events around each call, the calls
alternating in one process after a warm-up round, median (min .. max), each
beside its traffic floor at the 6.29 TB/s copy rate; the 20-sample render for
scale; the shader clock (rtw_sclk_probe) noted.  The frame's guides both ways, in
the same run: rtw_world_guides_device, and rtw_world_surface_device over the
frame's hits (equal bytes, checked first), with the animated
frame's total for each.
quality: frames of 20 spp, every sphere centre turned by 1 or 5 degrees per frame
(rtw_orbit.hpp's motion), RMSE of the linear mean against ref-spp frames of the
same positions, for the input, the spatial denoiser alone, temporal alone and
temporal + denoise; the mean history length and the share of pixels without
history per frame; the averaged frames' error split by what the pixel's feature
ray hits first (the sky, the ground, a diffuse, metal or glass primitive); and
the static case (0 degrees) frame by frame.
--clamp-gamma / --clamp-radius add the clamped call (rtw_temporal_clamped_device,
DESIGN.md §20) for every (gamma, radius) of the two lists (radius alone: the
default gamma, 0; gamma alone: radius 1).  time: one row per radius, static and
motion, in the same alternating rounds as rtw_temporal_device, each beside its
own floor (the unclamped floor with the 12 B/pixel of the mean read (4 + 2r) / 4
times, the tile's halo rows).  quality: every setting accumulates the same
renders beside the unclamped call in one pass, so all of them share their
inputs and references; the unclamped tables come first, unchanged, then each
setting's summary line and by-class split (with --max-history: the sweep with
the clamp on).
--mirror adds the mirror points (rtw_world_mirror_points_device).
time: the launch beside rtw_world_prev_points_device and beside what a caller
would run without it (rtw_world_prev_points_device + rtw_world_trace_device on
the compacted reflected rays), in the same alternating rounds.  quality: after
the tables above, unchanged, every setting once more with the mirror points as
its prev_p and once with the predictor alone, over the same renders; the metal
class split by the material's fuzz, and the share of the metal pixels whose
taps were all refused (no history)."""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "raytracinginoneweekend.zig_amd"))

COPY_RATE = 6.29e12  # bytes/s: the measured device copy rate floors are stated at


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("time", "quality"), required=True)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--spp", type=int, default=20)
    ap.add_argument("--ref-spp", type=int, default=500)
    ap.add_argument("--width", type=int, default=0)
    ap.add_argument("--scenes", default="1,7")
    ap.add_argument("--degrees", default="1,5,0", help="quality: degrees per frame, one turntable each (0: the static case)")
    ap.add_argument("--max-history", type=int, default=0, help="quality: rtw_temporal_opts.max_history (0 = the default)")
    ap.add_argument("--clamp-gamma", default="", help="rtw_temporal_clamp.gamma, a list (0 = the default)")
    ap.add_argument("--clamp-radius", default="", help="rtw_temporal_clamp.radius, a list (1..3)")
    ap.add_argument("--mirror", action="store_true", help="add the mirror points (DESIGN.md §21)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch

    import rtw_amd as R
    from rtw_amd import world as Wd
    from rtw_amd.device import TemporalAccumulator, update_world
    if not torch.cuda.is_available():
        raise SystemExit("temporal_bench needs a GPU (there is no CPU path)")
    dev = "cuda:0"
    lines = []
    gammas = [float(x) for x in args.clamp_gamma.split(",") if x]
    radii = [int(x) for x in args.clamp_radius.split(",") if x]
    if gammas or radii:
        gammas, radii = gammas or [0.0], radii or [1]

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def fmt(v):
        return f"median {statistics.median(v):8.4f}  ({min(v):.4f} .. {max(v):.4f})"

    def stream():
        return torch.cuda.current_stream().cuda_stream

    def turned(a0, kinds, xv0, ops, deg):
        """rtw_orbit.hpp's numbers: sphere centres about the y axis, RotateY angles advanced."""
        phi = np.deg2rad(deg)
        sn, cs = np.sin(phi), np.cos(phi)
        a = a0.copy()
        sph = kinds <= 1
        for e in (0, 3):
            x, z = a0[sph, e], a0[sph, e + 2]
            a[sph, e], a[sph, e + 2] = cs * x + sn * z, -sn * x + cs * z
        xv = xv0.copy()
        rot = ops == 1
        t = xv0[..., 2] + phi
        xv[..., 0] = np.where(rot, np.sin(t), xv0[..., 0])
        xv[..., 1] = np.where(rot, np.cos(t), xv0[..., 1])
        xv[..., 2] = np.where(rot, t, xv0[..., 2])
        return a, xv

    class Scene:
        def __init__(self, sid):
            self.sid = sid
            self.b = Wd.BuiltScene(sid, 42, image=Wd.earth_map() if sid in (4, 7) else None)
            d = self.b.desc
            s = self.b.settings
            self.W = args.width or s.width
            self.H = R.image_height(self.W, s.aspect) if args.width else s.height
            self.cam = self.b.camera()
            self.a0, self.xv0 = Wd.desc_numbers(d)
            self.kinds = np.array([d.prims[i].kind for i in range(d.n_prims)])
            self.ops = np.array([[d.xforms[i].op[k] if k < d.xforms[i].n else 0 for k in range(4)] for i in range(d.n_xforms)],
                                dtype=np.int64).reshape(d.n_xforms, 4)
            # the class of a pixel's first-hit primitive (index = guide prim, 0 = a miss): a sphere of radius >= 100
            # is the ground, everything else goes by its material's kind
            big = (self.kinds <= 1) & (self.a0[:, 6] >= 100.0)
            mk = np.array([d.mats[d.prims[i].mat].kind for i in range(d.n_prims)])
            self.cls = torch.from_numpy(np.concatenate([[0], np.where(big, 1, 2 + mk)]).astype(np.int64)).to(dev)
            # a metal primitive's fuzz bin (index = guide prim): 1: < 0.05, 2: < 0.25, 3: the rest; 0: no metal
            fz = np.array([d.mats[d.prims[i].mat].fuzz for i in range(d.n_prims)])
            self.fuzz_bin = torch.from_numpy(np.concatenate([[0], np.where(mk == 1, 1 + (fz >= 0.05) + (fz >= 0.25), 0)])
                                             .astype(np.int64)).to(dev)
            self.dw = Wd.DeviceWorld(d, dynamic=True)
            self.n = self.W * self.H
            W, H = self.W, self.H
            self.rays = torch.empty((self.n, 9), dtype=torch.float64, device=dev)
            self.hits = torch.empty((self.n, 10), dtype=torch.float64, device=dev)
            self.guides = torch.empty((H, W, 32), dtype=torch.uint8, device=dev)
            self.pp = torch.empty((H, W, 3), dtype=torch.float64, device=dev)
            self.rgb = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
            self.mean = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
            self._ws = None
            self.dn_opts = R.denoise_opts(flags=R.DENOISE_SPATIAL_VAR)
            nb = R.denoise_workspace_bytes(W, H, self.dn_opts)
            self.dn_ws = torch.empty(nb + 256, dtype=torch.uint8, device=dev)
            self.dn_ptr, self.dn_bytes = (self.dn_ws.data_ptr() + 255) & ~255, nb

        def params(self, spp, seed):
            return R.make_params(self.W, self.H, spp, 50, seed, background=self.b.background)

        def numbers(self, deg):
            a, xv = turned(self.a0, self.kinds, self.xv0, self.ops, deg)
            return torch.from_numpy(a).to(dev), (torch.from_numpy(xv).to(dev) if xv.size else None)

        def render(self, p, timer=None):
            need = self.dw.workspace_bytes(p)
            if self._ws is None or self._ws.numel() < need + 256:
                self._ws = torch.empty(need + 256, dtype=torch.uint8, device=dev)
            ptr = (self._ws.data_ptr() + 255) & ~255
            self.dw.render_async(self.cam, p, ptr, need, self.rgb.data_ptr(), self.mean.data_ptr(), stream(), timer)

        def pixel_rays(self):
            R.pixel_rays_device(self.cam, self.W, self.H, self.rays.data_ptr(), stream())

        def trace(self):
            self.dw.trace(self.rays.data_ptr(), self.n, self.hits.data_ptr(), None, stream())

        def make_guides(self, p):
            self.dw.guides(self.cam, p, self.guides.data_ptr(), stream())

        def surface_guides(self):
            """The same guides read off the frame's hits (rtw_world_surface_device)."""
            self.dw.surface(self.hits.data_ptr(), self.n, None, self.guides.data_ptr(), self.b.background, stream())

        def prev_points(self, a_prev, xv_prev):
            self.dw.prev_points_device(self.hits.data_ptr(), self.n, 0.5, self.pp.data_ptr(), a_prev.data_ptr(),
                                       xv_prev.data_ptr() if xv_prev is not None else None, stream())

        def mirror_points(self, a_prev, xv_prev, out, opts=None):
            self.dw.mirror_points_device(self.rays.data_ptr(), self.hits.data_ptr(), self.n, self.cam, out.data_ptr(),
                                         a_prev.data_ptr(), xv_prev.data_ptr() if xv_prev is not None else None, opts, None,
                                         stream())

        def denoise(self, mean, var):
            out = torch.empty_like(mean)
            R.denoise_device(mean.data_ptr(), var.data_ptr() if var is not None else None, self.guides.data_ptr(), self.W,
                             self.H, self.dn_opts, self.dn_ptr, self.dn_bytes, None, out.data_ptr(), stream())
            return out

        def close(self):
            self.dw.close()

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        f()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def mode_time():
        for sid in [int(x) for x in args.scenes.split(",")]:
            sc = Scene(sid)
            W, H, n = sc.W, sc.H, sc.n
            p = sc.params(args.spp, 42)
            a_prev, xv_prev = sc.numbers(0.0)
            a_now, xv_now = sc.numbers(1.0)
            update_world(sc.dw, a_now, xv_now)
            hist = [torch.zeros((H, W, 32), dtype=torch.uint8, device=dev) for _ in range(2)]
            acc, var = torch.empty((H, W, 3), dtype=torch.float32, device=dev), torch.empty((H, W), dtype=torch.float32, device=dev)

            def temporal(src, dst, pp):
                R.temporal_device(sc.mean.data_ptr(), sc.guides.data_ptr(), pp, sc.cam, sc.cam, src, W, H, dst, acc.data_ptr(),
                                  var.data_ptr(), None, stream())

            def clamped(src, dst, pp, r):
                R.temporal_clamped_device(sc.mean.data_ptr(), sc.guides.data_ptr(), pp, sc.cam, sc.cam, src, W, H, dst,
                                          acc.data_ptr(), var.data_ptr(), None, R.temporal_clamp(gammas[0], r), stream())
            sc.render(p)
            sc.pixel_rays(), sc.trace(), sc.make_guides(p), sc.prev_points(a_prev, xv_prev)
            temporal(None, hist[0].data_ptr(), None)  # a first frame: every record holds history from here on
            torch.cuda.synchronize()
            kernel_guides = sc.guides.clone()  # both ways to the guides give the same bytes: checked before either is timed
            sc.guides.fill_(0xA5)
            sc.surface_guides()
            torch.cuda.synchronize()
            if not torch.equal(kernel_guides, sc.guides):
                raise SystemExit(f"scene {sid}: rtw_world_surface_device's guides differ from rtw_world_guides_device's")
            steps = {
                "render (20 spp, all kernels)": lambda: sc.render(p),
                "rtw_pixel_rays_device": sc.pixel_rays,
                "rtw_world_trace_device": sc.trace,
                "rtw_world_guides_device": lambda: sc.make_guides(p),
                "rtw_world_surface_device (guides)": sc.surface_guides,
                "rtw_world_prev_points_device": lambda: sc.prev_points(a_prev, xv_prev),
                "rtw_temporal_device, static": lambda: temporal(hist[0].data_ptr(), hist[1].data_ptr(), None),
                "rtw_temporal_device, motion": lambda: temporal(hist[0].data_ptr(), hist[1].data_ptr(), sc.pp.data_ptr()),
                "rtw_denoise_device (+ spatial)": lambda: sc.denoise(acc, var),
            }
            floors = {"rtw_pixel_rays_device": 72, "rtw_world_prev_points_device": 80 + 24, "rtw_world_surface_device (guides)": 80 + 32,
                      "rtw_temporal_device, static": 12 + 32 + 32 + 48, "rtw_temporal_device, motion": 12 + 32 + 24 + 4 * 32 + 48}
            if args.mirror:  # the fused launch, and what a caller would run without it
                torch.cuda.synchronize()
                h_rays = sc.rays.cpu().numpy().reshape(-1).view(R.RAY_DTYPE)
                h_hits = sc.hits.cpu().numpy().reshape(-1).view(R.HIT_DTYPE)
                rays2, flag = Wd.mirror_rays_host(sc.b.desc, h_rays, h_hits)
                n_mirror = int(flag.sum())
                d_r2 = torch.from_numpy(np.ascontiguousarray(rays2[flag != 0]).view(np.float64).reshape(-1, 9)).to(dev)
                d_h2 = torch.empty((max(1, n_mirror), 10), dtype=torch.float64, device=dev)
                pp_m = torch.empty_like(sc.pp)

                def unfused():
                    sc.prev_points(a_prev, xv_prev)
                    if n_mirror:
                        sc.dw.trace(d_r2.data_ptr(), n_mirror, d_h2.data_ptr(), None, stream())
                steps["rtw_world_mirror_points_device"] = lambda: sc.mirror_points(a_prev, xv_prev, pp_m)
                steps["prev_points + trace (compacted)"] = unfused
                floors["rtw_world_mirror_points_device"] = 72 + 80 + 24
            for r in radii:  # the clamped call beside the unclamped one, in the same rounds
                steps[f"clamped r={r}, static"] = lambda r=r: clamped(hist[0].data_ptr(), hist[1].data_ptr(), None, r)
                steps[f"clamped r={r}, motion"] = lambda r=r: clamped(hist[0].data_ptr(), hist[1].data_ptr(), sc.pp.data_ptr(), r)
                halo = 12 * (4 + 2 * r) // 4 - 12
                floors[f"clamped r={r}, static"] = floors["rtw_temporal_device, static"] + halo
                floors[f"clamped r={r}, motion"] = floors["rtw_temporal_device, motion"] + halo
            t = {k: [] for k in steps}
            trace_ms = []
            est = timed(lambda: sc.render(p))
            clk_stream = torch.cuda.Stream()
            clk = R.SclkProbe(clk_stream.cuda_stream, max(1.0, 1.5 * est * (args.repeats + 1)))
            for r in range(args.repeats + 1):
                for k, f in steps.items():
                    if k.startswith("render"):
                        tm = R.Timer()
                        ms = timed(lambda: sc.render(p, tm))
                        if r:
                            trace_ms.append(tm.elapsed_ms())
                        tm.close()
                    else:
                        ms = timed(f)
                    if r:  # (round 0 warms up)
                        t[k].append(ms)
            mhz = clk.read()
            lens = hist[1].cpu().numpy().reshape(-1).view(R.HISTORY_DTYPE)["len"]
            say(f"# scene {sid}: {sc.b.desc.n_prims} primitives, {W}x{H} = {n} pixels, every sphere centre turned by 1 degree; "
                f"{args.repeats} alternating rounds after one warm-up, HIP-event ms; shader clock {mhz:.1f} MHz")
            say(f"  (motion step: {float((lens > 1).mean()) * 100:.2f} % of the pixels found history)")
            for k, v in t.items():
                fl = f"   floor {floors[k] * n / COPY_RATE * 1e3:.4f} ms ({floors[k]} B/pixel at 6.29 TB/s): x{statistics.median(v) / (floors[k] * n / COPY_RATE * 1e3):.1f}" if k in floors else ""
                say(f"  {k:32s} {fmt(v)}{fl}")
            say(f"  {'  of which the trace kernel':32s} {fmt(trace_ms)}")
            for r in radii:
                for what in ("static", "motion"):
                    c, u = statistics.median(t[f"clamped r={r}, {what}"]), statistics.median(t[f"rtw_temporal_device, {what}"])
                    say(f"  rtw_temporal_clamped_device r={r} (gamma {gammas[0]:g}), {what}: {c:.4f} ms = x{c / u:.2f} of rtw_temporal_device's {u:.4f} ms")
            med = {k: statistics.median(v) for k, v in t.items()}
            extra = sum(med[k] for k in ("rtw_pixel_rays_device", "rtw_world_trace_device", "rtw_world_guides_device",
                                         "rtw_world_prev_points_device", "rtw_temporal_device, motion"))
            rend = med["render (20 spp, all kernels)"]
            say(f"  per animated frame: render {rend:.3f} ms + temporal steps {extra:.3f} ms (+ {extra / rend * 100:.1f} %), of which the "
                f"guides {med['rtw_world_guides_device']:.3f} ms = {med['rtw_world_guides_device'] / (rend + extra) * 100:.1f} % of the frame; "
                f"without the guides the steps are {extra - med['rtw_world_guides_device']:.3f} ms (+ {(extra - med['rtw_world_guides_device']) / rend * 100:.1f} %); "
                f"the denoiser adds {med['rtw_denoise_device (+ spatial)']:.3f} ms")
            # the guides read off the hits the frame already has (pixel rays and trace are in `extra` either way)
            g_old, g_new = med["rtw_world_guides_device"], med["rtw_world_surface_device (guides)"]
            new_extra = extra - g_old + g_new
            say(f"  guides off the frame's hits (rtw_world_surface_device) {g_new:.4f} ms against rtw_world_guides_device {g_old:.4f} ms "
                f"in this run (x{g_old / g_new:.1f}); per animated frame {rend + extra:.3f} ms -> {rend + new_extra:.3f} ms "
                f"(temporal steps {extra:.3f} -> {new_extra:.3f} ms, + {new_extra / rend * 100:.1f} % of the render); a caller with no hits "
                f"yet pays pixel rays + trace + surface = "
                f"{med['rtw_pixel_rays_device'] + med['rtw_world_trace_device'] + g_new:.4f} ms for a frame's guides")
            if args.mirror:
                m_new, m_pp, m_un = (med[k] for k in ("rtw_world_mirror_points_device", "rtw_world_prev_points_device",
                                                       "prev_points + trace (compacted)"))
                say(f"  mirror points: {n_mirror} of {n} records are mirrors ({n_mirror / n * 100:.2f} %); the launch {m_new:.4f} ms = "
                    f"x{m_new / m_pp:.1f} of rtw_world_prev_points_device's {m_pp:.4f} ms, x{m_new / m_un:.2f} of prev_points + "
                    f"rtw_world_trace_device on the {n_mirror} compacted reflected rays ({m_un:.4f} ms; the compaction and "
                    f"rtw_world_mirror_points_host's arithmetic are not in that figure); per animated frame "
                    f"{rend + new_extra:.3f} ms -> {rend + new_extra - m_pp + m_new:.3f} ms")
            sc.close()

    CLASSES = ("miss (the sky)", "ground (r >= 100)", "diffuse", "metal", "glass", "light")

    def rmse(a, b):
        return float(torch.sqrt(((a.double() - b.double()) ** 2).mean()))

    def mode_quality():
        for sid in [int(x) for x in args.scenes.split(",")]:
            sc = Scene(sid)
            W, H = sc.W, sc.H
            say(f"# scene {sid}: {W}x{H}, {args.spp} spp per frame (seed 42 + k), reference {args.ref_spp} spp (seed 1000 + k), "
                f"RMSE of the linear mean over all pixels and channels; max_history {args.max_history or 32}, depth_tol 0.02, min_len_var 4")
            variants = [("unclamped", None)] + [(f"clamp gamma {g:g} radius {r}", R.temporal_clamp(g, r)) for r in radii for g in gammas]
            source = ["surface"] * len(variants)  # what each variant takes as prev_p
            if args.mirror:
                base = list(variants)
                for how, word in (("mirror", "mirror points"), ("predict", "mirror points, predictor only")):
                    variants += [(f"{label} + {word}", c) for label, c in base]
                    source += [how] * len(base)
            FUZZ = ("metal, fuzz < 0.05", "metal, fuzz < 0.25", "metal, fuzz <= 0.5")
            for deg in [float(x) for x in args.degrees.split(",")]:
                frames = args.frames if deg else 2 * args.frames
                tas = [TemporalAccumulator(W, H, R.temporal_opts(max_history=args.max_history), device=0, clamp=c) for _, c in variants]
                prev = None
                rows = [[] for _ in variants]
                # per variant and class: pixels, squared error of the input, of temporal, sum of len
                by_class = np.zeros((len(variants), len(CLASSES), 4))
                by_fuzz = np.zeros((len(variants), 3, 4))  # pixels, squared error of the input, of temporal, pixels without history
                pps = {"surface": None}
                ref0 = None
                for k in range(frames):
                    a, xv = sc.numbers(k * deg)
                    if deg or k == 0:
                        update_world(sc.dw, a, xv)
                    if deg or ref0 is None:
                        sc.render(sc.params(args.ref_spp, 1000 + k))
                        ref = sc.mean.clone()
                        ref0 = ref
                    else:
                        ref = ref0
                    p = sc.params(args.spp, 42 + k)
                    sc.render(p)
                    cur = sc.mean.clone()
                    sc.pixel_rays(), sc.trace(), sc.make_guides(p)
                    pp = None
                    if k and deg:
                        sc.prev_points(*prev)
                        pp = sc.pp
                        if args.mirror:
                            for how, o in (("mirror", None), ("predict", R.mirror_opts(flags=R.MIRROR_PREDICT_ONLY))):
                                if pps.get(how) is None:
                                    pps[how] = torch.empty_like(sc.pp)
                                sc.mirror_points(*prev, pps[how], o)
                    spatial = sc.denoise(cur, None)
                    cls = sc.cls[sc.guides.view(torch.int32)[..., 7].long()]
                    for v, ta in enumerate(tas):  # every variant accumulates the same renders
                        acc, var = ta.step(cur, sc.guides, sc.cam, pp if pp is None or source[v] == "surface" else pps[source[v]])
                        both = sc.denoise(acc, var)
                        torch.cuda.synchronize()
                        if k >= frames // 2:  # the frames the summary line averages, split by what the pixel shows
                            for c in range(len(CLASSES)):
                                m = cls == c
                                by_class[v, c] += np.array([float(m.sum()), float(((cur.double() - ref.double()) ** 2)[m].sum()),
                                                            float(((acc.double() - ref.double()) ** 2)[m].sum()),
                                                            float(ta.history().view(torch.float32)[..., 3][m].sum())])
                            if args.mirror:
                                fb = sc.fuzz_bin[sc.guides.view(torch.int32)[..., 7].long()]
                                lens = ta.history().view(torch.float32)[..., 3]
                                for b in range(3):
                                    m = fb == b + 1
                                    by_fuzz[v, b] += np.array([float(m.sum()), float(((cur.double() - ref.double()) ** 2)[m].sum()),
                                                               float(((acc.double() - ref.double()) ** 2)[m].sum()),
                                                               float((lens[m] == 1).sum())])
                        hist = ta.history().cpu().numpy().reshape(-1).view(R.HISTORY_DTYPE)
                        rows[v].append((k, rmse(cur, ref), rmse(spatial, ref), rmse(acc, ref), rmse(both, ref), float(hist["len"].mean()),
                                        float((hist["len"] == 1).mean()), float((var.cpu().numpy() < 0).mean())))
                    prev = (a, xv)
                say(f"## {deg:g} degrees per frame, {frames} frames")
                for v, (label, _) in enumerate(variants):
                    if v == 0:
                        say("  frame   input   denoise+spatial   temporal   temporal+denoise   mean len   no history   var unknown")
                        for r in rows[0]:
                            say(f"  {r[0]:5d}  {r[1]:.5f}       {r[2]:.5f}       {r[3]:.5f}       {r[4]:.5f}       {r[5]:7.3f}    {r[6] * 100:6.2f} %    {r[7] * 100:6.2f} %")
                    else:
                        say(f"### {label} ({deg:g} degrees per frame)")
                    tail = rows[v][len(rows[v]) // 2:]
                    m = [statistics.mean(r[i] for r in tail) for i in range(1, 5)]
                    say(f"  mean over the last {len(tail)} frames: input {m[0]:.5f}  denoise+spatial {m[1]:.5f} ({m[1] / m[0]:.3f}x)  "
                        f"temporal {m[2]:.5f} ({m[2] / m[0]:.3f}x)  temporal+denoise {m[3]:.5f} ({m[3] / m[0]:.3f}x)")
                    say("  the same frames by what the pixel's feature ray hits first (RMSE over the class's pixels; share of the temporal "
                        "image's squared error):")
                    for c, name in enumerate(CLASSES):
                        n, se_in, se_t, ln = by_class[v, c]
                        if n:
                            say(f"    {name:22s} {n / by_class[v, :, 0].sum() * 100:6.2f} % of the pixels   input {np.sqrt(se_in / n / 3):.5f}   "
                                f"temporal {np.sqrt(se_t / n / 3):.5f} ({np.sqrt(se_t / se_in):.3f}x)   {se_t / by_class[v, :, 2].sum() * 100:6.2f} % "
                                f"of the error   mean len {ln / n:6.2f}")
                    if args.mirror:
                        for b, name in enumerate(FUZZ):
                            n, se_in, se_t, lost = by_fuzz[v, b]
                            if n:
                                say(f"    {name:22s} {n / by_class[v, :, 0].sum() * 100:6.2f} % of the pixels   input {np.sqrt(se_in / n / 3):.5f}   "
                                    f"temporal {np.sqrt(se_t / n / 3):.5f} ({np.sqrt(se_t / se_in):.3f}x)   {lost / n * 100:6.2f} % without history")
                    if not deg:
                        for frac in (0.5, 0.25):
                            hit = next((r[0] + 1 for r in rows[v] if r[3] <= frac * rows[v][0][1]), None)
                            say(f"  static: temporal alone reaches {frac:g} x the input's RMSE after {hit} frames (1 / sqrt(n) says {round(1 / frac ** 2)})")
            sc.close()

    (mode_time if args.mode == "time" else mode_quality)()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
