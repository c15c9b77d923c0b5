"""Torch-side plumbing for the device-resident API: HBM buffers from torch's
caching allocator, the render launched on torch's current HIP stream.
Torch is plumbing here (device memory, streams, torch.distributed); the
rendering is the HIP kernels of lib/librtw_hip.so."""
from __future__ import annotations

import torch

from . import (Accumulator, Camera, DeviceScene, Params, QueryOpts, TemporalClamp, TemporalOpts, Timer,
               pixel_rays_device, temporal_clamped_device, temporal_device, workspace_bytes)


class TorchRenderer:
    def __init__(self, spheres, mats, device: int | torch.device = 0):
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        if not torch.cuda.is_available():
            raise RuntimeError("no GPU visible: the rtw render path has no CPU fallback")
        torch.cuda.set_device(self.device)
        self.scene = DeviceScene(spheres, mats)  # uploads to the current device
        self._ws = None

    def workspace(self, params: Params) -> torch.Tensor:
        need = workspace_bytes(params)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need + 256, dtype=torch.uint8, device=self.device)
        return self._ws

    def _ws_ptr(self, params: Params):
        ws = self.workspace(params)
        base = ws.data_ptr()
        ptr = (base + 255) & ~255
        return ptr, ws.numel() - (ptr - base)

    def render(self, cam: Camera, params: Params, out: torch.Tensor | None = None,
               mean: torch.Tensor | None = None, timer: Timer | None = None) -> torch.Tensor:
        """Asynchronous on torch.cuda.current_stream(); returns the rgb tensor (rows, W, 3) uint8."""
        if out is None:
            out = torch.empty((params.row_count, params.width, 3), dtype=torch.uint8, device=self.device)
        assert out.is_contiguous() and out.dtype == torch.uint8 and out.numel() == params.row_count * params.width * 3
        if mean is not None:
            assert mean.is_contiguous() and mean.dtype == torch.float32 and mean.numel() == out.numel()
        ptr, nbytes = self._ws_ptr(params)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        self.scene.render_async(cam, params, ptr, nbytes, out.data_ptr(),
                                mean.data_ptr() if mean is not None else None, stream, timer)
        return out

    def counts(self, cam: Camera, params: Params) -> dict:
        ptr, nbytes = self._ws_ptr(params)
        torch.cuda.synchronize(self.device)
        return self.scene.counts(cam, params, ptr, nbytes)

    def stats(self, cam: Camera, params: Params) -> dict:
        ptr, nbytes = self._ws_ptr(params)
        torch.cuda.synchronize(self.device)
        return self.scene.stats(cam, params, ptr, nbytes)


class TorchAccumulator:
    """Progressive rendering on torch's current HIP stream: an Accumulator over
    a DeviceScene or a world.DeviceWorld of the current device, its workspace
    and image tensors from torch's allocator.

        acc = TorchAccumulator(renderer.scene, params)
        for img in acc.passes(cam, 20):     # the rgb tensor after each pass
            ...

    Adaptive sampling (Accumulator): set_mask() / set_adaptive()
    before or between passes; passes() then also stops when no pixel is
    active.  In that state every pass begins with a small synchronising
    readback, and needs the same workspace as an unmasked pass.
    """

    def __init__(self, target, params: Params, device: int | torch.device | None = None,
                 workspace: torch.Tensor | None = None):
        """workspace (optional): a uint8 tensor to render the passes into, for instance another
        accumulator's workspace(); replaced by a larger one when a pass needs more."""
        if not torch.cuda.is_available():
            raise RuntimeError("no GPU visible: the rtw render path has no CPU fallback")
        if device is None:
            device = torch.cuda.current_device()
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        torch.cuda.set_device(self.device)
        self.params = params
        self.acc = Accumulator(target, params)
        self._ws = workspace
        shape = (params.row_count, params.width, 3)
        self.rgb = torch.empty(shape, dtype=torch.uint8, device=self.device)
        self.mean = torch.empty(shape, dtype=torch.float32, device=self.device)

    def _ws_ptr(self, pass_spp: int):
        need = self.acc.workspace_bytes(pass_spp)
        if self._ws is None or self._ws.numel() < need + 256:
            self._ws = torch.empty(need + 256, dtype=torch.uint8, device=self.device)
        base = self._ws.data_ptr()
        ptr = (base + 255) & ~255
        return ptr, self._ws.numel() - (ptr - base)

    def workspace(self, pass_spp: int) -> torch.Tensor:
        """The workspace tensor (uint8) the passes of pass_spp samples render into."""
        self._ws_ptr(pass_spp)
        return self._ws

    def render_pass(self, cam: Camera, pass_spp: int, timer: Timer | None = None) -> torch.Tensor:
        """One pass and its resolve, asynchronous; returns the rgb tensor (rows, W, 3) uint8
        (self.mean holds the f32 mean).  The tensors are reused by the next pass."""
        ptr, nbytes = self._ws_ptr(pass_spp)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        self.acc.render_pass(cam, pass_spp, ptr, nbytes, stream, timer)
        if self.acc.samples() > 0:  # (a masked pass with no active pixel renders nothing)
            self.acc.resolve(self.rgb.data_ptr(), self.mean.data_ptr(), stream)
        return self.rgb

    def passes(self, cam: Camera, pass_spp: int, max_noise: float | None = None):
        """Yield the image after each pass of pass_spp samples (the last one may
        be shorter) until the frame's spp, until noise() <= max_noise, or (with a
        mask or a per-pixel budget) until no pixel is active."""
        while self.acc.samples() < self.params.spp:
            if self.acc.masked and self.acc.active()[0] == 0:
                return
            yield self.render_pass(cam, min(pass_spp, self.params.spp - self.acc.samples()))
            if max_noise is not None and self.acc.samples() >= 2 * self.acc.chunk and self.noise() <= max_noise:
                return

    def guides(self, cam: Camera) -> torch.Tensor:
        """The frame's feature buffers (rtw_guide records as (rows, W, 32) uint8) from the
        accumulator's scene or world, on torch's current stream.  Compute them once per frame."""
        p = self.params
        g = torch.empty((p.row_count, p.width, 32), dtype=torch.uint8, device=self.device)
        self.acc.target.guides(cam, p, g.data_ptr(), torch.cuda.current_stream(self.device).cuda_stream)
        return g

    def denoised(self, guides: torch.Tensor | None = None, opts=None):
        """(rgb uint8, mean f32) tensors of the denoised image of the samples so far
        (rtw_accum_denoise_device), on torch's current stream; `guides` from guides(), or
        None for the variance-guided filter alone.  The accumulator is not modified.
        With opts.flags DENOISE_SPATIAL_VAR a first pass of a single chunk, whose variance the
        accumulator does not know yet, is filtered with a variance estimated from the image."""
        need = self.acc.denoise_workspace_bytes(opts)
        if getattr(self, "_dn_ws", None) is None or self._dn_ws.numel() < need + 256:
            self._dn_ws = torch.empty(need + 256, dtype=torch.uint8, device=self.device)
        base = self._dn_ws.data_ptr()
        ptr = (base + 255) & ~255
        shape = (self.params.row_count, self.params.width, 3)
        rgb = torch.empty(shape, dtype=torch.uint8, device=self.device)
        mean = torch.empty(shape, dtype=torch.float32, device=self.device)
        self.acc.denoise(guides.data_ptr() if guides is not None else None, ptr, self._dn_ws.numel() - (ptr - base),
                         rgb.data_ptr(), mean.data_ptr(), opts, torch.cuda.current_stream(self.device).cuda_stream)
        return rgb, mean

    def noise(self) -> float:
        return self.acc.noise(torch.cuda.current_stream(self.device).cuda_stream)

    def samples(self) -> int:
        return self.acc.samples()

    def set_mask(self, mask):
        self.acc.set_mask(mask)

    def set_adaptive(self, tol: float, min_spp: int = 0):
        self.acc.set_adaptive(tol, min_spp)

    def active(self):
        return self.acc.active()

    def counts(self):
        return self.acc.counts()

    def read(self):
        return self.acc.read()

    def load(self, sum_, stat, samples_done: int, counts=None):
        self.acc.load(sum_, stat, samples_done, counts)

    def close(self):
        self.acc.close()


class TorchTracer:
    """Ray queries on torch tensors (rtw_hip.h "ray queries"): closest hits and occlusion of
    caller-supplied rays over a DeviceScene or a world.DeviceWorld of the current device,
    launched on torch's current HIP stream.

        tr = TorchTracer(world)
        hit = tr.trace(origins, dirs)          # (N, 3) float64 device tensors
        lit = ~tr.occluded(hit["p"], to_light, t_max=1.0)
        what = tr.surface(hit)                 # material kind / index, texture value, fuzz, ir per hit
        g = tr.guides(cam, W, H, background)   # a frame's rtw_guide records from one BVH trace
    """

    def __init__(self, target, device: int | torch.device | None = None):
        if not torch.cuda.is_available():
            raise RuntimeError("no GPU visible: the rtw query path has no CPU fallback")
        if device is None:
            device = torch.cuda.current_device()
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        self.target = target
        self.is_world = not isinstance(target, DeviceScene)

    def pack(self, origins, dirs, time=0.5, t_min=0.001, t_max=float("inf")) -> torch.Tensor:
        """The (N, 9) float64 ray tensor (rtw_ray records) from (N, 3) origins and directions and
        scalars or (N,) tensors of time, t_min, t_max — torch ops on the current stream."""
        o = torch.as_tensor(origins, dtype=torch.float64, device=self.device)
        d = torch.as_tensor(dirs, dtype=torch.float64, device=self.device)
        if o.dim() != 2 or o.shape[1] != 3 or d.shape != o.shape:
            raise ValueError("origins and dirs must both be (N, 3)")
        rays = torch.empty((o.shape[0], 9), dtype=torch.float64, device=self.device)
        rays[:, 0:3] = o
        rays[:, 3:6] = d
        for col, v in ((6, time), (7, t_min), (8, t_max)):
            rays[:, col] = torch.as_tensor(v, dtype=torch.float64, device=self.device) if torch.is_tensor(v) else float(v)
        return rays

    def _launch(self, f, rays, out, opts):
        stream = torch.cuda.current_stream(self.device).cuda_stream
        if rays.shape[0] == 0:
            return
        if self.is_world:
            f(rays.data_ptr(), rays.shape[0], out.data_ptr(), opts, stream)
        else:
            f(rays.data_ptr(), rays.shape[0], out.data_ptr(), stream)

    def trace(self, origins, dirs, time=0.5, t_min=0.001, t_max=float("inf"), opts: QueryOpts | None = None) -> dict:
        """Closest hits: a dict of tensors viewing one (N, 10) float64 record buffer — t (N,), p (N, 3),
        normal (N, 3), uv (N, 2) — and prim (N,) int64 (the list index, -1 for a miss), front (N,) bool."""
        rays = self.pack(origins, dirs, time, t_min, t_max)
        rec = torch.empty((rays.shape[0], 10), dtype=torch.float64, device=self.device)
        self._launch(self.target.trace, rays, rec, opts)
        words = rec.view(torch.int32)[:, 18:20]  # {prim, front}: the record's last 8 bytes
        return {"t": rec[:, 0], "p": rec[:, 1:4], "normal": rec[:, 4:7], "uv": rec[:, 7:9],
                "prim": words[:, 0].to(torch.int64) - 1, "front": words[:, 1] != 0, "records": rec}

    def occluded(self, origins, dirs, time=0.5, t_min=0.001, t_max=float("inf"),
                 opts: QueryOpts | None = None) -> torch.Tensor:
        """(N,) bool: whether trace() of the same rays would hit."""
        rays = self.pack(origins, dirs, time, t_min, t_max)
        out = torch.empty((rays.shape[0],), dtype=torch.uint8, device=self.device)
        self._launch(self.target.occluded, rays, out, opts)
        return out != 0

    def surface(self, hits, guides: bool = False, background=None) -> dict:
        """What the surfaces under `hits` are (rtw_hip.h "surface queries"): hits is trace()'s dict or its
        (N, 10) float64 record tensor.  A dict of tensors viewing one (N, 8) float64 record buffer
        (rtw_surface) — value (N, 3), fuzz (N,), ir (N,) — and kind, mat, tex, tex_kind (N,) int64: the
        rtw_wmaterial_kind, material index, texture index and rtw_texture_kind, -1 where there is none (a
        miss; tex of a metal, a glass or a scene).  guides=True adds "guides": (N, 32) uint8 rtw_guide
        records of those rays (`background`: a miss's albedo)."""
        rec_in = hits["records"] if isinstance(hits, dict) else hits
        if rec_in.dtype != torch.float64 or rec_in.dim() != 2 or rec_in.shape[1] != 10 or not rec_in.is_contiguous():
            raise ValueError("hits must be trace()'s result or its contiguous (N, 10) float64 records")
        n = rec_in.shape[0]
        rec = torch.empty((n, 8), dtype=torch.float64, device=self.device)
        g = torch.empty((n, 32), dtype=torch.uint8, device=self.device) if guides else None
        if n:
            self.target.surface(rec_in.data_ptr(), n, rec.data_ptr(), g.data_ptr() if guides else None,
                                background if guides else None, torch.cuda.current_stream(self.device).cuda_stream)
        words = rec.view(torch.int32)[:, 10:14].to(torch.int64) - 1  # {kind, mat, tex, tex_kind}, each + 1
        out = {"value": rec[:, 0:3], "fuzz": rec[:, 3], "ir": rec[:, 4], "kind": words[:, 0], "mat": words[:, 1],
               "tex": words[:, 2], "tex_kind": words[:, 3], "records": rec}
        if guides:
            out["guides"] = g
        return out

    def guides(self, cam: Camera, width: int, height: int, background) -> torch.Tensor:
        """A frame's feature buffers, (height, width, 32) uint8 rtw_guide records, from the frame's feature
        rays (rtw_pixel_rays_device), their closest hits and the surface query: the bytes of
        rtw_world_guides_device / rtw_scene_guides_device of the whole frame, at the cost of one BVH trace.
        On torch's current stream; the ray and hit tensors are kept between calls of one size."""
        n = width * height
        if getattr(self, "_frame_n", None) != n:
            self._frame_rays = torch.empty((n, 9), dtype=torch.float64, device=self.device)
            self._frame_hits = torch.empty((n, 10), dtype=torch.float64, device=self.device)
            self._frame_n = n
        stream = torch.cuda.current_stream(self.device).cuda_stream
        pixel_rays_device(cam, width, height, self._frame_rays.data_ptr(), stream)
        self._launch(self.target.trace, self._frame_rays, self._frame_hits, None)
        g = torch.empty((height, width, 32), dtype=torch.uint8, device=self.device)
        self.target.surface(self._frame_hits.data_ptr(), n, None, g.data_ptr(), background, stream)
        return g

    def mirror_points(self, rays, hits, cam_prev: Camera, a_prev=None, xv_prev=None, opts=None, hits2: bool = False):
        """The prev_p of TemporalAccumulator.step with the mirrors followed (rtw_hip.h "mirror points"): rays is
        the (N, 9) float64 ray tensor the hits came from (pack()'s), hits trace()'s dict or its (N, 10) record
        tensor.  (N, 3) float64: each hit's surface point under the previous numbers (a_prev (n_prims, 9),
        xv_prev (n_xforms, 4, 3) float64 device tensors; None: the current ones), and for a front hit of a
        metal primitive the point of the mirror that showed the same reflected thing from cam_prev.  One
        launch on torch's current stream.  hits2=True: (prev_p, the reflected rays' (N, 10) records)."""
        if not self.is_world:
            raise ValueError("mirror_points needs a world.DeviceWorld")
        rec_in = hits["records"] if isinstance(hits, dict) else hits
        n = rec_in.shape[0]
        for name, t, cols in (("rays", rays, 9), ("hits", rec_in, 10)):
            if t.dtype != torch.float64 or t.dim() != 2 or t.shape != (n, cols) or not t.is_contiguous() or not t.is_cuda:
                raise ValueError(f"{name} must be a contiguous (N, {cols}) float64 tensor on the world's device")
        for name, t, shape in (("a_prev", a_prev, (self.target.n_prims, 9)), ("xv_prev", xv_prev, (self.target.n_xforms, 4, 3))):
            if t is not None and (t.dtype != torch.float64 or tuple(t.shape) != shape or not t.is_contiguous() or not t.is_cuda):
                raise ValueError(f"{name} must be a contiguous float64 device tensor of shape {shape}")
        out = torch.empty((n, 3), dtype=torch.float64, device=self.device)
        rec2 = torch.empty((n, 10), dtype=torch.float64, device=self.device) if hits2 else None
        if n:
            self.target.mirror_points_device(rays.data_ptr(), rec_in.data_ptr(), n, cam_prev, out.data_ptr(),
                                             a_prev.data_ptr() if a_prev is not None and a_prev.numel() else None,
                                             xv_prev.data_ptr() if xv_prev is not None and xv_prev.numel() else None, opts,
                                             rec2.data_ptr() if hits2 else None,
                                             torch.cuda.current_stream(self.device).cuda_stream)
        return (out, rec2) if hits2 else out


def update_world(dw, a: torch.Tensor, xv: torch.Tensor | None = None):
    """New numbers for a dynamic world.DeviceWorld from torch tensors of its device
    (rtw_world_update_device on torch's current stream, no host round trip): a is
    (n_prims, 9) float64 in list order (a triangle's row is its three vertices v0, v1, v2), xv (n_xforms, 4, 3) float64 or None (the transforms
    keep their values).  Renders and queries enqueued afterwards on that stream see the new
    world; torch's caching allocator keeps the tensors' memory valid for work of that stream."""
    _numbers_to_world(dw.update_device, dw, a, xv)


def rebuild_world(dw, a: torch.Tensor, xv: torch.Tensor | None = None):
    """A new tree for a dynamic world.DeviceWorld from torch tensors of its device
    (rtw_world_rebuild_device on torch's current stream): the arguments of update_world.  The
    world takes the numbers as an update does and is re-sorted and split anew from them;
    dw.bvh_cost() against its value after the last rebuild tells when that pays."""
    _numbers_to_world(dw.rebuild_device, dw, a, xv)


def _numbers_to_world(entry, dw, a, xv):
    for name, t, tail in (("a", a, (9,)), ("xv", xv, (4, 3))):
        if t is None:
            continue
        if t.dtype != torch.float64 or not t.is_cuda or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous float64 tensor on the world's device")
        if tuple(t.shape[1:]) != tail or t.dim() != len(tail) + 1:
            raise ValueError(f"{name} must have shape (n, {', '.join(map(str, tail))})")
    if a.shape[0] != dw.n_prims or (xv is not None and xv.shape[0] != dw.n_xforms):
        raise ValueError(f"the world has {dw.n_prims} primitives and {dw.n_xforms} transforms")
    if xv is not None and xv.device != a.device:
        raise ValueError("a and xv live on different devices")
    with torch.cuda.device(a.device):
        entry(a.data_ptr(), xv.data_ptr() if xv is not None and xv.numel() else None,
              torch.cuda.current_stream(a.device).cuda_stream)


class TemporalAccumulator:
    """Temporal accumulation on torch tensors (rtw_hip.h "temporal accumulation"): owns the two
    history images of a width x height animation and blends one frame per step() into them on
    torch's current HIP stream.

        ta = TemporalAccumulator(W, H)
        mean_out, var_out = ta.step(mean, guides, cam, prev_p)   # feed both to the denoiser

    clamp (rtw_amd.temporal_clamp(...)): each step clamps the history to the frame's neighbourhood
    (rtw_temporal_clamped_device); None: rtw_temporal_device as before.
    """

    def __init__(self, width: int, height: int, opts: TemporalOpts | None = None,
                 device: int | torch.device | None = None, clamp: TemporalClamp | None = None):
        if not torch.cuda.is_available():
            raise RuntimeError("no GPU visible: the rtw temporal path has no CPU fallback")
        if device is None:
            device = torch.cuda.current_device()
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        self.width, self.height, self.opts, self.clamp = int(width), int(height), opts, clamp
        self.hist = [torch.zeros((self.height, self.width, 32), dtype=torch.uint8, device=self.device) for _ in range(2)]
        self.reset()

    def reset(self):
        """Forget the history: the next step() is a first frame."""
        self.frames, self.cam_prev = 0, None

    def history(self) -> torch.Tensor:
        """The history image the last step() wrote ((H, W, 32) uint8: rtw_history records)."""
        return self.hist[(self.frames + 1) & 1]

    def step(self, mean: torch.Tensor, guides: torch.Tensor, cam: Camera, prev_p: torch.Tensor | None = None):
        """One frame: mean (H, W, 3) float32, guides (H, W, 32) uint8 (rtw_guide records), prev_p
        (H, W, 3) float64 or None (nothing moved).  Returns (mean_out (H, W, 3) float32, var_out
        (H, W) float32): the accumulated mean and the variance for rtw_denoise_device's d_var."""
        H, W = self.height, self.width
        for name, t, dt, n in (("mean", mean, torch.float32, H * W * 3), ("guides", guides, torch.uint8, H * W * 32),
                               ("prev_p", prev_p, torch.float64, H * W * 3)):
            if t is None:
                continue
            if t.dtype != dt or t.device != self.device or not t.is_contiguous() or t.numel() != n:
                raise ValueError(f"{name} must be a contiguous {dt} tensor of {n} elements on {self.device}")
        src, dst = self.hist[(self.frames + 1) & 1], self.hist[self.frames & 1]
        mean_out = torch.empty((H, W, 3), dtype=torch.float32, device=self.device)
        var_out = torch.empty((H, W), dtype=torch.float32, device=self.device)
        cam_now = Camera.from_buffer_copy(cam)
        args = (mean.data_ptr(), guides.data_ptr(), prev_p.data_ptr() if prev_p is not None else None,
                self.cam_prev if self.frames else cam_now, cam_now, src.data_ptr() if self.frames else None,
                W, H, dst.data_ptr(), mean_out.data_ptr(), var_out.data_ptr(), self.opts)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            if self.clamp is None:
                temporal_device(*args, stream)
            else:
                temporal_clamped_device(*args, self.clamp, stream)
        self.frames += 1
        self.cam_prev = cam_now
        return mean_out, var_out
