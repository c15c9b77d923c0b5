"""Torch-side plumbing for the device-resident API: HBM buffers from torch's
caching allocator, the render launched on torch's current HIP stream.
Torch is plumbing here (device memory, streams, torch.distributed); the
rendering is the HIP kernels of lib/librtw_hip.so."""
from __future__ import annotations

import torch

from . import Accumulator, Camera, DeviceScene, Params, Timer, workspace_bytes


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
    """

    def __init__(self, target, params: Params, device: int | torch.device | None = None):
        if not torch.cuda.is_available():
            raise RuntimeError("no GPU visible: the rtw render path has no CPU fallback")
        if device is None:
            device = torch.cuda.current_device()
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        torch.cuda.set_device(self.device)
        self.params = params
        self.acc = Accumulator(target, params)
        self._ws = None
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

    def render_pass(self, cam: Camera, pass_spp: int, timer: Timer | None = None) -> torch.Tensor:
        """One pass and its resolve, asynchronous; returns the rgb tensor (rows, W, 3) uint8
        (self.mean holds the f32 mean).  The tensors are reused by the next pass."""
        ptr, nbytes = self._ws_ptr(pass_spp)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        self.acc.render_pass(cam, pass_spp, ptr, nbytes, stream, timer)
        self.acc.resolve(self.rgb.data_ptr(), self.mean.data_ptr(), stream)
        return self.rgb

    def passes(self, cam: Camera, pass_spp: int, max_noise: float | None = None):
        """Yield the image after each pass of pass_spp samples (the last one may
        be shorter) until the frame's spp, or until noise() <= max_noise."""
        while self.acc.samples() < self.params.spp:
            yield self.render_pass(cam, min(pass_spp, self.params.spp - self.acc.samples()))
            if max_noise is not None and self.acc.samples() >= 2 * self.acc.chunk and self.noise() <= max_noise:
                return

    def noise(self) -> float:
        return self.acc.noise(torch.cuda.current_stream(self.device).cuda_stream)

    def samples(self) -> int:
        return self.acc.samples()

    def close(self):
        self.acc.close()
