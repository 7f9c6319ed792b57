"""Batched ray-cast renderer over the native library (mjl_render_qpos, csrc/render_kernels.hip).

    reference                                                   here
    mujoco.Renderer(mj_model, height, width)  rendering.py:181  Renderer(sys, max_frames, device)
    mj_data.qpos[:] = q; mj_forward;                            Renderer.render(qpos [n, nq], camera, width,
    renderer.update_scene(camera=...); render()  :186-192           height) -> frames [n, H, W, 3] uint8

One call renders n frames: a qpos history (video) or the qpos rows of a batch (per-env camera
images: RGB, depth, segmentation). Planes, spheres and capsules only; the shading model is
DESIGN.md "Rendering". There is no fallback: without the library or a GPU this raises.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Union

import torch

from . import abi, mjcf
from ._lib import MjlError, check, lib
from .mjx import Model, _ptr, _stream


class Frames(NamedTuple):
    rgb: Optional[torch.Tensor]    # uint8 [n, H, W, 3]
    depth: Optional[torch.Tensor]  # float32 [n, H, W]: distance along the pixel's ray, +inf = nothing within zfar
    seg: Optional[torch.Tensor]    # int32 [n, H, W]: geom id, -1 = background


class Renderer:
    """Renders up to `max_frames` frames per call of model `sys` on GPU `device`."""

    def __init__(self, sys: Model, max_frames: int = 64, device: int = 0):
        if not torch.cuda.is_available():
            raise MjlError("mjx355 needs a GPU (torch.cuda.is_available() is False)")
        self.sys = sys
        self.max_frames = int(max_frames)
        self.device = torch.device("cuda", device)
        self.visual = abi.visual_desc(sys.m)
        h = C.c_void_p()
        check(lib().mjl_renderer_create(sys.handle, C.byref(self.visual), self.max_frames, int(device), C.byref(h)))
        self._h = h

    @property
    def handle(self):
        return self._h

    def render(self, qpos: torch.Tensor, camera: Union[str, int] = "side_view", width: int = 640, height: int = 480,
               shadows: bool = True, rgb: bool = True, depth: bool = False, seg: bool = False) -> Frames:
        """qpos [n, nq] (n <= max_frames) -> Frames; an output that was not asked for is None."""
        cam = mjcf.camera_id(self.sys.m, camera)
        q = qpos.to(device=self.device, dtype=torch.float32).reshape(-1, self.sys.nq).contiguous()
        n, dev = q.shape[0], self.device
        o_rgb = torch.empty((n, height, width, 3), dtype=torch.uint8, device=dev) if rgb else None
        o_depth = torch.empty((n, height, width), dtype=torch.float32, device=dev) if depth else None
        o_seg = torch.empty((n, height, width), dtype=torch.int32, device=dev) if seg else None
        raw = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
        check(lib().mjl_render_qpos(self._h, _ptr(q), n, cam, int(width), int(height),
                                    abi.RENDER_SHADOWS if shadows else 0, raw(o_rgb), raw(o_depth), raw(o_seg),
                                    _stream()))
        return Frames(o_rgb, o_depth, o_seg)

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                lib().mjl_renderer_destroy(self._h)
                self._h = None
        except Exception:
            pass
