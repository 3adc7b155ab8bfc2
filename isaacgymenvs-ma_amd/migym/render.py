"""Images of the envs' collision geometry: the Python side of ``mg_render`` (include/migym.h, csrc/render.hpp).

    r = Renderer(lib, sim, spec, num_envs, num_agents, "cuda:0", width=64, height=64)
    out = r.render([0, 5], rgb=True, depth=True)     # {"rgb": (2, 64, 64, 3) uint8, "depth": (2, 64, 64) fp32}

Two launches on the current (or the given) stream and no host synchronisation: the returned tensors are device
tensors the renderer owns and overwrites on its next call with the same shape; a caller that keeps a frame clones it.
The camera, the primitive order behind the id image and the shading are defined in include/migym.h; ``PALETTE`` and
the constants below restate the kernel's so that a host-side reference (tests/render_ref.py) can reproduce an image.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _abi

REC_FLOATS = 16          # one primitive record: rotation 9 (row-major), position 3, size 3, type | colour << 8
MAX_PRIMS = 512
T_MIN = 1e-4
NONE_TYPE = 7            # record type of an env id out of range
COL_OBJECT, COL_GOAL, COL_BOX, COL_GROUND, COL_SKY = 8, 9, 10, 11, 13
# the kernel's colour table: 0..7 by geom_body % 8, then object, goal, extra box, the ground's two greys, the sky
PALETTE = np.array([
    [0.90, 0.30, 0.25], [0.25, 0.60, 0.90], [0.35, 0.75, 0.35], [0.95, 0.75, 0.20],
    [0.65, 0.40, 0.85], [0.20, 0.75, 0.75], [0.95, 0.55, 0.25], [0.75, 0.75, 0.78],
    [0.95, 0.85, 0.30], [0.40, 0.95, 0.55], [0.90, 0.45, 0.75], [0.55, 0.55, 0.55],
    [0.75, 0.75, 0.75], [0.53, 0.73, 0.92]], np.float64)
LIGHT = np.array([0.3, 0.2, 1.0]) / math.sqrt(0.3 * 0.3 + 0.2 * 0.2 + 1.0)
AMBIENT, DIFFUSE = 0.35, 0.65


def num_primitives(spec, num_agents: int, num_boxes: int) -> int:
    """primitives per env: the actors' geoms, the free object and the goal, the extra boxes, the ground"""
    return num_agents * len(spec.geoms) + (2 if spec.obj else 0) + num_boxes + 1


class Renderer:
    """A camera on the envs of one ``mg_sim``.  ``eye_offset`` / ``target_offset`` are relative to the root position
    of the env's actor 0 (``follow=True``) or to the origin."""

    def __init__(self, lib, sim, spec, num_envs, num_agents, device, width, height, fov_deg=60.0,
                 eye_offset=(2.5, -2.5, 1.5), target_offset=(0.0, 0.0, 0.0), follow=True):
        self._lib, self.sim, self.spec = lib, sim, spec
        self.num_envs, self.num_agents, self.device = int(num_envs), int(num_agents), torch.device(device)
        self.width, self.height, self.fov_deg = int(width), int(height), float(fov_deg)
        self.eye_offset = tuple(float(x) for x in eye_offset)
        self.target_offset = tuple(float(x) for x in target_offset)
        self.follow = bool(follow)
        if len(self.eye_offset) != 3 or len(self.target_offset) != 3:
            raise ValueError("eye_offset and target_offset are 3-vectors")
        self._bufs = {}       # name -> tensor, reused while the shape is unchanged
        self._id_cache = {}   # host id list -> its int32 device tensor
        self._keep = None

    # ------------------------------------------------------------------------------------------------
    def _buf(self, name, shape, dtype):
        t = self._bufs.get(name)
        if t is None or tuple(t.shape) != tuple(shape):
            t = self._bufs[name] = torch.zeros(shape, device=self.device, dtype=dtype)
        return t

    def _ids(self, env_ids):
        """(device int32 tensor or None, n_sel).  A host list is checked against 0..N-1 here; a device tensor is
        not (that would synchronise): an id out of range renders as sky."""
        if env_ids is None:
            return None, self.num_envs
        if isinstance(env_ids, torch.Tensor):
            t = env_ids.flatten()
            if t.device != self.device or t.dtype != torch.int32 or not t.is_contiguous():
                if t.device.type == "cpu":
                    return self._ids(t.tolist())
                t = t.to(device=self.device, dtype=torch.int32).contiguous()
            return t, int(t.numel())
        key = tuple(int(i) for i in np.asarray(env_ids).reshape(-1))
        for i in key:
            if i < 0 or i >= self.num_envs:
                raise ValueError(f"render: env id {i} is outside 0..{self.num_envs - 1}")
        t = self._id_cache.get(key)
        if t is None:
            if len(self._id_cache) > 64:
                self._id_cache.clear()
            t = self._id_cache[key] = torch.tensor(key, dtype=torch.int32, device=self.device)
        return t, len(key)

    def scratch_records(self, n_sel: int, num_boxes: int = 0) -> torch.Tensor:
        """the (n_sel, P, 16) primitive records of the last render with these counts (tests, debugging)"""
        P = num_primitives(self.spec, self.num_agents, num_boxes)
        return self._bufs["scratch"][:n_sel * P * REC_FLOATS].view(n_sel, P, REC_FLOATS)

    def render(self, env_ids=None, *, rgb=True, depth=False, ids=False, boxes=None, stream=None):
        """Ray-cast the listed envs (None = all).  ``boxes``: (N, K, 10) fp32 device tensor of extra boxes per env
        (pos 3, quat xyzw 4, half extents 3).  Returns {"rgb": (n, H, W, 3) uint8, "depth": (n, H, W) fp32 (+inf =
        sky), "ids": (n, H, W) int32 (-1 = sky)} with the requested entries, asynchronously on ``stream`` (a
        torch.cuda.Stream or a raw handle; None = the current stream)."""
        id_t, n_sel = self._ids(env_ids)
        K = 0
        if boxes is not None:
            if boxes.dim() != 3 or boxes.shape[0] != self.num_envs or boxes.shape[2] != 10:
                raise ValueError(f"boxes must be ({self.num_envs}, K, 10), got {tuple(boxes.shape)}")
            if boxes.device != self.device or boxes.dtype != torch.float32 or not boxes.is_contiguous():
                boxes = boxes.to(device=self.device, dtype=torch.float32).contiguous()
            K = int(boxes.shape[1])
            if K == 0:
                boxes = None
        a = _abi.RenderArgs()
        a.width, a.height, a.fov_y = self.width, self.height, math.radians(self.fov_deg)
        for k in range(3):
            a.eye_offset[k], a.target_offset[k] = self.eye_offset[k], self.target_offset[k]
        a.follow = int(self.follow)
        a.env_ids, a.n_sel = _abi.ptr(id_t), n_sel
        a.boxes, a.num_boxes = _abi.ptr(boxes), K
        out = {}
        if n_sel >= 1:
            need = int(self._lib.mg_render_scratch_floats(self.sim, n_sel, K))
            scratch = self._bufs.get("scratch")
            if need and (scratch is None or scratch.numel() < need):
                scratch = self._bufs["scratch"] = torch.zeros(need, device=self.device, dtype=torch.float32)
            a.scratch = _abi.ptr(scratch) if need else None
            H, W = self.height, self.width
            if H >= 1 and W >= 1:
                if rgb:
                    out["rgb"] = self._buf("rgb", (n_sel, H, W, 3), torch.uint8)
                if depth:
                    out["depth"] = self._buf("depth", (n_sel, H, W), torch.float32)
                if ids:
                    out["ids"] = self._buf("ids", (n_sel, H, W), torch.int32)
            a.rgb, a.depth, a.ids = _abi.ptr(out.get("rgb")), _abi.ptr(out.get("depth")), _abi.ptr(out.get("ids"))
        if stream is None:
            stream = torch.cuda.current_stream(self.device).cuda_stream
        elif hasattr(stream, "cuda_stream"):
            stream = stream.cuda_stream
        self._keep = (id_t, boxes)   # alive until the launches have consumed them
        _abi.check(self._lib.mg_render(self.sim, _abi.C.byref(a), stream), self._lib)
        return out


def write_ppm(path, frame):
    """one (H, W, 3) uint8 array as a binary PPM"""
    frame = np.ascontiguousarray(frame, np.uint8)
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (frame.shape[1], frame.shape[0]))
        f.write(frame.tobytes())
