"""Motion clips for HumanoidAMP as one device table (no poselib).

Reference counterpart: ``tasks/amp/utils_amp/motion_lib.py`` (MotionLib) on top of poselib's ``SkeletonMotion``.  The
reference keeps its clips on the host and samples them with numpy on every reset; here everything a sample needs is
computed once, on the host, and packed into a flat fp32 array that the reset and demo kernels read
(``mg_amp_views.motion_frames``, include/migym.h): per frame, 113 floats

    root position 3 | root rotation 4 (xyzw) | root velocity 3 | root angular velocity 3 |
    local rotations 15 x 4 | DOF velocities 28 | key-body positions 4 x 3

and per motion (first frame, frame count) as int32 and (frame dt, length, cumulative normalised weight) as fp64.

A motion file is
  * the reference's ``.npy``: the pickled dict ``SkeletonMotion.from_file`` reads (``rotation``, ``root_translation``,
    ``global_velocity``, ``global_angular_velocity``, ``skeleton_tree``, ``is_local``, ``fps``);
  * a plain ``.npz`` with the same arrays and no pickled objects: ``rotation``, ``root_translation``,
    ``global_velocity``, ``global_angular_velocity``, ``parent_indices``, ``local_translation``, ``is_local``, ``fps``;
  * a ``.yaml`` list ``motions: [{file, weight}, ...]`` of such files, relative to the yaml's directory
    (MotionLib._fetch_motion_files).

The per-frame tensors are computed in fp32 torch on the CPU with poselib's expressions (forward kinematics over the
skeleton tree, ``quat_mul_norm``, ``quat_angle_axis``), so that they agree with MotionLib's to rounding.
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import List, Sequence

import numpy as np
import torch

from . import _abi

# DOF_BODY_IDS, DOF_OFFSETS (amp/humanoid_amp_base.py:41-42)
DOF_BODY_IDS = [1, 2, 3, 4, 6, 7, 9, 10, 11, 12, 13, 14]
DOF_OFFSETS = [0, 3, 6, 9, 10, 13, 14, 17, 18, 21, 24, 25, 28]
FRAME = _abi.MG_AMP_FRAME_FLOATS
F_ROT, F_DOF_VEL, F_KEY = 13, 13 + 4 * _abi.MG_AMP_BODIES, 13 + 4 * _abi.MG_AMP_BODIES + _abi.MG_AMP_DOFS


# ---- poselib's quaternion expressions (poselib/core/rotation3d.py), xyzw, fp32 torch
def _quat_mul(a, b):
    x1, y1, z1, w1 = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    x2, y2, z2, w2 = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    w = w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2
    x = w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2
    y = w1 * y2 + y1 * w2 + z1 * x2 - x1 * z2
    z = w1 * z2 + z1 * w2 + x1 * y2 - y1 * x2
    return torch.stack([x, y, z, w], dim=-1)


def _quat_normalize(q):
    q = (1 - 2 * (q[..., 3:] < 0).float()) * q                            # quat_pos
    return q / q.norm(p=2, dim=-1).unsqueeze(-1).clamp(min=1e-9)          # quat_unit


def _quat_mul_norm(a, b):
    return _quat_normalize(_quat_mul(a, b))


def _quat_conjugate(q):
    return torch.cat([-q[..., :3], q[..., 3:]], dim=-1)


def _quat_rotate(rot, vec):
    other = torch.cat([vec, torch.zeros_like(vec[..., :1])], dim=-1)
    return _quat_mul(_quat_mul(rot, other), _quat_conjugate(rot))[..., :3]


def _quat_angle_axis(q):
    s = 2 * (q[..., 3] ** 2) - 1
    angle = s.clamp(-1, 1).arccos()
    axis = q[..., :3]
    axis = axis / axis.norm(p=2, dim=-1, keepdim=True).clamp(min=1e-9)
    return angle, axis


@dataclass
class Motion:
    """One clip's per-frame tensors, what MotionLib holds of a SkeletonMotion (numpy)."""
    fps: float
    global_translation: np.ndarray    # (F, 15, 3) fp32
    global_rotation: np.ndarray       # (F, 15, 4) fp32
    local_rotation: np.ndarray        # (F, 15, 4) fp32
    root_velocity: np.ndarray         # (F, 3) fp32
    root_angular_velocity: np.ndarray  # (F, 3) fp32
    dof_vels: np.ndarray              # (F, 28) fp64 holding fp32 values, the last frame repeated

    @property
    def num_frames(self) -> int:
        return int(self.global_translation.shape[0])


def read_clip(path: str) -> dict:
    """The arrays of one motion file (``.npy`` dict or plain ``.npz``) under the ``.npz`` names."""
    ext = os.path.splitext(path)[1].lower()
    if ext == ".npz":
        with np.load(path, allow_pickle=False) as z:
            return {k: z[k] for k in z.files}
    if ext == ".npy":
        d = np.load(path, allow_pickle=True).item()
        tree = d["skeleton_tree"]
        return {"rotation": d["rotation"]["arr"], "root_translation": d["root_translation"]["arr"],
                "global_velocity": d["global_velocity"]["arr"],
                "global_angular_velocity": d["global_angular_velocity"]["arr"],
                "parent_indices": tree["parent_indices"]["arr"], "local_translation": tree["local_translation"]["arr"],
                "is_local": np.asarray(bool(d["is_local"])), "fps": np.asarray(d["fps"])}
    raise ValueError(f"motion file {path!r}: expected .npy, .npz or .yaml")


def load_clip(path: str, num_dofs: int = _abi.MG_AMP_DOFS) -> Motion:
    """SkeletonMotion.from_file + MotionLib._compute_motion_dof_vels for one file."""
    c = read_clip(path)
    rot = torch.from_numpy(np.ascontiguousarray(c["rotation"], dtype=np.float32))
    rt = torch.from_numpy(np.ascontiguousarray(c["root_translation"], dtype=np.float32))
    parents = [int(p) for p in np.asarray(c["parent_indices"]).tolist()]
    tree_t = torch.from_numpy(np.ascontiguousarray(c["local_translation"], dtype=np.float32))
    nf, nj = int(rot.shape[0]), int(rot.shape[1])
    if nj != _abi.MG_AMP_BODIES or len(parents) != nj:
        raise ValueError(f"motion file {path!r}: {nj} joints, the AMP humanoid has {_abi.MG_AMP_BODIES}")
    if nf < 2:
        raise ValueError(f"motion file {path!r}: a motion needs at least 2 frames")
    if any(p >= j for j, p in enumerate(parents)):
        raise ValueError(f"motion file {path!r}: parents must come before their children")
    fps = float(np.asarray(c["fps"]))
    if bool(np.asarray(c["is_local"])):
        local_rot = rot
    else:   # SkeletonState.local_rotation of global rotations
        local_rot = torch.zeros_like(rot)
        for j, p in enumerate(parents):
            local_rot[:, j] = rot[:, j] if p < 0 else _quat_mul_norm(_quat_conjugate(rot[:, p]), rot[:, j])
    local_t = tree_t.unsqueeze(0).expand(nf, nj, 3).clone()
    local_t[:, 0] = rt
    # SkeletonState.global_transformation: transform_mul down the tree
    g_rot: List[torch.Tensor] = []
    g_t: List[torch.Tensor] = []
    for j, p in enumerate(parents):
        if p < 0:
            g_rot.append(local_rot[:, j])
            g_t.append(local_t[:, j])
        else:
            g_rot.append(_quat_mul_norm(g_rot[p], local_rot[:, j]))
            g_t.append(_quat_rotate(g_rot[p], local_t[:, j]) + g_t[p])
    global_rot = torch.stack(g_rot, dim=1) if bool(np.asarray(c["is_local"])) else rot
    global_t = torch.stack(g_t, dim=1)
    # MotionLib._local_rotation_to_dof_vel between consecutive frames, the last one repeated
    dt = 1.0 / fps
    diff = _quat_mul_norm(_quat_conjugate(local_rot[:-1]), local_rot[1:])
    angle, axis = _quat_angle_axis(diff)
    local_vel = (axis * angle.unsqueeze(-1) / dt).numpy()
    dof_vels = np.zeros((nf, num_dofs))
    for j, b in enumerate(DOF_BODY_IDS):
        o, size = DOF_OFFSETS[j], DOF_OFFSETS[j + 1] - DOF_OFFSETS[j]
        if size == 3:
            dof_vels[:-1, o:o + 3] = local_vel[:, b]
        else:
            dof_vels[:-1, o] = local_vel[:, b, 1]   # the joint is taken to turn about y
    dof_vels[-1] = dof_vels[-2]
    vel = np.ascontiguousarray(c["global_velocity"], dtype=np.float32)
    avel = np.ascontiguousarray(c["global_angular_velocity"], dtype=np.float32)
    return Motion(fps=fps, global_translation=global_t.numpy(), global_rotation=global_rot.numpy(),
                  local_rotation=local_rot.numpy(), root_velocity=vel[:, 0].copy(),
                  root_angular_velocity=avel[:, 0].copy(), dof_vels=dof_vels)


def fetch_motion_files(motion_file: str):
    """MotionLib._fetch_motion_files: ([files], [weights])"""
    if os.path.splitext(motion_file)[1].lower() == ".yaml":
        import yaml
        with open(motion_file, "r") as f:
            cfg = yaml.safe_load(f)
        files, weights = [], []
        for entry in cfg["motions"]:
            if entry["weight"] < 0:
                raise ValueError(f"{motion_file}: negative weight for {entry['file']}")
            files.append(os.path.join(os.path.dirname(motion_file), entry["file"]))
            weights.append(entry["weight"])
        return files, weights
    return [motion_file], [1.0]


class MotionTable:
    """Every clip of a motion file, packed for the device (module docstring)."""

    def __init__(self, motion_file: str, key_body_ids: Sequence[int], num_dofs: int = _abi.MG_AMP_DOFS):
        files, weights = fetch_motion_files(motion_file)
        if not files:
            raise ValueError(f"{motion_file}: no motions")
        self.files = files
        self.key_body_ids = [int(k) for k in key_body_ids]
        if len(self.key_body_ids) != _abi.MG_AMP_KEY_BODIES:
            raise ValueError("the AMP humanoid has four key bodies")
        self.motions = [load_clip(f, num_dofs) for f in files]
        self.fps = np.array([m.fps for m in self.motions])
        self.dt = np.array([1.0 / m.fps for m in self.motions])                      # motion_lib.py:173
        self.num_frames = np.array([m.num_frames for m in self.motions])
        self.lengths = np.array([1.0 / m.fps * (m.num_frames - 1) for m in self.motions])   # motion_lib.py:176
        w = np.array(weights, dtype=np.float64) if len(weights) else np.ones(1)
        self.weights = w / np.sum(w)                                                 # motion_lib.py:194-195
        # np.random.choice(p=...) draws from p.cumsum() normalised by its last entry, searchsorted side="right"
        cdf = self.weights.cumsum()
        self.cdf = cdf / cdf[-1]
        self.first_frame = np.concatenate([[0], np.cumsum(self.num_frames)[:-1]]).astype(np.int64)
        self.frames = np.concatenate([self._pack(m) for m in self.motions], axis=0)
        self.index = np.stack([self.first_frame, self.num_frames], axis=1).astype(np.int32)
        self.time = np.stack([self.dt, self.lengths, self.cdf], axis=1).astype(np.float64)

    def _pack(self, m: Motion) -> np.ndarray:
        nf = m.num_frames
        out = np.zeros((nf, FRAME), np.float32)
        out[:, 0:3] = m.global_translation[:, 0]
        out[:, 3:7] = m.global_rotation[:, 0]
        out[:, 7:10] = m.root_velocity
        out[:, 10:13] = m.root_angular_velocity
        out[:, F_ROT:F_DOF_VEL] = m.local_rotation.reshape(nf, -1)
        out[:, F_DOF_VEL:F_KEY] = m.dof_vels.astype(np.float32)
        out[:, F_KEY:] = m.global_translation[:, self.key_body_ids].reshape(nf, -1)
        return out

    def num_motions(self) -> int:
        return len(self.motions)

    def get_total_length(self) -> float:
        return float(sum(self.lengths))

    def to_device(self, device):
        """(frames, index, time) as device tensors, in the layout mg_amp_views names"""
        return (torch.from_numpy(self.frames).to(device).contiguous(),
                torch.from_numpy(self.index).to(device).contiguous(),
                torch.from_numpy(self.time).to(device).contiguous())
