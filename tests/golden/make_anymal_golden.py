#!/usr/bin/env python3
"""Anymal's pre- and post-physics step from the reference's own methods.

Run in the build container only (needs the reference checkout, MIGYM_REFERENCE):

    python tests/golden/make_anymal_golden.py

The task layer of ``Anymal`` (isaacgymenvs/tasks/anymal.py) is plain torch, so its methods are called here
unmodified, bound to a stand-in ``self`` that holds only the attributes they read: ``pre_physics_step`` (226-229),
``post_physics_step`` (231-239) and through it ``reset_idx`` (278-304), ``compute_observations`` (257-276) ->
``compute_anymal_observations`` (354-386) and ``compute_reward`` (241-255) -> ``compute_anymal_reward`` (311-351).
``gym`` is a stand-in: ``set_actor_root_state_tensor_indexed`` copies the listed rows into ``root_states`` at once
(the project's convention for indexed sets, FakeGym in make_traces.py), ``set_dof_position_target_tensor`` keeps the
targets it is handed, every other call is a no-op; ``gymtorch.unwrap_tensor`` is the identity; the module's
``torch_rand_float`` is replaced by a recorder that evaluates the same expression, ``(upper - lower) * u + lower``, on
a recorded ``u = torch.rand(shape)`` (make_traces.RandRecorder).  The constants come from the reference's
cfg/task/Anymal.yaml, through the expressions of ``Anymal.__init__`` (93-100) with ``dt`` a C float, as
``gymapi.SimParams.dt`` is; ``episodeLength_s`` is EPISODE_LENGTH_S, so that time-outs occur within six steps.

Two traces, N = 6 and N = 67 envs, 6 control steps each.  Before each step the post-simulate state is written the
way gym.simulate would leave it -- seeded random unit base quaternions, base positions and twists, DOF states, torques
of up to 80 N m, net contact force rows (feet always loaded; per env none, or the base, or one thigh, with a norm just
under or just over 1) -- with seeded random actions (some beyond the clip; VecTask.step's clamp is applied before they
are handed over) and a reset mask of done and not-done envs on top of what the previous step's reward set;
``progress`` starts so that some envs reach max_episode_length - 1.  Recorded: the inputs, the draws in the (N, 27)
layout [positions_offset 12 | velocities 12 | command x | y | yaw] (zero rows for envs that did not reset), and every
output after each step.  The DOF columns are in this build's DOF order (the loader's: LF, RF, LH, RH x HAA, HFE, KFE);
gym's own order is not observable here.  The fixture holds data only: tests/golden/trace_anymal.npz.

Preconditions are asserted, so a comparison against this file cannot hide a flip: no base or thigh contact norm lies
within 1e-3 of 1; no reward lies within 1e-4 of the clip at 0 (the torques of an env whose reward would are redrawn
until it does not); every branch of the reset predicate fires at least once in each trace: base, knee,
time-out, none.
"""
import os
import sys
import types

import numpy as np
import torch
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _refshim  # noqa: E402

_refshim.install()
import isaacgymenvs.tasks.anymal as ref  # noqa: E402
from isaacgymenvs.tasks.anymal import Anymal  # noqa: E402

ref.gymtorch.unwrap_tensor = lambda t: t

SIZES = [6, 67]
STEPS = 6
EPISODE_LENGTH_S = 0.24     # 12 control steps
DT = 0.02
NB, BASE, KNEES = 13, 0, [2, 5, 8, 11]    # tests/golden/anymal_c.json: base, {LF,RF,LH,RH}_{HIP,THIGH,SHANK}
FEET = [3, 6, 9, 12]
DOF_NAMES = [leg + "_" + j for leg in ("LF", "RF", "LH", "RH") for j in ("HAA", "HFE", "KFE")]


def load_cfg():
    with open(os.path.join(_refshim.REF, "isaacgymenvs/cfg/task/Anymal.yaml")) as f:
        txt = f.read()
    # the ${...} interpolations sit in keys this generator does not read
    return yaml.safe_load(txt)


class Gym:
    def __init__(self, s):
        self.s, self.targets = s, None

    def set_actor_root_state_tensor_indexed(self, sim, data, idx, n):
        idx = idx.long()
        self.s.root_states[idx] = data[idx]

    def set_dof_position_target_tensor(self, sim, t):
        self.targets = t.clone()

    def __getattr__(self, name):
        return lambda *a, **k: None


class RandRecorder:
    """the module's torch_rand_float, keeping each draw's raw U(0,1)"""

    def __init__(self):
        self.draws = []

    def __call__(self, lower, upper, shape, device):
        u = torch.rand(*shape, device=device)
        self.draws.append(u.clone())
        return (upper - lower) * u + lower


def stand_in(N, cfg):
    env, learn = cfg["env"], cfg["env"]["learn"]
    dt = float(np.float32(DT))     # self.dt = self.sim_params.dt (anymal.py:93): a C float
    s = types.SimpleNamespace(num_envs=N, device="cpu", sim=None, randomize=False, num_dof=12, num_actions=12,
                              lin_vel_scale=learn["linearVelocityScale"], ang_vel_scale=learn["angularVelocityScale"],
                              dof_pos_scale=learn["dofPositionScale"], dof_vel_scale=learn["dofVelocityScale"],
                              action_scale=env["control"]["actionScale"],
                              command_x_range=env["randomCommandVelocityRanges"]["linear_x"],
                              command_y_range=env["randomCommandVelocityRanges"]["linear_y"],
                              command_yaw_range=env["randomCommandVelocityRanges"]["yaw"])
    s.gym = Gym(s)
    for name in ("pre_physics_step", "post_physics_step", "reset_idx", "compute_observations", "compute_reward"):
        setattr(s, name, types.MethodType(getattr(Anymal, name), s))
    s.rew_scales = {"lin_vel_xy": learn["linearVelocityXYRewardScale"], "ang_vel_z": learn["angularVelocityZRewardScale"],
                    "torque": learn["torqueRewardScale"]}
    for k in s.rew_scales:
        s.rew_scales[k] *= dt                                        # anymal.py:99-100
    s.max_episode_length = int(EPISODE_LENGTH_S / dt + 0.5)          # anymal.py:95
    b = env["baseInitState"]
    s.base_init_state = b["pos"] + b["rot"] + b["vLinear"] + b["vAngular"]
    s.root_states = torch.zeros(N, 13)
    s.dof_state = torch.zeros(N * 12, 2)
    s.dof_pos = s.dof_state.view(N, 12, 2)[..., 0]
    s.dof_vel = s.dof_state.view(N, 12, 2)[..., 1]
    s.contact_forces = torch.zeros(N * NB, 3).view(N, -1, 3)
    s.torques = torch.zeros(N * 12).view(N, 12)
    s.commands = torch.zeros(N, 3)
    s.commands_y = s.commands.view(N, 3)[..., 1]
    s.commands_x = s.commands.view(N, 3)[..., 0]
    s.commands_yaw = s.commands.view(N, 3)[..., 2]
    s.default_dof_pos = torch.zeros_like(s.dof_pos)
    for i, name in enumerate(DOF_NAMES):
        s.default_dof_pos[:, i] = env["defaultJointAngles"][name]    # anymal.py:134-137
    s.initial_root_states = s.root_states.clone()
    s.initial_root_states[:] = torch.tensor(s.base_init_state, dtype=torch.float)
    s.gravity_vec = torch.tensor([0.0, 0.0, -1.0]).repeat((N, 1))     # get_axis_params(-1., 2)
    s.actions = torch.zeros(N, 12)
    s.knee_indices = torch.tensor(KNEES, dtype=torch.long)
    s.base_index = BASE
    s.obs_buf = torch.zeros(N, 48)
    s.rew_buf = torch.zeros(N)
    s.reset_buf = torch.ones(N, dtype=torch.long)
    s.progress_buf = torch.zeros(N, dtype=torch.long)
    return s


def f32(a):
    return np.asarray(a, np.float32)


def raw_reward(s, root, cmd, tq):
    """compute_anymal_reward's sum before the clip, in float64 (a precondition check, not the recorded value)"""
    q, v, w = root[:, 3:7].astype(np.float64), root[:, 7:10].astype(np.float64), root[:, 10:13].astype(np.float64)

    def rot_inv(q, v):
        qv, qw = q[:, :3], q[:, 3:4]
        return v * (2 * qw ** 2 - 1) - np.cross(qv, v) * qw * 2 + qv * (qv * v).sum(1, keepdims=True) * 2

    lin, ang = rot_inv(q, v), rot_inv(q, w)
    le = ((cmd[:, :2] - lin[:, :2]) ** 2).sum(1)
    ae = (cmd[:, 2] - ang[:, 2]) ** 2
    return np.exp(-le / 0.25) * s.rew_scales["lin_vel_xy"] + np.exp(-ae / 0.25) * s.rew_scales["ang_vel_z"] + \
        (tq.astype(np.float64) ** 2).sum(1) * s.rew_scales["torque"]


def run(N, cfg, rng):
    s = stand_in(N, cfg)
    tag = f"N{N}_"
    out = {}
    M = s.max_episode_length
    env = cfg["env"]
    lo = np.array([env["randomCommandVelocityRanges"][k][0] for k in ("linear_x", "linear_y", "yaw")])
    hi = np.array([env["randomCommandVelocityRanges"][k][1] for k in ("linear_x", "linear_y", "yaw")])
    s.commands[:] = torch.from_numpy(f32(rng.uniform(lo, hi, (N, 3))))
    out[tag + "commands_0"] = s.commands.numpy().copy()
    s.reset_buf[:] = 0
    s.progress_buf[:] = torch.from_numpy(rng.integers(M - 8, M - 2, N))
    s.progress_buf[2] = M - 4       # env 2 is never reset below: it times out from the third step on
    default = s.default_dof_pos.numpy()
    seen = dict(base=False, knee=False, timeout=False, none=False)
    for t in range(STEPS):
        # what gym.simulate leaves
        root = np.zeros((N, 13), np.float32)
        root[:, 0:2] = rng.uniform(-3, 3, (N, 2))
        root[:, 2] = rng.uniform(0.2, 0.7, N)
        quat = rng.normal(0, 1, (N, 4))
        root[:, 3:7] = quat / np.linalg.norm(quat, axis=-1, keepdims=True)
        slow = rng.random(N) < 0.5      # half the envs move slowly: their tracking rewards are not negligible
        root[:, 7:13] = rng.uniform(-2, 2, (N, 6)) * np.where(slow, 0.15, 1.0)[:, None]
        dof = np.zeros((N, 12, 2), np.float32)
        dof[..., 0] = default + rng.uniform(-0.5, 0.5, (N, 12))
        dof[..., 1] = rng.uniform(-5, 5, (N, 12))
        tq = f32(rng.uniform(-80, 80, (N, 12)) * rng.uniform(0, 1, (N, 1)))
        tq[rng.integers(0, N), rng.integers(0, 12)] = 80.0       # a saturated drive
        ncf = np.zeros((N, NB, 3), np.float32)
        ncf[:, FEET] = rng.uniform(-30, 200, (N, 4, 3))
        kind = (np.arange(N) + t) % 5      # 0: none | 1: base under | 2: base over | 3: one thigh under | 4: over
        direc = rng.normal(0, 1, (N, 3))
        direc /= np.linalg.norm(direc, axis=-1, keepdims=True)
        mag = np.where((kind == 1) | (kind == 3), rng.uniform(0.5, 0.998, N), rng.uniform(1.002, 50.0, N))
        body = np.where(kind <= 2, BASE, np.array(KNEES)[rng.integers(0, 4, N)])
        for e in np.nonzero(kind)[0]:
            ncf[e, body[e]] = direc[e] * mag[e]
        norms = np.linalg.norm(ncf[:, [BASE] + KNEES].astype(np.float64), axis=-1)
        assert (np.abs(norms - 1.0) > 1e-3).all(), "a contact norm within 1e-3 of 1"
        actions = f32(rng.uniform(-1.5, 1.5, (N, 12)))
        forced = (rng.random(N) < 0.4).astype(np.int64)
        reset_in = np.maximum(s.reset_buf.numpy(), forced)
        reset_in[0] = 1
        reset_in[2] = 0
        s.root_states[:] = torch.from_numpy(root)
        s.dof_state[:] = torch.from_numpy(dof.reshape(N * 12, 2))
        s.contact_forces[:] = torch.from_numpy(ncf)
        s.reset_buf[:] = torch.from_numpy(reset_in)
        progress_in = s.progress_buf.numpy().copy()
        cmd_in = s.commands.numpy().copy()
        ids = np.nonzero(reset_in)[0]
        # the reward's distance from its clip is known only after the reset draws: run the step on a copy of the RNG
        # state first, redraw the torques of the envs that would land within 2e-4 of 0, until none does
        state = torch.get_rng_state()
        for attempt in range(50):
            torch.set_rng_state(state)
            s.root_states[:] = torch.from_numpy(root)
            s.dof_state[:] = torch.from_numpy(dof.reshape(N * 12, 2))
            s.commands[:] = torch.from_numpy(cmd_in)
            s.reset_buf[:] = torch.from_numpy(reset_in)
            s.progress_buf[:] = torch.from_numpy(progress_in)
            s.torques[:] = torch.from_numpy(tq)
            clamped = torch.clamp(torch.from_numpy(actions), -env["clipActions"], env["clipActions"])  # VecTask.step
            s.pre_physics_step(clamped)
            rec = RandRecorder()
            ref.torch_rand_float = rec
            s.post_physics_step()
            raw = raw_reward(s, s.root_states.numpy(), s.commands.numpy().astype(np.float64), tq)
            close = np.abs(raw) < 2e-4
            if not close.any():
                break
            k = int(close.sum())
            tq[close] = f32(rng.uniform(-80, 80, (k, 12)) * rng.uniform(0.1, 1, (k, 1)))
        assert not close.any(), "a reward within 1e-4 of the clip at 0"
        rew = s.rew_buf.numpy()
        assert ((rew == 0) == (raw < 0)).all()
        noise = np.zeros((N, 27), np.float32)
        assert [tuple(d.shape) for d in rec.draws] == [(len(ids), 12), (len(ids), 12)] + [(len(ids), 1)] * 3
        noise[ids, 0:12], noise[ids, 12:24] = rec.draws[0].numpy(), rec.draws[1].numpy()
        for c in range(3):
            noise[ids, 24 + c] = rec.draws[2 + c].numpy()[:, 0]
        prog = s.progress_buf.numpy()
        fb, fk, ft = norms[:, 0] > 1, (norms[:, 1:] > 1).any(1), prog >= M - 1
        assert np.array_equal(s.reset_buf.numpy() != 0, fb | fk | ft)
        seen["base"] |= bool((fb & ~fk & ~ft).any())
        seen["knee"] |= bool((fk & ~fb & ~ft).any())
        seen["timeout"] |= bool((ft & ~fb & ~fk).any())
        seen["none"] |= bool((~fb & ~fk & ~ft).any())
        assert (reset_in != 0).any() and (reset_in == 0).any()
        pre = f"{tag}s{t}_"
        out.update({pre + "root_in": root, pre + "dof_in": dof, pre + "torques": tq, pre + "ncf": ncf,
                    pre + "actions": actions, pre + "reset_in": reset_in, pre + "progress_in": progress_in,
                    pre + "noise": noise, pre + "targets": s.gym.targets.numpy().copy(),
                    pre + "obs": s.obs_buf.numpy().copy(), pre + "rew": rew.copy(),
                    pre + "reset": s.reset_buf.numpy().copy(), pre + "progress": prog.copy(),
                    pre + "root": s.root_states.numpy().copy(), pre + "dof": s.dof_state.numpy().reshape(N, 12, 2).copy(),
                    pre + "commands": s.commands.numpy().copy()})
    assert all(seen.values()), f"a branch of the reset predicate never fired alone: {seen}"
    return out, s


def main():
    torch.manual_seed(20261020)
    rng = np.random.default_rng(20261020)
    cfg = load_cfg()
    out = {"sizes": np.array(SIZES, np.int32), "steps": np.int32(STEPS), "episode_length_s": np.float64(EPISODE_LENGTH_S)}
    for N in SIZES:
        o, s = run(N, cfg, rng)
        out.update(o)
    out.update({"max_episode_length": np.int32(s.max_episode_length),
                "rew_scales": f32([s.rew_scales[k] for k in ("lin_vel_xy", "ang_vel_z", "torque")]),
                "default_dof_pos": s.default_dof_pos.numpy()[0].copy(),
                "base_init_state": f32(s.base_init_state)})
    path = os.path.join(HERE, "trace_anymal.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
