"""GPU tests of the Anymal task (include/migym.h: mg_anymal_pre, mg_anymal_post, mg_anymal_reset_idx;
migym/tasks/anymal.py).

References: the reference's own pre- and post-physics step (tests/golden/trace_anymal.npz, replayed through
mg_anymal_post's state injection), its numpy restatement fed the counter RNG's host twin (tests/anymal_ref.py,
pyoracle.uniform), torch's own expression for the targets, and the fp64 oracle's simulate (orc_simulate_views) of the
task model, the first PD drive on a free-base generic instance.

Shapes are the smallest that cross the kernels' edges: k_anymal_post takes 4 envs per 64-lane block (6 envs: a second,
ragged block; 67: many blocks and a ragged tail of 3), k_anymal_pre 256 elements per block (72 and 804 elements: a
partial block, and three full ones with a partial fourth); the step kernel's 32-lane instance takes 2 actors per wave
(6 and 66 actors).
"""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import anymal_ref as R
import isaacgymenvs
import parity_stats as PS
import pyoracle as O
from migym import _abi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [6, 67]


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return _abi.lib()


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.array(a)).to(DEV, dtype).contiguous()   # a copy: the golden arrays are read-only


class AnymalSim:
    """a sim of N task-configured robots with every tensor the three Anymal launches touch"""

    def __init__(self, lib, N, cfg=None):
        self.lib, self.N = lib, N
        self.cfg = cfg or R.golden_cfg(N)
        self.spec, self.mnp, self.sp, self.ap = R.task_model(self.cfg)
        self.nb = nb = len(self.spec.bodies)
        z = lambda *s, dtype=torch.float32: torch.zeros(s, device=DEV, dtype=dtype)   # noqa: E731
        self.root = dev(np.tile(np.array(list(self.ap.base_init_state), np.float32), (N, 1)))
        self.dof, self.act, self.tgt = z(N * 12, 2), z(N * 12), z(N * 12)
        self.dof_force, self.ncf, self.commands = z(N, 12), z(N * nb, 3), z(N, 3)
        self.actions, self.actions_out = z(N, 12), z(N, 12)
        self.obs, self.obs_clamped, self.rew = z(N, 48), z(N, 48), z(N)
        self.reset, self.progress = z(N, dtype=torch.long), z(N, dtype=torch.long)
        self.timeout = z(N, dtype=torch.bool)
        v = _abi.StateViews()
        v.root_states, v.dof_state = self.root.data_ptr(), self.dof.data_ptr()
        v.dof_actuation, v.dof_targets = self.act.data_ptr(), self.tgt.data_ptr()
        v.dof_force, v.net_contact_forces = self.dof_force.data_ptr(), self.ncf.data_ptr()
        self.sim = C.c_void_p()
        _abi.check(lib.mg_sim_create(self.mnp.ctypes.data, C.byref(self.sp), N, 0, C.byref(self.sim)), lib)
        _abi.check(lib.mg_sim_bind(self.sim, C.byref(v)), lib)
        av = _abi.AnymalViews()
        av.commands, av.dof_targets = self.commands.data_ptr(), self.tgt.data_ptr()
        self.av = av
        self.noise = None
        self.out_pack = None   # (N, 50) [clamped obs | rew | reset], the output gather's message rows

    def tb(self, seed=0, step=0, env_offset=0):
        b = _abi.TaskBuffers()
        b.actions, b.actions_out = self.actions.data_ptr(), self.actions_out.data_ptr()
        b.obs, b.obs_clamped, b.rew = self.obs.data_ptr(), self.obs_clamped.data_ptr(), self.rew.data_ptr()
        b.reset, b.progress, b.timeout = self.reset.data_ptr(), self.progress.data_ptr(), self.timeout.data_ptr()
        b.noise = None if self.noise is None else self.noise.data_ptr()
        b.seed, b.step_counter, b.env_offset = seed, step, env_offset
        b.out_pack = None if self.out_pack is None else self.out_pack.data_ptr()
        return b

    def stream(self):
        return torch.cuda.current_stream().cuda_stream

    def pre(self):
        b = self.tb()
        _abi.check(self.lib.mg_anymal_pre(self.sim, C.byref(self.ap), C.byref(self.av), C.byref(b), self.stream()),
                   self.lib)

    def simulate(self):
        _abi.check(self.lib.mg_sim_simulate(self.sim, self.stream()), self.lib)

    def post(self, state=None, **kw):
        b = self.tb(**kw)
        _abi.check(self.lib.mg_anymal_post(self.sim, C.byref(self.ap), C.byref(self.av), C.byref(b),
                                           None if state is None else C.byref(state), self.stream()), self.lib)

    def reset_idx(self, ids, **kw):
        b = self.tb(**kw)
        self._ids = dev(ids, torch.int32)
        _abi.check(self.lib.mg_anymal_reset_idx(self.sim, C.byref(self.ap), C.byref(self.av), C.byref(b),
                                                self._ids.data_ptr(), int(self._ids.numel()), self.stream()), self.lib)

    def lanes(self):
        t, lay = C.c_int32(), C.c_int32()
        _abi.check(self.lib.mg_sim_kernel_layout(self.sim, C.byref(t), C.byref(lay)), self.lib)
        return t.value

    def close(self):
        if self.sim is not None:
            self.lib.mg_sim_destroy(self.sim)
            self.sim = None


# ------------------------------------------------------------------------------------------------ mg_anymal_post
@pytest.mark.parametrize("N", SIZES)
def test_post_replays_the_reference(lib, N):
    """all 6 recorded steps through the state-injection path with the recorded draws: reset, progress, timeout, the
    DOF state, root rows and commands bit-equal, observations and reward by the 1e-4 rule (measured on the MI355X:
    max |obs - ref| 4.8e-7, max |rew - ref| 1.9e-9; printed per step); every branch of the reset predicate is in the
    file (tests/test_anymal_host.py)"""
    g = R.golden()
    s = AnymalSim(lib, N)
    p = R.params_from(s.ap)
    s.commands.copy_(dev(g[f"N{N}_commands_0"]))
    worst_obs = worst_rew = 0.0
    for t in range(int(g["steps"])):
        pre = f"N{N}_s{t}_"
        # the post-simulate state in tensors of its own (not the sim's bound ones)
        inj_root, inj_dof = dev(g[pre + "root_in"]), dev(g[pre + "dof_in"].reshape(N * 12, 2))
        inj_tq, inj_ncf = dev(g[pre + "torques"]), dev(g[pre + "ncf"].reshape(N * s.nb, 3))
        v = _abi.StateViews()
        v.root_states, v.dof_state = inj_root.data_ptr(), inj_dof.data_ptr()
        v.dof_force, v.net_contact_forces = inj_tq.data_ptr(), inj_ncf.data_ptr()
        s.reset.copy_(dev(g[pre + "reset_in"], torch.long))
        s.progress.copy_(dev(g[pre + "progress_in"], torch.long))
        s.actions.copy_(dev(g[pre + "actions"]))
        s.noise = dev(g[pre + "noise"])
        s.post(state=v, step=t)
        torch.cuda.synchronize()
        assert np.array_equal(s.reset.cpu().numpy(), g[pre + "reset"]), f"step {t}: reset"
        assert np.array_equal(s.progress.cpu().numpy(), g[pre + "progress"]), f"step {t}: progress"
        tmo = (g[pre + "progress"] >= p["max_episode_length"] - 1) & (g[pre + "reset"] != 0)
        assert np.array_equal(s.timeout.cpu().numpy(), tmo), f"step {t}: timeout"
        assert np.array_equal(inj_dof.view(N, 12, 2).cpu().numpy(), g[pre + "dof"]), f"step {t}: DOF state"
        assert np.array_equal(inj_root.cpu().numpy(), g[pre + "root"]), f"step {t}: root rows"
        assert np.array_equal(s.commands.cpu().numpy(), g[pre + "commands"]), f"step {t}: commands"
        obs, rew = s.obs.cpu().numpy(), s.rew.cpu().numpy()
        e_obs = np.abs(obs.astype(np.float64) - g[pre + "obs"]).max()
        e_rew = np.abs(rew.astype(np.float64) - g[pre + "rew"]).max()
        worst_obs, worst_rew = max(worst_obs, e_obs), max(worst_rew, e_rew)
        print(f"N={N} step {t}: max |obs - ref| = {e_obs:.3g}, max |rew - ref| = {e_rew:.3g}")
        test = f"test_post_replays_the_reference[{N}] step {t}"
        PS.record(test, "obs", obs, g[pre + "obs"], atol=1e-4, rtol=1e-4)
        PS.record(test, "reward", rew, g[pre + "rew"], atol=1e-4, rtol=1e-4)
        assert R.close(obs, g[pre + "obs"]).all(), f"step {t}: obs off by {e_obs:.3g}"
        assert R.close(rew, g[pre + "rew"]).all(), f"step {t}: reward off by {e_rew:.3g}"
        assert np.array_equal((rew == 0), (g[pre + "rew"] == 0)), "the clip at 0 falls on the same envs"
        assert np.array_equal(s.obs_clamped.cpu().numpy(), np.clip(obs, -p["clip_obs"], p["clip_obs"]))
        assert (s.dof.cpu().numpy() == 0).all(), "the sim's own DOF state is not touched under state injection"
    print(f"N={N}: max |obs - ref| = {worst_obs:.3g}, max |rew - ref| = {worst_rew:.3g} over the trace")
    s.close()


# ------------------------------------------------------------------------------------------------ mg_anymal_pre
@pytest.mark.parametrize("N", SIZES)
def test_pre_equals_the_torch_expression_bitwise(lib, N):
    """actions_out = clamp(actions), targets = action_scale * actions_out + default_dof_pos: bit-equal to torch's
    evaluation of the reference's expression (anymal.py:228) and to the recorded targets"""
    g = R.golden()
    s = AnymalSim(lib, N)
    a = g[f"N{N}_s0_actions"]
    s.actions.copy_(dev(a))
    s.tgt.fill_(7.0)
    s.pre()
    torch.cuda.synchronize()
    clamped = torch.clamp(s.actions, -1.0, 1.0)
    default = dev(np.tile(np.array(list(s.ap.default_dof_pos), np.float32), (N, 1)))
    want = float(s.ap.action_scale) * clamped + default
    assert torch.equal(s.actions_out, clamped) and (np.abs(a) > 1).any()
    assert torch.equal(s.tgt.view(N, 12), want)
    assert np.array_equal(s.tgt.view(N, 12).cpu().numpy(), g[f"N{N}_s0_targets"])
    s.close()


# ------------------------------------------------------------------------------------------------ the device RNG
@pytest.mark.parametrize("env_offset", [0, 5])
def test_device_rng_matches_its_host_twin(lib, env_offset):
    """tb.noise = NULL: one reset of 9 envs equals the restatement fed pyoracle.uniform(seed, env_offset + e, step,
    column), bit for bit; mg_anymal_reset_idx draws from the | 2^62 stream"""
    N, seed, step = 9, 20261020, 7
    s = AnymalSim(lib, N)
    p = R.params_from(s.ap)
    for counter, manual in ((step, False), (step | (1 << 62), True)):
        noise = np.array([[O.uniform(seed, env_offset + e, counter, c) for c in range(27)] for e in range(N)],
                         np.float32)
        st = dict(root=np.ones((N, 13), np.float32), dof=np.ones((N, 12, 2), np.float32),
                  commands=np.zeros((N, 3), np.float32), progress=np.full(N, 3, np.int64), reset=np.ones(N, np.int64))
        s.root.fill_(1.0)
        s.dof.fill_(1.0)
        s.commands.zero_()
        s.reset.fill_(1)
        s.progress.fill_(3)
        if manual:
            R.reset_envs(p, st, np.arange(N), noise)
            s.reset_idx(np.arange(N), seed=seed, step=step, env_offset=env_offset)
        else:
            R.post_step(p, st, np.zeros((N, 12), np.float32), np.zeros((N, s.nb, 3), np.float32),
                        np.zeros((N, 12), np.float32), noise)
            s.post(seed=seed, step=step, env_offset=env_offset)
        torch.cuda.synchronize()
        who = "reset_idx" if manual else "post"
        assert np.array_equal(s.root.cpu().numpy(), st["root"]), who
        assert np.array_equal(s.dof.view(N, 12, 2).cpu().numpy(), st["dof"]), who
        assert np.array_equal(s.commands.cpu().numpy(), st["commands"]), who
        assert (s.progress == 0).all()
        assert np.array_equal(s.reset.cpu().numpy(), np.ones(N) if manual else st["reset"])
        assert len(np.unique(s.commands.cpu().numpy())) == 3 * N, "every command has a draw of its own"
    s.close()


def test_reset_idx_with_a_repeated_id(lib):
    """the listed envs reset (one of them listed twice, one in the last, ragged team block), all others stay bit for
    bit; progress = 0 and reset = 1 on the listed envs, as the reference's reset_idx leaves them"""
    N = 11
    s = AnymalSim(lib, N)
    rng = np.random.default_rng(5)
    s.noise = dev(rng.uniform(0, 1, (N, 27)).astype(np.float32))
    s.root.copy_(dev(rng.uniform(-1, 1, (N, 13))))
    s.dof.copy_(dev(rng.uniform(-1, 1, (N * 12, 2))))
    s.commands.copy_(dev(rng.uniform(-1, 1, (N, 3))))
    s.progress.fill_(4)
    before = [x.clone() for x in (s.root, s.dof.view(N, 24), s.commands, s.progress, s.reset)]
    ids = [7, 2, 7, 10, 0]
    s.reset_idx(ids)
    torch.cuda.synchronize()
    listed = np.array([e in ids for e in range(N)])
    p = R.params_from(s.ap)
    st = dict(root=before[0].cpu().numpy(), dof=before[1].cpu().numpy().reshape(N, 12, 2).copy(),
              commands=before[2].cpu().numpy(), progress=before[3].cpu().numpy(), reset=before[4].cpu().numpy())
    R.reset_envs(p, st, sorted(set(ids)), s.noise.cpu().numpy())
    st["reset"][listed] = 1
    for k, got in (("root", s.root), ("dof", s.dof.view(N, 12, 2)), ("commands", s.commands), ("progress", s.progress),
                   ("reset", s.reset)):
        assert np.array_equal(got.cpu().numpy(), st[k]), k
    for b, now in zip(before, (s.root, s.dof.view(N, 24), s.commands, s.progress, s.reset)):
        assert torch.equal(b[~torch.as_tensor(listed)], now[~torch.as_tensor(listed)]), "an unlisted env changed"
    assert (s.progress.cpu().numpy() == np.where(listed, 0, 4)).all()
    s.close()


# ------------------------------------------------------------------------------------------------ physics
@pytest.mark.parametrize("n", [R.PHYS_SMALL, R.PHYS_ACTORS])
@pytest.mark.parametrize("kind", ["standing", "fallen"])
def test_task_model_physics_matches_oracle(lib, kind, n):
    """one mg_sim_simulate of the task model (free base, 12 PD drives with an effort clamp, sphere / capsule / box
    geoms on the ground) at 6 and 66 actors against the fp64 oracle, by the one-step rule of
    tests/tree_physics_ref.compare; the 32-lane generic instance runs"""
    spec, mnp, sp, root, dof, tgt, ref = R.physics_states(kind)
    s = AnymalSim(lib, n, cfg=R.task_cfg(n))
    assert s.lanes() == 32, "the 13-node, 37-geom quadruped runs on the (32, 32, 48, 48, 192) instance"
    s.root.copy_(dev(root[:n]))
    s.dof.copy_(dev(dof[:n].reshape(n * 12, 2)))
    s.tgt.copy_(dev(tgt[:n].reshape(-1)))
    s.ncf.fill_(float("nan"))   # every row must be written
    s.dof_force.fill_(float("nan"))
    s.simulate()
    torch.cuda.synchronize()
    got = types.SimpleNamespace(root=s.root.cpu().numpy(), dof=s.dof.view(n, 12, 2).cpu().numpy(),
                                dof_force=s.dof_force.cpu().numpy(), ncf=s.ncf.view(n, s.nb, 3).cpu().numpy())
    s.close()
    p = R.params_from(s.ap)
    rows = np.linalg.norm(ref.ncf[:n][:, [p["base"]] + p["knees"]], axis=-1)
    if kind == "fallen":
        assert (rows[:, 1:] > 0).any(), "no thigh touches in the fallen states"
        assert n < R.PHYS_ACTORS or (rows[:, 0] > 0).any(), "no base touches in the fallen states"
        assert n < R.PHYS_ACTORS or (np.abs(ref.dof_force[:n]) >= 80.0 - 1e-3).any(), "no drive saturates"
    else:
        loaded = (np.linalg.norm(ref.ncf[:n], axis=-1) > 1).sum(1)   # a random target may lift a foot for a step
        assert (rows == 0).all() and np.median(loaded) >= 2, "the robots stand on their feet"
    assert np.abs(got.dof_force).max() <= 80.0 + 1e-3, "the effort clamp"
    R.compare_step(f"test_task_model_physics_matches_oracle[{kind}-{n}]", kind, n, got)


# ------------------------------------------------------------------------------------------------ the task
def make_env(N, seed=0, cfg=None):
    return isaacgymenvs.make(seed=seed, task="Anymal", num_envs=N, sim_device=DEV, rl_device=DEV, headless=True,
                             cfg={"task": cfg or R.golden_cfg(N)})


def test_whole_step_equals_the_three_launches(lib):
    """isaacgymenvs.make(Anymal), 67 envs: 8 steps of random actions with injected noise equal, bit for bit, the same
    sequence driven by hand through mg_anymal_pre -> mg_sim_simulate -> mg_anymal_post on a second sim; resets come
    from the first step (reset_buf starts at ones), from forced flags and from the 12-step episode limit"""
    N = 67
    env = make_env(N)
    assert env.num_obs == 48 and env.num_actions == 12 and env.obs_buf.shape == (N, 48) and env.num_agents == 1
    assert (env.progress_buf == 0).all() and (env.reset_buf == 1).all(), "the constructor resets every env"
    assert env.contact_forces.shape == (N, 13, 3) and env.torques.shape == (N, 12) and env.commands.shape == (N, 3)
    assert env.knee_indices.tolist() == [2, 5, 8, 11] and env.feet_indices.tolist() == [3, 6, 9, 12]
    assert env.base_index == 0 and (env.Kp, env.Kd) == (85.0, 2.0) and env.max_episode_length == 12
    assert env.dof_names[:3] == ["LF_HAA", "LF_HFE", "LF_KFE"] and env.gravity_vec.shape == (N, 3)
    assert torch.equal(env.commands_x, env.commands[:, 0])
    assert env.commands_yaw.data_ptr() == env.commands[:, 2].data_ptr()
    s = AnymalSim(lib, N)
    assert s.lanes() == 32
    s.out_pack = torch.full((N, 50), float("nan"), device=DEV)
    rng = np.random.default_rng(9)
    for a, b in ((s.root, env.root_states), (s.dof, env.dof_state), (s.commands, env.commands),
                 (s.reset, env.reset_buf), (s.progress, env.progress_buf)):
        a.copy_(b)
    saw_reset = saw_timeout = False
    for t in range(8):
        noise = rng.uniform(0, 1, (N, 27)).astype(np.float32)
        a = rng.uniform(-1.3, 1.3, (N, 12)).astype(np.float32)
        if t == 3:
            for b in (env.reset_buf, s.reset):
                b[0:5] = 1
                b[64:67] = 1
            for b in (env.progress_buf, s.progress):
                b[10:20] = 9    # these reach max_episode_length - 1 at the next step
        env.set_reset_noise(dev(noise))
        obs, rew, reset, extras = env.step(dev(a))
        s.noise = dev(noise)
        s.actions.copy_(dev(a))
        s.pre()
        s.simulate()
        s.post(step=t)
        torch.cuda.synchronize()
        assert torch.equal(env.obs_buf, s.obs) and torch.equal(obs["obs"], s.obs_clamped), f"step {t}"
        assert torch.equal(env.rew_buf, s.rew) and torch.equal(env.reset_buf, s.reset)
        assert torch.equal(env.progress_buf, s.progress) and torch.equal(env.timeout_buf, s.timeout)
        assert torch.equal(env.dof_state, s.dof) and torch.equal(env.root_states, s.root)
        assert torch.equal(env.dof_targets, s.tgt) and torch.equal(env.commands, s.commands)
        assert torch.equal(env.torques, s.dof_force) and torch.equal(env.net_contact_force_tensor, s.ncf)
        assert torch.equal(env.actions, s.actions_out) and torch.equal(rew, s.rew) and torch.equal(reset, s.reset)
        assert torch.isfinite(env.obs_buf).all() and extras["time_outs"].dtype == torch.bool
        want_pack = torch.cat([s.obs_clamped, s.rew.view(N, 1), s.reset.view(N, 1).to(torch.float32)], 1)
        assert torch.equal(s.out_pack, want_pack), f"step {t}: out_pack is not [clamped obs | rew | reset]"
        saw_reset |= bool((env.progress_buf == 0).any()) and t > 0
        saw_timeout |= bool(extras["time_outs"].any())
    assert saw_reset and saw_timeout and (env.progress_buf > 0).any()
    assert torch.equal(env.obs_buf[:, 36:48], env.actions) and env.torques.abs().max() > 1.0
    env.close()
    s.close()


def test_rollout_facts_through_make(lib):
    """64 envs from injected reset draws, 50 zero-action steps through the task: finite, no base or thigh net contact
    force above 1 and so no reset, at most 48 contact candidates at every step (counted by the fp64 oracle on the GPU's
    states: the rollout stays clear of the truncation at max_contacts), the drive torques within the effort limit, the
    robots standing at the height the fp64 oracle settles at (tests/test_anymal_host.py asserts the same three facts
    of the oracle's own rollout)"""
    N = 64
    env = make_env(N, cfg=R.task_cfg(N))
    p = R.params_from(env.anymal_params)
    _, _, noise = R.reset_state(p, N, 11)
    env.set_reset_noise(dev(noise))
    zero = torch.zeros((N, 12), device=DEV)
    _, mnp, sp, _ = R.task_model(env.cfg)

    def candidates():   # the fp64 oracle's contact candidates of the GPU's states (capacity: max_contacts = 48)
        return R.num_candidates(mnp, sp, env.root_states.cpu().numpy(), env.dof_state.view(N, 12, 2).cpu().numpy()).max()

    most = 0
    for t in range(51):   # the first step applies the constructor's reset flags, with the injected draws
        most = max(most, candidates())   # the states each simulate starts from ...
        obs, rew, reset, _ = env.step(zero)
        if t == 0:
            env.set_reset_noise(None)
        torch.cuda.synchronize()
        nrm = env.contact_forces[:, [0, 2, 5, 8, 11]].norm(dim=-1)
        assert torch.isfinite(obs["obs"]).all() and torch.isfinite(env.root_states).all(), f"step {t}"
        assert nrm.max() <= 1.0 and (reset == 0).all(), f"step {t}: a base or thigh force of {nrm.max():.3g}"
    most = max(most, candidates())       # ... and the one the last step left
    print(f"most contact candidates {most}")
    assert most <= 48 == sp.max_contacts
    z = env.root_states[:, 2]
    print(f"final base z {z.min():.3f}..{z.max():.3f}, max |torque| {env.torques.abs().max():.3g}")
    assert (z > 0.4).all() and (z < 0.62).all() and env.torques.abs().max() <= 80.0 + 1e-3
    assert (env.progress_buf == 50).all() and (env.contact_forces[:, [3, 6, 9, 12]].norm(dim=-1) > 1).sum(1).min() >= 2
    assert (env.rew_buf >= 0).all() and torch.equal(env.dof_targets.view(N, 12), env.default_dof_pos)
    env.close()


def test_reset_done_and_env_state_resume(lib):
    """reset_done resets the done envs now; get_env_state / set_env_state (commands and dof_targets included) resume a
    rollout bit for bit"""
    N = 67
    env = make_env(N, seed=3)
    rng = np.random.default_rng(4)
    acts = [dev(rng.uniform(-1, 1, (N, 12)).astype(np.float32)) for _ in range(6)]
    for a in acts[:2]:
        env.step(a)
    env.reset_buf[5] = 1
    env.reset_buf[66] = 1
    before = env.dof_state.clone()
    obs0 = env.obs_buf.clone()
    _, done = env.reset_done()
    torch.cuda.synchronize()
    done = done.cpu().numpy()
    assert {5, 66} <= set(done.tolist())
    changed = (env.dof_state.view(N, 24) != before.view(N, 24)).any(1).cpu().numpy()
    assert np.array_equal(np.nonzero(changed)[0], done) and (env.progress_buf[done] == 0).all()
    assert torch.equal(env.root_states[done], env.initial_root_states[done]) and torch.equal(env.obs_buf, obs0)
    snap = env.get_env_state()
    for k in ("commands", "dof_targets", "root_states", "dof_state", "net_contact_force_tensor", "dof_force_tensor",
              "progress_buf", "reset_buf", "control_steps"):
        assert k in snap, k
    outs = []
    for a in acts[2:]:
        o, r, d, _ = env.step(a)
        outs.append((o["obs"].clone(), r.clone(), d.clone(), env.commands.clone(), env.dof_state.clone()))
    env.commands.zero_()
    env.dof_targets.fill_(3.0)
    env.set_env_state(snap)
    assert torch.equal(env.commands, snap["commands"]) and torch.equal(env.dof_targets, snap["dof_targets"])
    for a, want in zip(acts[2:], outs):
        o, r, d, _ = env.step(a)
        got = (o["obs"], r, d, env.commands, env.dof_state)
        for x, y in zip(got, want):
            assert torch.equal(x, y), "the resumed rollout differs"
    with pytest.raises(ValueError, match="reset noise"):
        env.set_reset_noise(torch.zeros((N, 26), device=DEV))
    env.close()
