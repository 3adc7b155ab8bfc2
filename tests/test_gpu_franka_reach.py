"""GPU tests of the FrankaReachMA task (include/migym.h: mg_reach_pre, mg_reach_post, mg_reach_reset_idx;
migym/tasks/franka_reach_ma.py).

References: the reference's own post-physics step (tests/golden/trace_franka_reach_ma.npz, replayed through
mg_reach_post's state injection), its numpy restatement fed the counter RNG's host twin (tests/franka_reach_ref.py,
pyoracle.uniform), mg_osc_torques on the same state (the pre kernel runs the same device code), the reference's
_compute_osc_torques (tests/golden/osc_franka.npz) and the fp64 oracle's simulate (orc_simulate_views).

Shapes are the smallest that cross the kernels' edges: k_reach_post takes 8 envs per wave (9 envs: a second, ragged
block; 5: a partial one), k_reach_pre four arms per wave (6 and 27 arms: ragged last waves), A = 1, 2, 3, 4 agents in
the 8-lane groups, T < A and T = A.
"""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import franka_reach_ref as R
import isaacgymenvs
import parity_stats as PS
import pyoracle as O
from migym import _abi, model as M, taskdefs
from migym.dynamics import DynamicsTensors

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CONFIGS = [(2, 2, 16), (3, 3, 8), (4, 2, 8), (1, 1, 8)]


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return _abi.lib()


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.array(a)).to(DEV, dtype).contiguous()   # a copy: the golden arrays are read-only


class ReachSim:
    """a sim of N envs x A task-configured Franka arms with every tensor the three reach launches touch"""

    def __init__(self, lib, A, T, N, **env):
        self.lib, self.A, self.T, self.N, self.n = lib, A, T, N, N * A
        self.cfg = R.golden_cfg(A, T, N, **env)
        base = M.load_json(R.FRANKA_JSON)
        self.spec = spec = taskdefs.reach_spec(base)
        self.rp = taskdefs.reach_params(self.cfg, base)
        self.sp = taskdefs.sim_params(self.cfg, taskdefs.TASK_INFO["FrankaReachMA"][5], A)
        self.mnp = M.pack_model(spec)
        self.nd, self.nb, n = spec.num_dofs, len(spec.bodies), self.n
        pos, rot = taskdefs.franka_start_poses(A)
        row = torch.zeros((A, 13))
        row[:, 0:2], row[:, 2], row[:, 3:7] = pos, taskdefs.TASK_INFO["FrankaReachMA"][4], rot
        self.root = row.repeat(N, 1).to(DEV).contiguous()
        z = lambda *s, dtype=torch.float32: torch.zeros(s, device=DEV, dtype=dtype)   # noqa: E731
        self.dof, self.act, self.tgt = z(n * self.nd, 2), z(n * self.nd), z(n * self.nd)
        self.rbs, self.ncf = z(n * self.nb, 13), z(n * self.nb, 3)
        self.cube, self.init_cube = z(N, T, 13), z(N, T, 13)
        no = self.rp.num_obs
        self.actions, self.actions_out = z(n, 6), z(n, 6)
        self.obs, self.obs_clamped, self.rew = z(n, no), z(n, no), z(n)
        self.reset, self.progress = z(n, dtype=torch.long), z(n, dtype=torch.long)
        self.timeout = z(n, dtype=torch.bool)
        v = _abi.StateViews()
        v.root_states, v.dof_state = self.root.data_ptr(), self.dof.data_ptr()
        v.dof_actuation, v.dof_targets = self.act.data_ptr(), self.tgt.data_ptr()
        v.rigid_body_states, v.net_contact_forces = self.rbs.data_ptr(), self.ncf.data_ptr()
        self.views = v
        self.sim = C.c_void_p()
        _abi.check(lib.mg_sim_create(self.mnp.ctypes.data, C.byref(self.sp), n, 0, C.byref(self.sim)), lib)
        _abi.check(lib.mg_sim_bind(self.sim, C.byref(v)), lib)
        rv = _abi.ReachViews()
        rv.cube_states, rv.init_cube_states = self.cube.data_ptr(), self.init_cube.data_ptr()
        rv.dof_targets, rv.dof_actuation = self.tgt.data_ptr(), self.act.data_ptr()
        self.rv = rv
        self.noise = None
        self.out_pack = None   # (N*A, num_obs + 2) [clamped obs | rew | reset], the output gather's message rows

    def tb(self, seed=0, step=0, env_offset=0):
        b = _abi.TaskBuffers()
        b.actions, b.actions_out = self.actions.data_ptr(), self.actions_out.data_ptr()
        b.obs, b.obs_clamped, b.rew = self.obs.data_ptr(), self.obs_clamped.data_ptr(), self.rew.data_ptr()
        b.reset, b.progress, b.timeout = self.reset.data_ptr(), self.progress.data_ptr(), self.timeout.data_ptr()
        b.noise = None if self.noise is None else self.noise.data_ptr()
        b.out_pack = None if self.out_pack is None else self.out_pack.data_ptr()
        b.seed, b.step_counter, b.env_offset = seed, step, env_offset
        return b

    def stream(self):
        return torch.cuda.current_stream().cuda_stream

    def pre(self):
        b = self.tb()
        _abi.check(self.lib.mg_reach_pre(self.sim, C.byref(self.rp), C.byref(self.rv), C.byref(b), self.stream()),
                   self.lib)

    def simulate(self):
        _abi.check(self.lib.mg_sim_simulate(self.sim, self.stream()), self.lib)

    def post(self, state=None, **kw):
        b = self.tb(**kw)
        _abi.check(self.lib.mg_reach_post(self.sim, C.byref(self.rp), C.byref(self.rv), C.byref(b),
                                          None if state is None else C.byref(state), self.stream()), self.lib)

    def reset_idx(self, ids, **kw):
        b = self.tb(**kw)
        self._ids = dev(ids, torch.int32)
        _abi.check(self.lib.mg_reach_reset_idx(self.sim, C.byref(self.rp), C.byref(self.rv), C.byref(b),
                                               self._ids.data_ptr(), int(self._ids.numel()), self.stream()), self.lib)

    def state_dict(self):
        """the task state as tests/franka_reach_ref.py names it, from the device"""
        N, A, nd = self.N, self.A, self.nd
        d = self.dof.view(N, A * nd, 2).cpu().numpy()
        return dict(cube=self.cube.cpu().numpy(), init_cube=self.init_cube.cpu().numpy(), q=d[..., 0], qd=d[..., 1],
                    pos_control=self.tgt.view(N, A * nd).cpu().numpy(),
                    effort_control=self.act.view(N, A * nd).cpu().numpy(), reset=self.reset.cpu().numpy(),
                    progress=self.progress.cpu().numpy())

    def close(self):
        if self.sim is not None:
            self.lib.mg_sim_destroy(self.sim)
            self.sim = None


# ------------------------------------------------------------------------------------------------ mg_reach_post
@pytest.mark.parametrize("A,T,N", CONFIGS)
def test_post_replays_the_reference(lib, A, T, N):
    """all 6 recorded steps through the state-injection path with the recorded draws: obs, reset, progress, cubes,
    q, qd, the position and effort controls bit-equal, the reward by the 1e-4 rule; punished agents and partly done
    envs included (asserted by tests/test_franka_reach_host.py on the same file).  The gather's message rows
    (out_pack): the clip of the recorded observations, the launch's own reward bit for bit, the recorded reset."""
    g = R.golden()
    s = ReachSim(lib, A, T, N)
    no = s.rp.num_obs
    s.out_pack = torch.full((N * A, no + 2), float("nan"), device=DEV)
    nd, nb, grip, hand = s.nd, s.nb, s.rp.eef_body, s.rp.hand_body
    st0 = R.golden_state0(g, A, T, N)
    s.cube.copy_(dev(st0["cube"]))
    s.init_cube.copy_(dev(st0["init_cube"]))
    s.tgt.copy_(dev(st0["pos_control"]).view(-1))
    s.act.copy_(dev(st0["effort_control"]).view(-1))
    p = R.params_from(s.rp)
    for t in range(int(g["steps"])):
        pre = f"A{A}T{T}_s{t}_"
        # the post-simulate state in tensors of its own (not the sim's bound ones)
        inj_dof = dev(np.stack([g[pre + "q_in"], g[pre + "qd_in"]], -1).reshape(N * A * nd, 2))
        inj_rbs = torch.full((N, A, nb, 13), 7.0, device=DEV)
        inj_rbs[:, :, grip] = dev(g[pre + "eef"])
        inj_ncf = torch.full((N, A, nb, 3), 9.0, device=DEV)
        inj_ncf[:, :, hand] = dev(g[pre + "hand_force"])
        v = _abi.StateViews()
        v.dof_state, v.rigid_body_states, v.net_contact_forces = inj_dof.data_ptr(), inj_rbs.data_ptr(), \
            inj_ncf.data_ptr()
        s.reset.copy_(dev(g[pre + "reset_in"], torch.long))
        s.progress.copy_(dev(g[pre + "progress_in"], torch.long))
        s.actions.copy_(dev(g[pre + "actions"]))
        s.noise = dev(g[pre + "noise"])
        s.post(state=v, step=t)
        torch.cuda.synchronize()
        got = s.state_dict()
        d = inj_dof.view(N, A * nd, 2).cpu().numpy()
        got["q"], got["qd"] = d[..., 0], d[..., 1]
        obs = s.obs.cpu().numpy()
        assert np.array_equal(obs, g[pre + "obs"]), f"step {t}: obs"
        for k in ("reset", "progress") + R.STATE_KEYS:
            assert np.array_equal(got[k], g[pre + k]), f"step {t}: {k}"
        rew = s.rew.cpu().numpy()
        worst = np.abs(rew.astype(np.float64) - g[pre + "rew"]).max()
        print(f"A={A} T={T} step {t}: max |rew - ref| = {worst:.3g}")
        assert R.reward_close(rew, g[pre + "rew"]).all(), f"step {t}: reward off by {worst:.3g}"
        assert np.array_equal(s.obs_clamped.cpu().numpy(), np.clip(obs, -p["clip_obs"], p["clip_obs"]))
        pack = s.out_pack.cpu().numpy()
        want_obs = np.clip(g[pre + "obs"], -p["clip_obs"], p["clip_obs"])
        assert np.array_equal(pack[:, :no], want_obs), f"step {t}: out_pack's observation columns"
        assert np.array_equal(pack[:, no], rew), f"step {t}: out_pack's reward column is not rew_buf"
        assert np.array_equal(pack[:, no + 1], g[pre + "reset"].astype(np.float32)), f"step {t}: pack reset"
        tmo = (g[pre + "progress"] >= p["max_episode_length"] - 1) & (g[pre + "reset"] != 0)
        assert np.array_equal(s.timeout.cpu().numpy(), tmo)
        assert (s.dof.cpu().numpy() == 0).all(), "the sim's own DOF state is not touched under state injection"
    s.close()


@pytest.mark.parametrize("env_offset", [0, 5])
def test_device_rng_matches_its_host_twin(lib, env_offset):
    """tb.noise = NULL: one reset of (A, T, N) = (3, 3, 9) equals the restatement fed pyoracle.uniform(seed,
    env_offset + e, step, column), bit for bit; mg_reach_reset_idx draws from the | 2^62 stream"""
    A, T, N, seed, step = 3, 3, 9, 20261020, 7
    s = ReachSim(lib, A, T, N)
    p = R.params_from(s.rp)
    rng = np.random.default_rng(3)
    eef = np.zeros((N, A, 13), np.float32)
    eef[..., 0:3] = rng.uniform(-0.5, 0.5, (N, A, 3)) + (0, 0, 1.3)
    eef[..., 6] = 1.0
    s.rbs.view(N, A, s.nb, 13)[:, :, s.rp.eef_body] = dev(eef)
    for counter, manual in ((step, False), (step | (1 << 62), True)):
        noise = np.array([[O.uniform(seed, env_offset + e, counter, c) for c in range(3 * T + 9)] for e in range(N)],
                         np.float32)
        st = dict(cube=np.zeros((N, T, 13), np.float32), init_cube=np.zeros((N, T, 13), np.float32),
                  q=np.ones((N, A * 9), np.float32), qd=np.ones((N, A * 9), np.float32),
                  pos_control=np.ones((N, A * 9), np.float32), effort_control=np.ones((N, A * 9), np.float32),
                  progress=np.full(N * A, 3, np.int64), reset=np.ones(N * A, np.int64))
        for x in (s.dof, s.tgt, s.act):
            x.fill_(1.0)
        s.cube.zero_()
        s.init_cube.zero_()
        s.reset.fill_(1)
        s.progress.fill_(3)
        if manual:
            R.reset_envs(p, st, np.arange(N), noise)
            s.reset_idx(np.arange(N * A), seed=seed, step=step, env_offset=env_offset)
        else:
            R.post_step(p, st, eef, np.zeros((N, A, 3), np.float32), np.zeros((N * A, 6), np.float32), noise)
            s.post(seed=seed, step=step, env_offset=env_offset)
        torch.cuda.synchronize()
        got = s.state_dict()
        for k in ("reset", "progress") + R.STATE_KEYS:
            assert np.array_equal(got[k], st[k]), f"{'reset_idx' if manual else 'post'}: {k}"
        assert np.abs(got["cube"][:, :, 0:2]).max() <= 0.25 and (got["cube"][:, :, 2] >= 1.05).all()
        assert len(np.unique(got["cube"][:, :, 2])) == N * T, "every cube has a draw of its own"
    s.close()


def test_reset_idx_and_filter_counts_repeats(lib):
    """bincount(ids // A) >= A: a partial list resets nothing, a repeated id counts twice (ma_conventions.npz's rule)"""
    A, T, N = 3, 2, 9
    s = ReachSim(lib, A, T, N)
    s.noise = dev(np.random.default_rng(5).uniform(0, 1, (N, 3 * T + 9)).astype(np.float32))
    s.progress.fill_(4)
    s.reset.fill_(1)
    ids = [0, 1,            # env 0: two of three agents
           3, 3, 4,         # env 1: three ids, one repeated -> resets
           6, 7, 8,         # env 2: all
           26, 25, 24, 24]  # env 8 (second block): all, one twice
    s.reset_idx(ids)
    torch.cuda.synchronize()
    prog = s.progress.view(N, A).cpu().numpy()
    want = np.array([e in (1, 2, 8) for e in range(N)])
    assert np.array_equal((prog == 0).all(1), want) and np.array_equal((prog == 4).all(1), ~want)
    assert np.array_equal((s.reset.view(N, A).cpu().numpy() == 0).all(1), want)
    assert np.array_equal((s.cube[:, :, 6].cpu().numpy() == 1).all(1), want)
    s.close()


# ------------------------------------------------------------------------------------------------ mg_reach_pre
def random_arm_state(s, seed):
    rng = np.random.default_rng(seed)
    lo = np.array([x.lower for x in s.spec.nodes[1:]])
    hi = np.array([x.upper for x in s.spec.nodes[1:]])
    q = lo + (hi - lo) * rng.uniform(0.05, 0.95, (s.n, s.nd))
    qd = rng.uniform(-1, 1, (s.n, s.nd))
    s.dof.copy_(dev(np.stack([q, qd], -1).reshape(s.n * s.nd, 2)))
    s.rbs.copy_(dev(rng.uniform(-1, 1, (s.n * s.nb, 13))))
    return rng


@pytest.mark.parametrize("A,N,scale", [(2, 3, 1.0), (3, 9, 2.0)])
def test_pre_equals_osc_torques_bitwise(lib, A, N, scale):
    """6 and 27 arms (ragged last waves): columns :6 of dof_actuation are bit-equal to mg_osc_torques called with
    dpose = (clamp(a) * cmd_limit) / action_scale computed by torch on the same state; column 6 and the finger
    columns stay; actions beyond +-1 are clamped in actions_out.  (action_scale 2.0: torch divides by a Python
    scalar as a product with its reciprocal, exact for a power of two.)"""
    s = ReachSim(lib, A, A, N, actionScale=scale)
    rng = random_arm_state(s, 100 + A)
    a = rng.uniform(-1.6, 1.6, (s.n, 6)).astype(np.float32)
    s.actions.copy_(dev(a))
    s.act.fill_(7.0)
    s.pre()
    torch.cuda.synchronize()
    act = s.act.view(s.n, s.nd).cpu().numpy()
    clamped = torch.clamp(s.actions, -1.0, 1.0)
    assert np.array_equal(s.actions_out.cpu().numpy(), np.clip(a, -1, 1)) and (np.abs(a) > 1).any()
    dpose = ((clamped * dev(np.array(list(s.rp.cmd_limit), np.float32))) / scale).contiguous()
    dyn = DynamicsTensors(lib, s.sim, s.spec, s.n, DEV)
    eef_vel = s.rbs.view(s.n, s.nb, 13)[:, s.rp.eef_body, 7:13]
    u = dyn.osc_torques(dpose, eef_vel, jac_body=s.rp.jac_body, arm_dofs=7, kp=list(s.rp.kp), kd=list(s.rp.kd),
                        kp_null=list(s.rp.kp_null), kd_null=list(s.rp.kd_null),
                        default_dof_pos=list(s.rp.osc_default_dof_pos), effort_limit=list(s.rp.effort_limit))
    torch.cuda.synchronize()
    u = u.cpu().numpy()
    s.close()
    assert np.isfinite(act).all() and np.abs(u[:, :6]).max() > 1.0
    assert np.array_equal(act[:, :6], u[:, :6]), f"max diff {np.abs(act[:, :6] - u[:, :6]).max():.3g}"
    assert (act[:, 6:] == 7.0).all(), "column 6 and the finger columns must stay untouched"


def test_pre_matches_the_reference_osc(lib):
    """osc_franka.npz's 64 actors (32 envs x 2 arms) with actions chosen so that dpose is the golden's:
    max |u - u_ref64| / ref_err <= 8 on the written columns, tests/test_gpu_dynamics.py's end-to-end bound"""
    g = dict(np.load(R.HERE + "/golden/osc_franka.npz"))
    A, N = 2, 32
    s = ReachSim(lib, A, A, N)
    assert np.array_equal(s.root.cpu().numpy(), g["root_states"]), "the task's base poses are the golden's"
    s.dof.copy_(dev(np.stack([g["q"], g["qd"]], -1).reshape(-1, 2)))
    s.rbs.view(s.n, s.nb, 13)[:, s.rp.eef_body, 7:13] = dev(g["eef_vel"])
    cmd = np.array(list(s.rp.cmd_limit), np.float32)
    a = (g["dpose"] / cmd).astype(np.float32)
    assert np.abs(a).max() <= 1.0 and np.abs(a * cmd - g["dpose"]).max() <= 1e-7
    s.actions.copy_(dev(a))
    s.pre()
    torch.cuda.synchronize()
    act = s.act.view(s.n, s.nd).cpu().numpy()
    s.close()
    ratio = np.abs(act[:, :6].astype(np.float64) - g["u_ref64"][:, :6]).max() / float(g["ref_err"])
    print(f"reach pre vs the reference's fp64 OSC: max |u - u_ref64| / ref_err = {ratio:.3f} (bound 8)")
    assert np.isfinite(act).all() and ratio <= 8.0
    assert (act[:, 6:] == 0).all()


# ------------------------------------------------------------------------------------------------ physics
class ArmHost:
    """host views of the task's arms for orc_simulate_views / orc_step_flips (dof_targets and rigid_body_states
    bound, as the task binds them)"""

    def __init__(self, spec, root, dof, act, tgt):
        self.n = len(root)
        self.root, self.dof, self.act_eff, self.tgt = (np.array(x, np.float32) for x in (root, dof, act, tgt))
        self.rbs = np.zeros((self.n, len(spec.bodies), 13), np.float32)
        self.ncf = np.zeros((self.n, len(spec.bodies), 3), np.float32)

    def views(self):
        v = _abi.StateViews()
        v.root_states, v.dof_state, v.dof_actuation = O.p(self.root), O.p(self.dof), O.p(self.act_eff)
        v.dof_targets, v.rigid_body_states, v.net_contact_forces = O.p(self.tgt), O.p(self.rbs), O.p(self.ncf)
        return v


@pytest.mark.parametrize("A,N", [(2, 3), (3, 9)])
def test_task_model_physics_matches_oracle(lib, A, N):
    """one mg_sim_simulate of the task-configured arm (effort-driven arm joints, PD-driven fingers off target, no
    gravity) at 6 and 27 arms against the fp64 oracle, by the one-step rule of tests/test_gpu_tree_physics.py
    (positions 2e-4, velocities 2e-3 + 2e-3 |v|, net contact forces 1 % of the batch's largest, envs at a
    discontinuity exempt up to 5 %); the grip site's and the hand's rigid-body rows against
    pyoracle.rigid_body_states of the state the kernel left"""
    s = ReachSim(lib, A, A, N)
    spec, n, nd, nb = s.spec, s.n, s.nd, s.nb
    rng = np.random.default_rng(40 + A)
    lo = np.array([x.lower for x in spec.nodes[1:]])
    hi = np.array([x.upper for x in spec.nodes[1:]])
    q = lo + (hi - lo) * rng.uniform(0.1, 0.9, (n, nd))
    q[:, 7:] = rng.uniform(0.005, 0.03, (n, 2))            # fingers off their 0.035 target
    qd = rng.uniform(-0.5, 0.5, (n, nd))
    qd[:, 7:] = rng.uniform(-0.02, 0.02, (n, 2))
    eff = np.array([x.effort_limit for x in spec.nodes[1:]])
    act = np.zeros((n, nd))
    # arm torques within a quarter of the effort limits: at the full limits the light distal links reach the 64 rad/s
    # link-velocity cap inside this one 16.67 ms step, and at those rates the oracle's own fp32 build is 1.8e-4 rad
    # from its fp64 build, the whole position tolerance
    act[:, :7] = rng.uniform(-0.25, 0.25, (n, 7)) * eff[:7]
    tgt = np.zeros((n, nd))
    tgt[:, 7:] = 0.035
    dof0 = np.stack([q, qd], -1).astype(np.float32)
    root0 = s.root.cpu().numpy()
    s.dof.copy_(dev(dof0.reshape(n * nd, 2)))
    s.act.copy_(dev(act.reshape(-1)))
    s.tgt.copy_(dev(tgt.reshape(-1)))
    s.ncf.fill_(float("nan"))
    s.simulate()
    torch.cuda.synchronize()
    got = types.SimpleNamespace(root=s.root.cpu().numpy(), dof=s.dof.view(n, nd, 2).cpu().numpy(),
                                rbs=s.rbs.view(n, nb, 13).cpu().numpy(), ncf=s.ncf.view(n, nb, 3).cpu().numpy())
    lanes, lay = C.c_int32(), C.c_int32()
    _abi.check(lib.mg_sim_kernel_layout(s.sim, C.byref(lanes), C.byref(lay)), lib)
    s.close()
    assert lanes.value == 16, "the 10-node Franka tree runs on a 16-lane instance"
    ref = ArmHost(spec, root0, dof0, act, tgt)
    v = ref.views()
    O.lib().orc_simulate_views(s.mnp.ctypes.data, C.byref(s.sp), n, C.byref(v), 8)
    for x in (got.dof, got.rbs, got.ncf):
        assert np.isfinite(x).all()
    np.testing.assert_array_equal(got.root, root0)
    assert np.abs(got.dof[..., 0] - dof0[..., 0]).max() > 1e-3, "the step moved nothing"
    assert np.abs(got.dof[:, 7:, 1] - dof0[:, 7:, 1]).max() > 1e-2, "the finger drives did nothing"
    test = f"test_task_model_physics_matches_oracle[{A}-{N}]"
    gh = [s.rp.eef_body, s.rp.hand_body]
    checks = [("dof pos", got.dof[..., 0], ref.dof[..., 0], 2e-4, 0),
              ("dof vel", got.dof[..., 1], ref.dof[..., 1], 2e-3, 2e-3),
              ("rigid-body pose", got.rbs[:, gh, 0:3], ref.rbs[:, gh, 0:3], 2e-4, 0),
              ("rigid-body twist", got.rbs[:, gh, 7:13], ref.rbs[:, gh, 7:13], 2e-3, 2e-3),
              ("net contact forces", got.ncf, ref.ncf, 1e-2 * max(1.0, np.abs(ref.ncf).max()), 0)]
    bad = np.zeros(n, bool)
    for name, a, b, atol, rtol in checks:
        eb = PS.env_bad(a, b, atol, rtol)
        err = np.abs(a.astype(np.float64) - b)
        print(f"{test} {name}: max err {err.max():.3g}, envs outside {int(eb.sum())} / {n}")
        PS.record(test, name, a, b, envs_outside=int(eb.sum()), atol=atol, rtol=rtol)
        bad |= eb
    flags = PS.step_flags(s.mnp, s.sp, ArmHost(spec, root0, dof0, act, tgt))
    PS.assert_steps_explained(test, bad[None], flags[None], sens=None, reach_cap=PS.REACH_CAP, allow_unexplained=0.0)
    # the rows the task reads, against forward kinematics of the state the kernel left (fp32 FK of a ~1 m chain
    # against fp64: 1e-5 m, quaternions 1e-5 up to sign, twists 1e-4 (1 + |v|))
    for a in range(n):
        want = O.rigid_body_states(s.mnp, got.root[a], got.dof[a], nb)
        for b in gh:
            assert np.abs(got.rbs[a, b, 0:3] - want[b, 0:3]).max() <= 1e-5
            dq = np.minimum(np.abs(got.rbs[a, b, 3:7] - want[b, 3:7]).max(), np.abs(got.rbs[a, b, 3:7] + want[b, 3:7]).max())
            assert dq <= 1e-5
            ev = np.abs(got.rbs[a, b, 7:13] - want[b, 7:13]) / (1.0 + np.abs(want[b, 7:13]))
            assert ev.max() <= 1e-4, f"arm {a} body {b}: twist off by {ev.max():.3g}"


# ------------------------------------------------------------------------------------------------ the task
def make_env(A, T, N, seed=0):
    cfg = R.golden_cfg(A, T, N, episodeLength=150)
    return isaacgymenvs.make(seed=seed, task="FrankaReachMA", num_envs=N, sim_device=DEV, rl_device=DEV,
                             headless=True, cfg={"task": cfg})


def test_whole_step_equals_the_three_launches(lib):
    """isaacgymenvs.make(FrankaReachMA), 9 envs x 3 arms: 4 steps of random actions with injected noise equal, bit
    for bit, the same sequence driven by hand through mg_reach_pre -> mg_sim_simulate -> mg_reach_post on a second
    sim; then a forced full reset"""
    A, T, N = 3, 3, 9
    env = make_env(A, T, N)
    assert env.num_obs == 25 and env.obs_buf.shape == (27, 25) and env.num_agents == 3
    assert (env.progress_buf == 0).all() and (env.reset_buf == 0).all(), "the constructor resets every env"
    s = ReachSim(lib, A, T, N, episodeLength=150)
    s.out_pack = torch.full((N * A, 27), float("nan"), device=DEV)
    rng = np.random.default_rng(9)
    # start the hand-driven sim from the task's state after its constructor
    s.dof.copy_(env.dof_state)
    s.tgt.copy_(env.dof_targets)
    s.act.copy_(env.dof_actuation)
    s.cube.copy_(env._cubeA_state)
    s.init_cube.copy_(env._init_cubeA_state)
    s.rbs.copy_(env.rigid_body_states)
    s.ncf.copy_(env.net_contact_force_tensor)
    for t in range(4):
        noise = rng.uniform(0, 1, (N, 3 * T + 9)).astype(np.float32)
        a = rng.uniform(-1.3, 1.3, (N * A, 6)).astype(np.float32)
        if t == 2:   # envs 0 and 8 fully done, env 1 partly
            for b in (env.reset_buf, s.reset):
                b[0:A] = 1
                b[A] = 1
                b[8 * A:9 * A] = 1
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
        assert torch.equal(env.dof_state, s.dof) and torch.equal(env.dof_actuation, s.act)
        assert torch.equal(env.dof_targets, s.tgt) and torch.equal(env._cubeA_state, s.cube)
        assert torch.equal(env.rigid_body_states, s.rbs) and torch.equal(env.actions, s.actions_out)
        assert torch.isfinite(env.obs_buf).all() and extras["time_outs"].dtype == torch.bool
        want_pack = torch.cat([s.obs_clamped, s.rew.view(-1, 1), s.reset.view(-1, 1).to(torch.float32)], 1)
        assert torch.equal(s.out_pack, want_pack), f"step {t}: out_pack is not [clamped obs | rew | reset]"
        if t == 2:
            p = env.progress_buf.view(N, A).cpu().numpy()
            assert (p[[0, 8]] == 0).all() and (p[1:8] == 3).all()
            assert env.reset_buf.view(N, A)[1].tolist() == [1, 0, 0], "a partly done env keeps its flags"
    # the documented column order: [cubes 3T | eef_quat 4 | eef_pos 3 | nearest - eef 3 | others 3(A-1)]
    o = env.obs_buf.view(N, A, 25)
    eef = env._eef_state
    assert torch.equal(o[:, :, 0:9], env._cubeA_state[:, :, 0:3].reshape(N, 1, 9).expand(N, A, 9))
    assert torch.equal(o[:, :, 9:13], eef[:, :, 3:7]) and torch.equal(o[:, :, 13:16], eef[:, :, 0:3])
    st = env.states
    assert torch.equal(o[:, :, 16:19], st["cubeA_pos_min_relative"])
    assert torch.equal(o[:, 0, 19:25], torch.cat([eef[:, 1, 0:3], eef[:, 2, 0:3]], -1))
    assert torch.equal(o[:, 2, 19:25], torch.cat([eef[:, 0, 0:3], eef[:, 1, 0:3]], -1))
    assert (eef[:, :, 0:3].norm(dim=-1) < 2.5).all(), "a 0.86 m arm on a base 1.2 m from the origin"
    # a forced full reset
    env.reset_idx(torch.arange(N * A, device=DEV))
    torch.cuda.synchronize()
    assert (env.progress_buf == 0).all() and (env.reset_buf == 0).all()
    c = env._cubeA_state.cpu().numpy()
    assert (np.abs(c[:, :, 0:2]) <= 0.25).all() and (c[:, :, 2] >= 1.05 - 1e-6).all() and (c[:, :, 2] <= 1.55).all()
    q = env.dof_pos.cpu().numpy()
    assert (q >= env.franka_dof_lower_limits.cpu().numpy()).all() and (q <= env.franka_dof_upper_limits.cpu().numpy()).all()
    assert (env.dof_vel == 0).all() and (env._effort_control == 0).all() and torch.equal(env._pos_control, env._q)
    # get_env_state / set_env_state carry the cubes
    snap = env.get_env_state()
    assert "_cubeA_state" in snap and "_init_cubeA_state" in snap and "dof_targets" in snap
    env._cubeA_state.zero_()
    env.set_env_state(snap)
    assert torch.equal(env._cubeA_state, snap["_cubeA_state"])
    env.close()
    s.close()


@pytest.mark.parametrize("A,T", [(1, 1), (2, 2), (4, 2)])
def test_shapes_and_and_filter_through_the_api(lib, A, T):
    N = 5
    env = make_env(A, T, N)
    no = 10 + 3 * T + 3 * (A - 1)
    assert env.num_obs == no and env.obs_buf.shape == (N * A, no) and env._cubeA_state.shape == (N, T, 13)
    assert env.rew_buf.shape == (N * A,) and env.zero_actions().shape == (N * A, 6)
    obs, rew, reset, _ = env.step(torch.zeros((N * A, 6), device=DEV))
    assert obs["obs"].shape == (N * A, no) and torch.isfinite(obs["obs"]).all() and (env.progress_buf == 1).all()
    before = env._cubeA_state.clone()
    if A > 1:
        env.reset_idx(torch.arange(3 * A, 4 * A - 1, device=DEV))   # all but one agent of env 3
        torch.cuda.synchronize()
        assert torch.equal(env._cubeA_state, before) and (env.progress_buf == 1).all(), "a partial list resets nothing"
    env.reset_idx(torch.arange(3 * A, 4 * A, device=DEV))
    torch.cuda.synchronize()
    prog = env.progress_buf.view(N, A).cpu().numpy()
    assert (prog[3] == 0).all() and (np.delete(prog, 3, 0) == 1).all()
    changed = (env._cubeA_state != before).any(-1).any(-1).cpu().numpy()
    assert changed.tolist() == [e == 3 for e in range(N)], "exactly that env resets"
    env.close()
