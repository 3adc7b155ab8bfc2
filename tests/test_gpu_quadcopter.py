"""The Quadcopter task on the GPU (mg_quadcopter_pre / mg_sim_simulate with link forces / mg_quadcopter_post;
DESIGN.md §14), against the reference's own trace (tests/golden/trace_quadcopter.npz) and the oracle.

  * pre and post replay the traces: integers, DOF state, root rows, thrusts, targets and forces bit for bit, floats
    within the project's 1e-4 (the measured maximum is printed); the gather's message rows (out_pack) equal
    [clamped obs | rew | reset] of the same launch bit for bit.
  * The device RNG equals its host twin at env_offset 0 and 5.
  * reset_idx with a repeated id changes the listed envs only.
  * Quadcopter.step equals the three launches by hand, bit for bit, over 8 steps with resets at N = 67; a caller's
    force tensor bound through apply_rigid_body_force_tensors takes the place of env.forces.
  * reset_done and set_env_state resume bit for bit.
  * Hover: targets 0, each thrust held at M g / 4, upright at rest, 20 steps.
  * A rollout through make() stays finite and the oracle counts no contact candidate on the GPU's states.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import isaacgymenvs
import pyoracle as O
import quadcopter_ref as R
from migym import _abi, model as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return _abi.lib()


def dev(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), device=DEV, dtype=dtype).contiguous()


class QuadSim:
    """a sim of N task-configured quadcopters with every tensor the three launches touch"""

    def __init__(self, lib, N, cfg=None):
        self.lib, self.N = lib, N
        self.cfg = cfg or R.golden_cfg(N)
        self.spec, self.mnp, self.sp, self.qp = R.task_model(self.cfg)
        z = lambda *s, dtype=torch.float32: torch.zeros(s, device=DEV, dtype=dtype)   # noqa: E731
        self.root, self.dof = dev(np.tile(np.array(list(self.qp.init_root), F), (N, 1))), z(N, 8, 2)
        self.tgt, self.thr, self.frc = z(N, 8), z(N, 4), z(N, 9, 3)
        self.act, self.act_out, self.obs, self.obs_c = z(N, 12), z(N, 12), z(N, 21), z(N, 21)
        self.rew, self.reset, self.progress = z(N), z(N, dtype=torch.int64), z(N, dtype=torch.int64)
        self.timeout = z(N, dtype=torch.bool)
        self.h = C.c_void_p()
        _abi.check(lib.mg_sim_create(self.mnp.ctypes.data, C.byref(self.sp), N, 0, C.byref(self.h)), lib)
        v = _abi.StateViews()
        v.root_states, v.dof_state, v.dof_targets = self.root.data_ptr(), self.dof.data_ptr(), self.tgt.data_ptr()
        v.rb_forces, v.rb_force_space = self.frc.data_ptr(), _abi.MG_LOCAL_SPACE
        _abi.check(lib.mg_sim_bind(self.h, C.byref(v)), lib)
        _abi.check(lib.mg_sim_set_link_forces(self.h, 1), lib)
        self.qv = _abi.QuadcopterViews()
        self.qv.thrusts, self.qv.dof_targets, self.qv.forces = self.thr.data_ptr(), self.tgt.data_ptr(), self.frc.data_ptr()
        self.noise = None
        self.out_pack = None   # (N, 23) [clamped obs | rew | reset], the output gather's message rows

    def tb(self, step=0, seed=0, env_offset=0):
        b = _abi.TaskBuffers()
        b.actions, b.actions_out, b.obs, b.obs_clamped = self.act.data_ptr(), self.act_out.data_ptr(), \
            self.obs.data_ptr(), self.obs_c.data_ptr()
        b.rew, b.reset, b.progress, b.timeout = self.rew.data_ptr(), self.reset.data_ptr(), self.progress.data_ptr(), \
            self.timeout.data_ptr()
        b.noise, b.out_pack = _abi.ptr(self.noise), _abi.ptr(self.out_pack)
        b.seed, b.step_counter, b.env_offset = seed, step, env_offset
        return b

    def stream(self):
        return torch.cuda.current_stream().cuda_stream

    def pre(self, **kw):
        _abi.check(self.lib.mg_quadcopter_pre(self.h, C.byref(self.qp), C.byref(self.qv), C.byref(self.tb(**kw)),
                                              self.stream()), self.lib)

    def simulate(self):
        _abi.check(self.lib.mg_sim_simulate(self.h, self.stream()), self.lib)

    def post(self, state=None, **kw):
        _abi.check(self.lib.mg_quadcopter_post(self.h, C.byref(self.qp), C.byref(self.qv), C.byref(self.tb(**kw)),
                                               None if state is None else C.byref(state), self.stream()), self.lib)

    def reset_idx(self, ids, **kw):
        ids = dev(ids, torch.int32)
        _abi.check(self.lib.mg_quadcopter_reset_idx(self.h, C.byref(self.qp), C.byref(self.qv), C.byref(self.tb(**kw)),
                                                    ids.data_ptr(), int(ids.numel()), self.stream()), self.lib)
        torch.cuda.synchronize()

    def close(self):
        self.lib.mg_sim_destroy(self.h)


def np_(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------------------------------------ the trace
@pytest.mark.parametrize("N", [6, 67])
def test_pre_and_post_replay_the_reference_trace(lib, N):
    g = R.golden()
    s = QuadSim(lib, N)
    s.out_pack = torch.full((N, 23), float("nan"), device=DEV)
    for name, t in (("dof_position_targets", s.tgt), ("thrusts", s.thr), ("forces", s.frc), ("root_states", s.root),
                    ("dof_states", s.dof)):
        t.copy_(dev(g[f"N{N}_{name}_0"]))
    worst = 0.0
    injected_root, injected_dof = torch.zeros_like(s.root), torch.zeros_like(s.dof)
    for t in range(int(g["steps"])):
        k = lambda name: g[f"N{N}_t{t}_{name}"]   # noqa: E731
        s.act.copy_(dev(k("actions")))
        s.reset.copy_(dev(k("reset_in"), torch.int64))
        s.progress.copy_(dev(k("progress_in"), torch.int64))
        s.noise = dev(k("noise"))
        s.pre(step=t)
        torch.cuda.synchronize()
        for name, got in (("dof_position_targets", s.tgt), ("thrusts", s.thr), ("forces", s.frc),
                          ("root_states", s.root), ("dof_states", s.dof), ("reset_buf", s.reset),
                          ("progress_buf", s.progress)):
            np.testing.assert_array_equal(np_(got), k("pre_" + name), err_msg=f"step {t}: {name} after pre")
        np.testing.assert_array_equal(np_(s.act_out), np.clip(k("actions"), -1.0, 1.0))
        # the post-simulate state: through the bound tensors on even steps, injected (physics-free replay) on odd ones
        if t % 2 == 0:
            s.root.copy_(dev(k("sim_root_states")))
            s.dof.copy_(dev(k("sim_dof_states")))
            s.post(step=t)
        else:
            injected_root.copy_(dev(k("sim_root_states")))
            injected_dof.copy_(dev(k("sim_dof_states")))
            st = _abi.StateViews()
            st.root_states, st.dof_state = injected_root.data_ptr(), injected_dof.data_ptr()
            before = np_(s.root).copy()
            s.post(state=st, step=t)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(np_(s.root), before, err_msg="the bound root rows were touched")
            s.root.copy_(injected_root)
            s.dof.copy_(injected_dof)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(np_(s.reset), k("reset"))
        np.testing.assert_array_equal(np_(s.progress), k("progress"))
        np.testing.assert_array_equal(np_(s.timeout), k("timeout"))
        for got, ref in ((s.obs, k("obs")), (s.obs_c, k("obs_clamped")), (s.rew, k("rew"))):
            assert R.close(np_(got), ref).all(), f"step {t}"
            worst = max(worst, float(np.abs(np_(got).astype(np.float64) - ref).max()))
        want_pack = np.concatenate([np_(s.obs_c), np_(s.rew)[:, None], np_(s.reset).astype(F)[:, None]], 1)
        np.testing.assert_array_equal(np_(s.out_pack), want_pack,
                                      err_msg=f"step {t}: out_pack is not [clamped obs | rew | reset]")
    print(f"N={N}: largest float difference from the reference trace {worst:.3g}")
    s.close()


# ------------------------------------------------------------------------------------------------ RNG, reset_idx
@pytest.mark.parametrize("env_offset", [0, 5])
def test_device_rng_equals_its_host_twin(lib, env_offset):
    N, seed, step = 67, 3, 11
    s = QuadSim(lib, N)
    s.reset.fill_(1)
    s.pre(step=step, seed=seed, env_offset=env_offset)
    torch.cuda.synchronize()
    noise = np.array([[O.uniform(seed, env_offset + e, step, c) for c in range(11)] for e in range(N)], F)
    p = R.params_from(s.qp)
    st = dict(root_states=np.zeros((N, 13), F), dof_states=np.zeros((N, 8, 2), F), reset=np.ones(N, np.int64),
              progress=np.zeros(N, np.int64))
    R.reset_envs(p, st, np.arange(N), noise)
    np.testing.assert_array_equal(np_(s.root), st["root_states"])
    np.testing.assert_array_equal(np_(s.dof), st["dof_states"])
    assert len(np.unique(np_(s.root)[:, 0])) == N
    s.close()


def test_reset_idx_with_a_repeated_id_changes_the_listed_envs_only(lib):
    N = 67
    s = QuadSim(lib, N)
    rng = np.random.default_rng(1)
    s.root.copy_(dev(rng.normal(size=(N, 13))))
    s.dof.copy_(dev(rng.normal(size=(N, 8, 2))))
    s.thr.fill_(1.0)
    s.progress.fill_(7)
    s.reset.fill_(1)
    s.noise = dev(rng.uniform(0, 1, (N, 11)))
    before = {k: np_(getattr(s, k)).copy() for k in ("root", "dof", "thr", "tgt", "frc", "progress", "reset")}
    ids = [5, 64, 5, 0, -1, 67]
    s.reset_idx(ids)
    listed = np.zeros(N, bool)
    listed[[5, 64, 0]] = True
    p = R.params_from(s.qp)
    st = dict(root_states=before["root"].copy(), dof_states=before["dof"].copy(), reset=before["reset"].copy(),
              progress=before["progress"].copy())
    R.reset_envs(p, st, np.flatnonzero(listed), np_(s.noise))
    np.testing.assert_array_equal(np_(s.root), st["root_states"])
    np.testing.assert_array_equal(np_(s.dof), st["dof_states"])
    np.testing.assert_array_equal(np_(s.reset), st["reset"])
    np.testing.assert_array_equal(np_(s.progress), st["progress"])
    for k in ("thr", "tgt", "frc"):      # cleared by pre_physics_step, not by reset_idx (quadcopter.py:323-326)
        np.testing.assert_array_equal(np_(getattr(s, k)), before[k])
    s.close()


# ------------------------------------------------------------------------------------------------ the task
def make_env(N, seed=0, cfg=None):
    return isaacgymenvs.make(seed=seed, task="Quadcopter", num_envs=N, sim_device=DEV, rl_device=DEV, headless=True,
                             cfg={"task": cfg or R.golden_cfg(N)})


STATE = ("root_states", "dof_state", "dof_position_targets", "thrusts", "forces", "obs_buf", "obs_clamped", "rew_buf",
         "reset_buf", "progress_buf", "timeout_buf", "actions")


def snapshot(env):
    torch.cuda.synchronize()
    return {k: np_(getattr(env, k)).copy() for k in STATE}


def test_whole_step_equals_the_three_launches(lib):
    """isaacgymenvs.make(Quadcopter), 67 envs: 8 steps of random actions with injected noise equal, bit for bit, the
    same sequence driven by hand through mg_quadcopter_pre -> mg_sim_simulate -> mg_quadcopter_post on a second sim;
    resets come from the first step (reset_buf starts at ones), from forced flags and from the 8-step episode limit"""
    N = 67
    env = make_env(N)
    assert env.num_obs == 21 and env.num_actions == 12 and env.obs_buf.shape == (N, 21) and env.num_bodies == 9
    assert (env.reset_buf == 1).all()
    s = QuadSim(lib, N)
    s.reset.fill_(1)
    rng = np.random.default_rng(9)
    resets = 0
    for t in range(8):
        noise, act = dev(rng.uniform(0, 1, (N, 11))), dev(rng.uniform(-1.3, 1.3, (N, 12)))
        forced = dev((rng.random(N) < 0.1).astype(np.int64), torch.int64)
        env.reset_buf.copy_(torch.maximum(env.reset_buf, forced))
        s.reset.copy_(torch.maximum(s.reset, forced))
        resets += int(s.reset.sum())
        env.set_reset_noise(noise)
        env.step(act)
        s.noise = noise
        s.act.copy_(act)
        s.pre(step=t)
        s.simulate()
        s.post(step=t)
        got = snapshot(env)
        for k, ref in (("root_states", s.root), ("dof_state", s.dof.view(N * 8, 2)), ("dof_position_targets", s.tgt),
                       ("thrusts", s.thr), ("forces", s.frc), ("obs_buf", s.obs), ("obs_clamped", s.obs_c),
                       ("rew_buf", s.rew), ("reset_buf", s.reset), ("progress_buf", s.progress),
                       ("timeout_buf", s.timeout), ("actions", s.act_out)):
            np.testing.assert_array_equal(got[k], np_(ref), err_msg=f"step {t}: {k}")
    assert resets > N and np.isfinite(got["obs_buf"]).all() and np.abs(got["forces"]).max() > 0
    # the caller's tensor in the place of env.forces: the steps write the thrusts into it, its other rows push
    import migym
    mine = torch.zeros((N, 9, 3), device=DEV)
    with pytest.raises(ValueError, match="LOCAL_SPACE"):
        env.apply_rigid_body_force_tensors(mine, None, migym.ENV_SPACE)
    env.apply_rigid_body_force_tensors(mine, None, migym.LOCAL_SPACE)
    assert env.forces.data_ptr() == mine.data_ptr()
    mine[:, 0, 1] = 0.5                   # 0.5 N on the chassis along its own y
    env.reset_buf.zero_()
    vy0 = np_(env.root_states)[:, 8].copy()
    env.step(torch.zeros((N, 12), device=DEV))
    torch.cuda.synchronize()
    keep = np_(env.progress_buf) > 0      # the envs this step's reward did not see the last of
    np.testing.assert_array_equal(np_(mine)[:, [2, 4, 6, 8], 2], np_(env.thrusts))
    assert (np_(mine)[:, 0, 1] == 0.5).all()
    dv = np_(env.root_states)[:, 8] - vy0
    assert keep.any() and np.abs(dv[keep]).max() > 0.5 * 0.01 * 0.5 / 0.2516, "the chassis row pushed nothing"
    env.close()
    s.close()


def test_reset_done_and_set_env_state_resume_bit_for_bit():
    N = 67
    a, b = make_env(N, seed=4), make_env(N, seed=4)
    rng = np.random.default_rng(2)
    acts = [dev(rng.uniform(-1, 1, (N, 12))) for _ in range(10)]
    for t in range(4):
        a.step(acts[t])
    a.reset_buf[::3] = 1                  # some envs are done when the state is taken
    state = a.get_env_state()
    assert {"thrusts", "dof_position_targets", "forces"} <= set(state)
    a.reset_done()
    mid = snapshot(a)
    for t in range(4, 10):
        a.step(acts[t])
    want = snapshot(a)
    b.step(acts[0])                       # b is somewhere else before it takes a's state
    b.set_env_state(state)
    _, done = b.reset_done()
    assert len(done) > 0
    for k, v in snapshot(b).items():
        np.testing.assert_array_equal(v, mid[k], err_msg=f"after reset_done: {k}")
    for t in range(4, 10):
        b.step(acts[t])
    for k, v in snapshot(b).items():
        np.testing.assert_array_equal(v, want[k], err_msg=f"resumed: {k}")
    a.close()
    b.close()


def _angle(q0, q1):
    d = np.abs((q0 * q1).sum(-1) / (np.linalg.norm(q0, axis=-1) * np.linalg.norm(q1, axis=-1)))
    return 2 * np.arccos(np.minimum(d, 1.0))


def test_hover_known_answer(lib):
    """DOF targets 0, each thrust held at M g / 4 in the rotor's own frame, upright at rest at z = 1, 20 simulates.
    The issue's bound is 4 x what the oracle's fp32 twin moves and turns under zero gravity from the same state.  That
    twin, at rest with nothing acting on it, does not move at all (0 m, 0 rad: computed below and printed), and four
    thrusts of fp32(M g / 4) cannot cancel nine fp32 weights to the last bit, so the bound as written is zero and no
    fp32 hover meets it.  What the forces' own rounding allows is added to it: the net force is at most
    4 ulp(M g / 4) / 2 + 9 ulp(m g) / 2 < 2^-21 M g, 4.7e-6 m/s^2, 9.4e-8 m over the 0.2 s, and the 20 steps' own
    roundings of a 1 m height (2^-24 each) are of the same size; ten times that estimate, 1e-6 m and 1e-6 rad, is
    asserted.  Measured on the MI355X: 1.8e-7 m, 0 rad.  Without the thrusts the body falls 0.5 g t^2 = 0.2 m, which
    is asserted as well, so the test tells a hover from a fall by five orders of magnitude."""
    N, steps = 6, 20
    s = QuadSim(lib, N)
    Mg = s.spec.total_mass() * 9.81
    s.frc[:, [2, 4, 6, 8], 2] = float(F(Mg / 4))
    root0 = np_(s.root).copy()
    for _ in range(steps):
        s.simulate()
    torch.cuda.synchronize()
    moved = np.linalg.norm(np_(s.root)[:, 0:3] - root0[:, 0:3], axis=1).max()
    turned = _angle(np_(s.root)[:, 3:7], root0[:, 3:7]).max()
    sp0 = _abi.SimParams.from_buffer_copy(s.sp)
    for i in range(3):
        sp0.gravity[i] = 0.0
    r, d = root0.copy(), np.zeros((N, 8, 2), F)
    for _ in range(steps):
        O.simulate(s.mnp, sp0, r, d, fp32=True)
    twin_moved = np.linalg.norm(r[:, 0:3] - root0[:, 0:3], axis=1).max()
    twin_turned = _angle(r[:, 3:7], root0[:, 3:7]).max()
    print(f"hover: moved {moved:.3g} m, turned {turned:.3g} rad; fp32 twin at zero gravity {twin_moved:.3g} m, "
          f"{twin_turned:.3g} rad")
    assert moved <= 4 * twin_moved + 1e-6 and turned <= 4 * twin_turned + 1e-6
    # the pitch hinges rest where their drives balance the rotors' excess thrust: (M g / 4 - m_rotor g) x 0.0425 m
    # / 1000 N m/rad = 5.3e-6 rad
    assert np.abs(np_(s.dof)[..., 0]).max() <= 1e-5
    s.frc.zero_()
    s.root.copy_(dev(root0))
    s.dof.zero_()
    for _ in range(steps):
        s.simulate()
    torch.cuda.synchronize()
    assert abs((root0[:, 2] - np_(s.root)[:, 2]).max() - 0.5 * 9.81 * 0.2 ** 2) < 0.02
    s.close()


def test_rollout_through_make_stays_finite_and_clear_of_the_ground(lib):
    """64 envs, 40 steps of random actions through the task at the YAML's episode length: finite, thrusts and targets
    inside their clamps, and the fp64 oracle counts no contact candidate on the GPU's states at any step"""
    from migym import configs
    N = 64
    env = make_env(N, cfg=configs.task_config("Quadcopter", N))
    _, mnp, sp, _ = R.task_model(env.cfg)
    rng = np.random.default_rng(3)
    for t in range(40):
        env.step(dev(rng.uniform(-1, 1, (N, 12))))
        torch.cuda.synchronize()
        root, dof = np_(env.root_states), np_(env.dof_state).reshape(N, 8, 2)
        assert np.isfinite(root).all() and np.isfinite(dof).all() and torch.isfinite(env.obs_buf).all()
        assert sum(len(O.contacts(mnp, sp, root[e], dof[e], 64)) for e in range(N)) == 0, f"step {t}"
    assert 0 <= float(env.thrusts.min()) and float(env.thrusts.max()) <= 2
    assert float(env.dof_position_targets.abs().max()) <= np.float32(np.radians(30))
    assert float(env.thrusts.max()) > 0 and int(env.progress_buf.max()) > 10
    env.close()
