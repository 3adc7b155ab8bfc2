"""GPU tests of the HumanoidAMP task (include/migym.h: mg_amp_pre, mg_amp_post, mg_amp_reset_idx, mg_amp_obs_demo;
migym/tasks/humanoid_amp.py).

References: the reference's own methods (tests/golden/trace_amp_*.npz, written by tests/golden/make_amp_golden.py and
replayed through mg_amp_post's state injection and mg_amp_reset_idx's recorded uniforms), their numpy restatement fed
the counter RNG's host twin (tests/amp_ref.py, pyoracle.uniform), and torch's own expression for the targets.

Shapes are the smallest that cross the kernels' edges: a team of 32 lanes per env and two envs per 64-lane block, so 6
envs are three blocks and 67 envs end in a block with one env (the odd tail); reset lists of 2 to 40 ids in shuffled
order; 5 and 130 demo samples; k_amp_pre takes 256 elements per block (168 and 1876 elements).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import amp_ref as R
import isaacgymenvs
import pyoracle as O
from migym import _abi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = [(N, name) for name in R.CONFIGS for N in R.SIZES]


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return _abi.lib()


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.array(a)).to(DEV, dtype).contiguous()   # a copy: the golden arrays are read-only


def rb_rows(pos):
    """(N, 15, 3) positions as rigid_body_states rows (N * 15, 13), identity rotations, zero twists"""
    n = pos.shape[0]
    rb = np.zeros((n, 15, 13), np.float32)
    rb[..., 0:3], rb[..., 6] = pos, 1.0
    return rb.reshape(n * 15, 13)


class AmpSim:
    """a sim of N task-configured humanoids with every tensor the AMP launches touch"""

    def __init__(self, lib, N, name="random", cfg=None):
        self.lib, self.N = lib, N
        self.cfg = cfg or R.golden_cfg(N, name)
        self.spec, self.mnp, self.sp, self.ap = R.task_model(self.cfg)
        self.steps = steps = int(self.ap.num_amp_obs_steps)
        z = lambda *s, dtype=torch.float32: torch.zeros(s, device=DEV, dtype=dtype)   # noqa: E731
        self.root = dev(np.tile(np.array(list(self.ap.initial_root), np.float32), (N, 1)))
        self.dof, self.act, self.tgt = z(N * 28, 2), z(N * 28), z(N * 28)
        self.dof_force, self.ncf, self.rb = z(N, 28), z(N * 15, 3), dev(rb_rows(np.zeros((N, 15, 3), np.float32)))
        self.actions, self.actions_out = z(N, 28), z(N, 28)
        self.obs, self.obs_clamped, self.rew = z(N, 105), z(N, 105), z(N)
        self.reset, self.progress = z(N, dtype=torch.long), z(N, dtype=torch.long)
        self.terminate, self.timeout = z(N, dtype=torch.long), z(N, dtype=torch.bool)
        self.amp = z(N, steps, 105)
        v = _abi.StateViews()
        v.root_states, v.dof_state = self.root.data_ptr(), self.dof.data_ptr()
        v.dof_actuation = self.act.data_ptr()
        v.dof_targets = self.tgt.data_ptr() if self.ap.pd_control else None
        v.dof_force, v.net_contact_forces = self.dof_force.data_ptr(), self.ncf.data_ptr()
        v.rigid_body_states = self.rb.data_ptr()
        self.sensors = z(N * len(self.spec.sensors), 6)
        v.sensors = self.sensors.data_ptr()
        self.sim = C.c_void_p()
        _abi.check(lib.mg_sim_create(self.mnp.ctypes.data, C.byref(self.sp), N, 0, C.byref(self.sim)), lib)
        _abi.check(lib.mg_sim_bind(self.sim, C.byref(v)), lib)
        self.table = R.table()
        self.frames, self.index, self.time = self.table.to_device(DEV)
        av = _abi.AmpViews()
        av.dof_targets, av.dof_actuation = self.tgt.data_ptr(), self.act.data_ptr()
        av.amp_obs, av.terminate = self.amp.data_ptr(), self.terminate.data_ptr()
        av.motion_frames, av.motion_index = self.frames.data_ptr(), self.index.data_ptr()
        av.motion_time = self.time.data_ptr()
        av.num_motions, av.num_frames = self.table.num_motions(), int(self.frames.shape[0])
        self.av = av
        self.noise = None
        self.out_pack = None

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
        _abi.check(self.lib.mg_amp_pre(self.sim, C.byref(self.ap), C.byref(self.av), C.byref(b), self.stream()),
                   self.lib)

    def simulate(self):
        _abi.check(self.lib.mg_sim_simulate(self.sim, self.stream()), self.lib)

    def post(self, state=None, **kw):
        b = self.tb(**kw)
        _abi.check(self.lib.mg_amp_post(self.sim, C.byref(self.ap), C.byref(self.av), C.byref(b),
                                        None if state is None else C.byref(state), self.stream()), self.lib)

    def reset_idx(self, ids, **kw):
        b = self.tb(**kw)
        self._ids = dev(ids, torch.int32)
        _abi.check(self.lib.mg_amp_reset_idx(self.sim, C.byref(self.ap), C.byref(self.av), C.byref(b),
                                             self._ids.data_ptr(), int(self._ids.numel()), self.stream()), self.lib)

    def demo(self, n, noise=None, seed=0, counter=0):
        out = torch.full((n, self.steps, 105), float("nan"), device=DEV)
        self._demo_noise = noise
        _abi.check(self.lib.mg_amp_obs_demo(C.byref(self.ap), C.byref(self.av),
                                            None if noise is None else noise.data_ptr(), seed, counter,
                                            out.data_ptr(), n, self.stream()), self.lib)
        return out

    def lanes(self):
        t, lay = C.c_int32(), C.c_int32()
        _abi.check(self.lib.mg_sim_kernel_layout(self.sim, C.byref(t), C.byref(lay)), self.lib)
        return t.value

    def close(self):
        if self.sim is not None:
            self.lib.mg_sim_destroy(self.sim)
            self.sim = None


# ------------------------------------------------------------------------------------------------ the traces
@pytest.mark.parametrize("N,name", CASES)
def test_kernels_replay_the_reference(lib, N, name):
    """all 6 recorded steps: mg_amp_pre bit-equal to torch's evaluation of the reference expression; mg_amp_post
    through the state-injection path with reset, terminate, progress and timeout bit-equal and observations, AMP
    buffer and reward by the 1e-4 rule; mg_amp_reset_idx from the recorded uniforms with the written velocities
    bit-equal (unblended frame rows: the frame index), states, observations and AMP history by the 1e-4 rule, and only
    the listed envs changed.  Measured on the MI355X: see DESIGN.md §13 (printed per trace)."""
    g = R.trace(N, name)
    s = AmpSim(lib, N, name)
    p = R.params_from(s.ap)
    s.amp.copy_(dev(g["amp_0"]))
    s.out_pack = torch.full((N, 107), float("nan"), device=DEV)
    worst = dict(obs=0.0, amp=0.0, r_state=0.0, r_obs=0.0)
    amp_ref = g["amp_0"].copy()
    for t in range(int(g["steps"])):
        k = f"s{t}_"
        s.progress.copy_(dev(g[k + "progress_in"], torch.long))
        s.actions.copy_(dev(g[k + "actions"]))
        s.pre()
        a = s.actions
        want = (dev(p["offset"]) + dev(p["scale"]) * a) if p["pd"] else (a * dev(p["effort"]) * float(p["power_scale"]))
        driven = (s.tgt if p["pd"] else s.act).view(N, 28)
        assert torch.equal(driven, want) and torch.equal(s.actions_out, a), f"step {t}: mg_amp_pre"
        assert np.array_equal(driven.cpu().numpy(), g[k + "driven"]), f"step {t}: targets against the trace"
        inj = _abi.StateViews()
        keep = [dev(g[k + "root_in"]), dev(g[k + "dof_in"].reshape(N * 28, 2)), dev(rb_rows(g[k + "rb_pos"])),
                dev(g[k + "ncf"].reshape(N * 15, 3))]
        inj.root_states, inj.dof_state = keep[0].data_ptr(), keep[1].data_ptr()
        inj.rigid_body_states, inj.net_contact_forces = keep[2].data_ptr(), keep[3].data_ptr()
        s.post(state=inj, step=t)
        torch.cuda.synchronize()
        for got, key in ((s.reset, "reset"), (s.terminate, "terminate"), (s.progress, "progress"),
                         (s.timeout, "timeout")):
            assert np.array_equal(got.cpu().numpy(), g[k + key]), f"step {t}: {key}"
        assert (s.rew == 1).all()
        amp_ref = np.concatenate([g[k + "obs"][:, None], amp_ref[:, :-1]], 1)
        for got, ref, w in ((s.obs, g[k + "obs"], "obs"), (s.amp, amp_ref, "amp")):
            err, ok = R.close(got.cpu().numpy(), ref)
            worst[w] = max(worst[w], err)
            assert ok, f"step {t}: {w} off by {err:.3g}"
        assert torch.equal(s.obs_clamped, s.obs), "HumanoidAMP.yaml has no clipObservations"
        pack = torch.cat([s.obs_clamped, s.rew.view(N, 1), s.reset.view(N, 1).float()], 1)
        assert torch.equal(s.out_pack, pack), f"step {t}: out_pack is not [clamped obs | rew | reset]"
        assert torch.equal(s.amp[:, 0], s.obs), "slot 0 is this step's observation"
        # reset_idx on the reference's state
        s.root.copy_(keep[0])
        s.dof.copy_(keep[1])
        s.rb.copy_(keep[2])
        s.obs.copy_(dev(g[k + "obs"]))
        s.amp.copy_(dev(amp_ref))
        before = [x.clone() for x in (s.root, s.dof.view(N, 56), s.obs, s.amp.view(N, -1), s.progress, s.reset,
                                      s.terminate)]
        ids = g[k + "ids"]
        s.noise = dev(g[k + "noise"])
        s.reset_idx(ids, step=t)
        s.noise = None
        torch.cuda.synchronize()
        idt = torch.as_tensor(ids.astype(np.int64), device=DEV)
        r_dof = s.dof.view(N, 28, 2)[idt].cpu().numpy()
        r_root = s.root[idt].cpu().numpy()
        if p["state_init"] != 0:
            assert np.array_equal(r_dof[..., 1], g[k + "r_dof"][..., 1]), f"step {t}: frame index (DOF velocities)"
            assert np.array_equal(r_root[:, 7:], g[k + "r_root"][:, 7:]), f"step {t}: frame index (root twist)"
        for got, ref, w in ((r_root, g[k + "r_root"], "r_state"), (r_dof, g[k + "r_dof"], "r_state"),
                            (s.obs[idt].cpu().numpy(), g[k + "r_obs"], "r_obs"),
                            (s.amp[idt].cpu().numpy(), g[k + "r_amp"], "r_obs")):
            err, ok = R.close(got, ref)
            worst[w] = max(worst[w], err)
            assert ok, f"step {t}: reset {w} off by {err:.3g}"
        assert (s.progress[idt] == 0).all() and (s.reset[idt] == 0).all() and (s.terminate[idt] == 0).all()
        rest = torch.ones(N, dtype=torch.bool, device=DEV)
        rest[idt] = False
        for b, now in zip(before, (s.root, s.dof.view(N, 56), s.obs, s.amp.view(N, -1), s.progress, s.reset,
                                   s.terminate)):
            assert torch.equal(b[rest], now[rest]), f"step {t}: an unlisted env changed"
        amp_ref = amp_ref.copy()
        amp_ref[ids] = g[k + "r_amp"]
        s.amp.copy_(dev(amp_ref))
    print(f"{name} N={N}: worst {worst}")
    s.close()


@pytest.mark.parametrize("name", ["random", "hybrid"])
@pytest.mark.parametrize("n", [5, 130])
def test_obs_demo_replays_the_reference(lib, name, n):
    d = R.demo()
    s = AmpSim(lib, 4, name)
    out = s.demo(n, dev(d[f"{name}_n{n}_noise"]))
    torch.cuda.synchronize()
    err, ok = R.close(out.view(n, -1).cpu().numpy(), d[f"{name}_n{n}_out"])
    print(f"demo {name} n={n}: {err:.3g}")
    assert ok, err
    s.close()


# ------------------------------------------------------------------------------------------------ the RNG, repeated ids
@pytest.mark.parametrize("env_offset", [0, 5])
def test_device_rng_matches_its_host_twin(lib, env_offset):
    """noise = NULL: a Hybrid reset of 9 envs equals the restatement fed pyoracle.uniform(seed, env_offset + e,
    step | 2^62, column) -- paths and frame rows bit for bit, the rest by the 1e-4 rule -- and a demo fetch the
    restatement fed uniform(seed, i, counter | 2^61, column)"""
    N, seed, step = 9, 20261021, 7   # a seed whose nine hybrid draws fall on both sides of 0.5 at both offsets
    s = AmpSim(lib, N, "hybrid")
    p = R.params_from(s.ap)
    rng = np.random.default_rng(3)
    rb = rng.uniform(0, 1, (N, 15, 3)).astype(np.float32)
    s.rb.copy_(dev(rb_rows(rb)))
    s.progress.fill_(3)
    ids = np.arange(N)[::-1].copy()
    noise = np.array([[O.uniform(seed, env_offset + int(e), step | (1 << 62), c) for c in range(3)] for e in ids],
                     np.float32)
    st = dict(root=np.ones((N, 13), np.float32), dof=np.ones((N, 28, 2), np.float32), obs=np.zeros((N, 105), np.float32),
              amp=np.zeros((N, p["steps"], 105), np.float32), progress=np.full(N, 3), reset=np.ones(N, np.int64),
              terminate=np.ones(N, np.int64))
    ref, _, _ = R.reset_idx(p, s.table, st, ids, noise, rb)
    assert ref.any() and not ref.all(), "both hybrid paths"
    s.reset_idx(ids, seed=seed, step=step, env_offset=env_offset)
    torch.cuda.synchronize()
    got_dof = s.dof.view(N, 28, 2).cpu().numpy()
    assert np.array_equal(got_dof[..., 1], st["dof"][..., 1]) and np.array_equal(s.root.cpu().numpy()[:, 7:], st["root"][:, 7:])
    for got, want in ((s.root, st["root"]), (s.dof.view(N, 28, 2), st["dof"]), (s.obs, st["obs"]), (s.amp, st["amp"])):
        err, ok = R.close(got.cpu().numpy(), want)
        assert ok, err
    assert (s.progress == 0).all()
    n, counter = 7, 11
    dn = np.array([[O.uniform(seed, i, counter | (1 << 61), c) for c in range(2)] for i in range(n)], np.float32)
    out = s.demo(n, None, seed=seed, counter=counter)
    torch.cuda.synchronize()
    err, ok = R.close(out.cpu().numpy(), R.obs_demo(p, s.table, dn))
    assert ok, err
    s.close()


def test_reset_idx_with_a_repeated_id(lib):
    """an id listed twice (with equal noise rows) resets like one listed once; an id out of range is skipped; the
    last team block is ragged"""
    N = 11
    s = AmpSim(lib, N, "random")
    p = R.params_from(s.ap)
    rng = np.random.default_rng(5)
    rb = rng.uniform(0, 1, (N, 15, 3)).astype(np.float32)
    s.rb.copy_(dev(rb_rows(rb)))
    s.root.copy_(dev(rng.uniform(-1, 1, (N, 13))))
    s.dof.copy_(dev(rng.uniform(-1, 1, (N * 28, 2))))
    s.amp.copy_(dev(rng.uniform(-1, 1, (N, p["steps"], 105))))
    s.progress.fill_(4)
    s.reset.fill_(1)
    ids = np.array([7, 2, 7, 10, N + 3, 0, -1], np.int32)
    noise = rng.uniform(0, 1, (len(ids), 3)).astype(np.float32)
    noise[2] = noise[0]
    st = dict(root=s.root.cpu().numpy(), dof=s.dof.view(N, 28, 2).cpu().numpy(), obs=s.obs.cpu().numpy(),
              amp=s.amp.cpu().numpy(), progress=s.progress.cpu().numpy(), reset=s.reset.cpu().numpy(),
              terminate=s.terminate.cpu().numpy())
    before = {k: v.copy() for k, v in st.items()}
    valid = [0, 1, 3, 5]
    R.reset_idx(p, s.table, st, ids[valid], noise[valid], rb)
    s.noise = dev(noise)
    s.reset_idx(ids)
    torch.cuda.synchronize()
    for k, got in (("root", s.root), ("dof", s.dof.view(N, 28, 2)), ("obs", s.obs), ("amp", s.amp)):
        err, ok = R.close(got.cpu().numpy(), st[k])
        assert ok, (k, err)
    listed = np.array([e in (7, 2, 10, 0) for e in range(N)])
    assert np.array_equal(s.dof.view(N, 28, 2).cpu().numpy()[~listed], before["dof"][~listed])
    assert np.array_equal(s.amp.cpu().numpy()[~listed], before["amp"][~listed])
    assert (s.progress.cpu().numpy() == np.where(listed, 0, 4)).all()
    assert (s.reset.cpu().numpy() == np.where(listed, 0, 1)).all()
    s.close()


# ------------------------------------------------------------------------------------------------ physics
@pytest.mark.parametrize("n", [R.PHYS_SMALL, R.PHYS_ACTORS])
@pytest.mark.parametrize("kind", ["clip", "fallen"])
def test_task_model_physics_matches_oracle(lib, kind, n):
    """one mg_sim_simulate of the task model (free base, 28 position drives, 122 self pairs, plane contact) at 6 and 66
    actors against the fp64 oracle, by the one-step rule of tests/tree_physics_ref.compare, with random position
    targets inside the action range; the 64-lane instance runs, on a real task's model for the first time.  The
    states are the oracle's choice (amp_ref.physics_states); none of the pool was passed over."""
    import types
    spec, mnp, sp, root, dof, tgt, ref, passed_over = R.physics_states(kind)
    print(f"{kind}: pool states passed over: {passed_over}")
    s = AmpSim(lib, n, cfg=R.physics_cfg(n))
    assert s.lanes() == 64
    s.root.copy_(dev(root[:n]))
    s.dof.copy_(dev(dof[:n].reshape(n * 28, 2)))
    s.tgt.copy_(dev(tgt[:n].reshape(-1)))
    s.ncf.fill_(float("nan"))   # every row must be written
    s.dof_force.fill_(float("nan"))
    s.rb.fill_(float("nan"))
    s.simulate()
    torch.cuda.synchronize()
    got = types.SimpleNamespace(root=s.root.cpu().numpy(), dof=s.dof.view(n, 28, 2).cpu().numpy(),
                                dof_force=s.dof_force.cpu().numpy(), ncf=s.ncf.view(n, 15, 3).cpu().numpy())
    rb = s.rb.view(n, 15, 13).cpu().numpy()
    s.close()
    nrm = np.linalg.norm(ref.ncf[:n], axis=-1)
    if kind == "fallen":
        assert (np.delete(nrm, [11, 14], 1) > 1).any(1).all(), "a fallen state with no force on a non-foot body"
    else:
        assert (nrm[:, [11, 14]] > 1).any(1).mean() > 0.8, "the clip states stand on their feet"
    err, ok = R.close(rb[:, 0, 0:3], got.root[:, 0:3])
    same_rot = np.abs((rb[:, 0, 3:7] * got.root[:, 3:7]).sum(-1)) > 1 - 1e-5   # q and -q are one rotation
    assert ok and same_rot.all() and np.isfinite(rb).all(), "rigid_body_states row 0 is the root's pose"
    err, ok = R.close(rb[..., 0:3], ref.rb[:n, :, 0:3], 2e-4)
    assert ok, f"rigid-body positions off by {err:.3g}"
    R.compare_step(f"test_task_model_physics_matches_oracle[{kind}-{n}]", kind, n, got)


# ------------------------------------------------------------------------------------------------ the task
def make_env(N, name="random", seed=0, cfg=None):
    return isaacgymenvs.make(seed=seed, task="HumanoidAMP", num_envs=N, sim_device=DEV, rl_device=DEV, headless=True,
                             cfg={"task": cfg or R.golden_cfg(N, name)})


def test_whole_step_equals_the_three_launches(lib):
    """isaacgymenvs.make(HumanoidAMP), 67 envs, Hybrid: 8 steps of random actions with reset_done() in between equal,
    bit for bit, the same sequence driven by hand through mg_amp_pre -> mg_sim_simulate x 2 -> mg_amp_post and
    mg_amp_reset_idx on a second sim"""
    N = 67
    env = make_env(N, "hybrid")
    assert env.num_obs == 105 and env.num_actions == 28 and env.get_num_amp_obs() == 315 and env.control_freq_inv == 2
    assert env.amp_observation_space.shape == (315,) and env.dt == 2 * 0.0166
    assert env._key_body_ids.tolist() == [5, 8, 11, 14] and env._contact_body_ids.tolist() == [11, 14]
    assert (env.reset_buf == 1).all() and (env._terminate_buf == 1).all()
    s = AmpSim(lib, N, "hybrid")
    assert s.lanes() == 64, "the 29-node, 18-geom humanoid runs on the (64, 40, 48, 48, 192) instance"
    rng = np.random.default_rng(9)
    s.reset.fill_(1)
    saw_reset = saw_timeout = False
    for t in range(8):
        _, done = env.reset_done()
        ids = s.reset.nonzero().flatten()
        assert torch.equal(done, ids)
        if len(ids):
            s.reset_idx(ids.cpu().numpy(), step=t)
            saw_reset |= t > 0
        a = rng.uniform(-1.3, 1.3, (N, 28)).astype(np.float32)
        if t == 3:
            for b in (env.progress_buf, s.progress):
                b[10:20] = 9    # these reach max_episode_length - 1 in two steps
        obs, rew, reset, extras = env.step(dev(a))
        s.actions.copy_(dev(a))
        s.pre()
        s.simulate()
        s.simulate()
        s.post(step=t)
        torch.cuda.synchronize()
        assert torch.equal(env.obs_buf, s.obs) and torch.equal(obs["obs"], s.obs), f"step {t}"
        assert torch.equal(env.rew_buf, s.rew) and torch.equal(env.reset_buf, s.reset)
        assert torch.equal(env.progress_buf, s.progress) and torch.equal(env.timeout_buf, s.timeout)
        assert torch.equal(env.dof_state, s.dof) and torch.equal(env.root_states, s.root)
        assert torch.equal(env.dof_targets, s.tgt) and torch.equal(env.rigid_body_states, s.rb)
        assert torch.equal(env.net_contact_force_tensor, s.ncf) and torch.equal(env.dof_force_tensor, s.dof_force)
        assert torch.equal(extras["amp_obs"], s.amp.view(N, -1)) and torch.equal(extras["terminate"], s.terminate)
        assert torch.isfinite(env.obs_buf).all() and extras["time_outs"].dtype == torch.bool
        saw_timeout |= bool(extras["time_outs"].any())
    assert saw_reset and saw_timeout
    demo = env.fetch_amp_obs_demo(5)
    torch.cuda.synchronize()
    assert demo.shape == (5, 315) and torch.isfinite(demo).all()
    with pytest.raises(ValueError, match="reset noise"):
        env.set_reset_noise(torch.zeros((N, 2), device=DEV))
    env.close()
    s.close()


def test_env_state_resumes_bitwise(lib):
    """get_env_state / set_env_state (the AMP history and terminate included) resume a rollout bit for bit"""
    N = 67
    env = make_env(N, "random", seed=3)
    rng = np.random.default_rng(4)
    acts = [dev(rng.uniform(-1, 1, (N, 28)).astype(np.float32)) for _ in range(6)]
    env.reset_done()
    for a in acts[:2]:
        env.step(a)
        env.reset_done()
    snap = env.get_env_state()
    for k in ("_amp_obs_buf", "_terminate_buf", "dof_targets", "root_states", "dof_state", "rigid_body_states",
              "net_contact_force_tensor", "progress_buf", "reset_buf", "control_steps"):
        assert k in snap, k
    outs = []
    for a in acts[2:]:
        o, r, d, ex = env.step(a)
        outs.append((o["obs"].clone(), r.clone(), d.clone(), ex["amp_obs"].clone(), ex["terminate"].clone(),
                     env.dof_state.clone()))
        env.reset_done()
    env._amp_obs_buf.zero_()
    env._terminate_buf.fill_(1)
    env.set_env_state(snap)
    assert torch.equal(env._amp_obs_buf, snap["_amp_obs_buf"]) and torch.equal(env._terminate_buf, snap["_terminate_buf"])
    for a, want in zip(acts[2:], outs):
        o, r, d, ex = env.step(a)
        for x, y in zip((o["obs"], r, d, ex["amp_obs"], ex["terminate"], env.dof_state), want):
            assert torch.equal(x, y), "the resumed rollout differs"
        env.reset_done()
    env.close()


def test_rollout_facts_through_make(lib):
    """64 envs reset to the default pose, 50 zero-action steps through the task (the PD targets are then the action
    offsets): everything stays finite, and the contact candidates of the GPU's states before each step, counted by the
    fp64 oracle, stay within max_contacts = 48, so the rollout stays clear of the truncation"""
    N = 64
    cfg = R.golden_cfg(N, "default")
    cfg["env"].update({"pdControl": True, "episodeLength": 300})
    env = make_env(N, cfg=cfg)
    _, mnp, sp, _ = R.task_model(cfg)
    zero = torch.zeros((N, 28), device=DEV)
    env.reset_done()
    most = 0
    for t in range(50):
        torch.cuda.synchronize()
        root, dof = env.root_states.cpu().numpy(), env.dof_state.view(N, 28, 2).cpu().numpy()
        most = max(most, max(len(O.contacts(mnp, sp, root[a], dof[a], 96)) for a in range(0, N, 8)))
        obs, rew, reset, extras = env.step(zero)
        assert torch.isfinite(obs["obs"]).all() and torch.isfinite(env.root_states).all(), f"step {t}"
        assert torch.isfinite(extras["amp_obs"]).all() and torch.isfinite(env.net_contact_force_tensor).all()
    print(f"most contact candidates {most}; final root z {env.root_states[:, 2].min():.3f}..{env.root_states[:, 2].max():.3f}")
    assert most <= 48 == sp.max_contacts
    assert (env.progress_buf == 50).all() and (rew == 1).all()
    env.close()
