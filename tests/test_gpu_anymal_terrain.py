"""GPU tests of the AnymalTerrain task (include/migym.h: mg_anymal_terrain_pre, _post, _reset_idx;
migym/tasks/anymal_terrain.py).

References: the reference's own post-physics step (tests/golden/trace_anymal_terrain.npz, replayed through
mg_anymal_terrain_post's state injection), its numpy restatement fed the counter RNG's host twin
(tests/anymal_terrain_ref.py, pyoracle.uniform), torch's own expressions for the torques and the height columns (the
latter from the existing mg_height_scan), and the fp64 oracle's simulate of the task model under the kernel's efforts.

Shapes are the smallest that cross the kernels' edges: k_at_post takes 4 envs per 64-lane block (6 envs: a second,
ragged block; 67: many blocks and a ragged tail of 3; the finishing pass adds 2 and 17 partial rows, the latter in two
rounds of its 16 segments), k_at_pre 256 elements per block (72 and 804 elements).
"""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import anymal_ref as AR
import anymal_terrain_ref as R
import isaacgymenvs
import parity_stats as PS
import pyoracle as O
from migym import _abi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [6, 67]
NR = _abi.MG_ANYMAL_TERRAIN_REWARDS


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return _abi.lib()


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.array(a)).to(DEV, dtype).contiguous()   # a copy: the golden arrays are read-only


class TerrainSim:
    """a sim of N task-configured robots with every tensor the AnymalTerrain launches touch; ``table`` (metres, numpy)
    and ``origins`` bind a terrain to the task layer (the physics stays on the plane unless ``physics_field``)"""

    def __init__(self, lib, N, cfg=None, table=None, origins=None, setup=None, physics_field=False):
        self.lib, self.N = lib, N
        self.cfg = cfg or R.golden_cfg(N)
        self.spec, self.mnp, self.sp, self.ap = R.task_model(self.cfg)
        if setup:
            setup(self.ap)
        self.nb = nb = len(self.spec.bodies)
        z = lambda *s, dtype=torch.float32: torch.zeros(s, device=DEV, dtype=dtype)   # noqa: E731
        self.root = dev(np.tile(np.array(list(self.ap.base_init_state), np.float32), (N, 1)))
        self.dof, self.act, self.ncf = z(N * 12, 2), z(N * 12), z(N * nb, 3)
        self.commands, self.torques = z(N, 4), z(N, 12)
        self.last_actions, self.last_dof_vel, self.feet_air_time = z(N, 12), z(N, 12), z(N, 4)
        self.episode_sums, self.episode_out = z(N, NR), z(NR + 1)
        self.terrain_levels, self.terrain_types = z(N, dtype=torch.int32), z(N, dtype=torch.int32)
        self.env_origins, self.measured = z(N, 3), z(N, 140)
        self.partials, self.mark = z((N + 3) // 4, 16), z(N, dtype=torch.int32)
        self.actions, self.actions_out = z(N, 12), z(N, 12)
        self.obs, self.obs_clamped, self.rew = z(N, 188), z(N, 188), z(N)
        self.reset, self.progress = z(N, dtype=torch.long), z(N, dtype=torch.long)
        self.timeout = z(N, dtype=torch.bool)
        self.table = None if table is None else dev(table)
        self.origins = z(1, 1, 3) if origins is None else dev(origins)
        if table is not None:
            self.ap.hf_heights = self.table.data_ptr()
        v = _abi.StateViews()
        v.root_states, v.dof_state = self.root.data_ptr(), self.dof.data_ptr()
        v.dof_actuation, v.net_contact_forces = self.act.data_ptr(), self.ncf.data_ptr()
        self.sim = C.c_void_p()
        _abi.check(lib.mg_sim_create(self.mnp.ctypes.data, C.byref(self.sp), N, 0, C.byref(self.sim)), lib)
        _abi.check(lib.mg_sim_bind(self.sim, C.byref(v)), lib)
        if physics_field:
            hf = _abi.Heightfield(heights=self.table.data_ptr(), nx=table.shape[0], ny=table.shape[1],
                                  dx=float(self.ap.hf_dx), x0=float(self.ap.hf_x0), y0=float(self.ap.hf_y0),
                                  hmax=float(table.max()), env_origins=None)
            _abi.check(lib.mg_sim_set_heightfield(self.sim, C.byref(hf)), lib)
        av = _abi.AnymalTerrainViews()
        av.commands, av.torques = self.commands.data_ptr(), self.torques.data_ptr()
        av.last_actions, av.last_dof_vel = self.last_actions.data_ptr(), self.last_dof_vel.data_ptr()
        av.feet_air_time, av.episode_sums = self.feet_air_time.data_ptr(), self.episode_sums.data_ptr()
        av.terrain_levels, av.terrain_types = self.terrain_levels.data_ptr(), self.terrain_types.data_ptr()
        av.env_origins, av.terrain_origins = self.env_origins.data_ptr(), self.origins.data_ptr()
        av.dof_actuation, av.episode_out = self.act.data_ptr(), self.episode_out.data_ptr()
        av.measured_heights, av.partials, av.reset_mark = self.measured.data_ptr(), self.partials.data_ptr(), \
            self.mark.data_ptr()
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
        _abi.check(self.lib.mg_anymal_terrain_pre(self.sim, C.byref(self.ap), C.byref(self.av), C.byref(b),
                                                  self.stream()), self.lib)

    def simulate(self):
        _abi.check(self.lib.mg_sim_simulate(self.sim, self.stream()), self.lib)

    def post(self, state=None, push=False, **kw):
        b = self.tb(**kw)
        self.av.push_now = int(push)
        _abi.check(self.lib.mg_anymal_terrain_post(self.sim, C.byref(self.ap), C.byref(self.av), C.byref(b),
                                                   None if state is None else C.byref(state), self.stream()), self.lib)

    def reset_idx(self, ids, update_levels=True, **kw):
        b = self.tb(**kw)
        self._ids = dev(ids, torch.int32)
        _abi.check(self.lib.mg_anymal_terrain_reset_idx(self.sim, C.byref(self.ap), C.byref(self.av), C.byref(b),
                                                        self._ids.data_ptr(), int(self._ids.numel()),
                                                        int(update_levels), self.stream()), self.lib)

    def load(self, st):
        """the task state of a restatement dict"""
        N = self.N
        for t, k, dt in ((self.progress, "progress", torch.long), (self.reset, "reset", torch.long),
                         (self.timeout, "timeout", torch.bool), (self.root, "root", None), (self.commands, "commands", None),
                         (self.torques, "torques", None), (self.last_actions, "last_actions", None),
                         (self.last_dof_vel, "last_dof_vel", None), (self.feet_air_time, "feet_air_time", None),
                         (self.episode_sums, "episode_sums", None), (self.env_origins, "env_origins", None),
                         (self.terrain_levels, "terrain_levels", torch.int32),
                         (self.terrain_types, "terrain_types", torch.int32), (self.episode_out, "episode_out", None)):
            t.copy_(dev(st[k], dt or torch.float32))
        self.dof.copy_(dev(st["dof"].reshape(N * 12, 2)))

    def state(self):
        N = self.N
        c = lambda t: t.cpu().numpy()   # noqa: E731
        return dict(progress=c(self.progress), reset=c(self.reset), timeout=c(self.timeout), root=c(self.root),
                    dof=c(self.dof).reshape(N, 12, 2), commands=c(self.commands), torques=c(self.torques),
                    last_actions=c(self.last_actions), last_dof_vel=c(self.last_dof_vel),
                    feet_air_time=c(self.feet_air_time), episode_sums=c(self.episode_sums),
                    env_origins=c(self.env_origins), terrain_levels=c(self.terrain_levels),
                    terrain_types=c(self.terrain_types), episode_out=c(self.episode_out))

    def close(self):
        if self.sim is not None:
            self.lib.mg_sim_destroy(self.sim)
            self.sim = None


def golden_sim(lib, N, trace=None):
    """a sim of N envs bound to the synthetic terrain of the trace of ``trace`` (default N) envs, and the
    restatement's params for it"""
    g, T = R.golden(), trace or N
    table = (g[f"N{T}_height_field_raw"].astype(np.float32) * np.float32(g["vertical_scale"])).astype(np.float32)
    origins = g[f"N{T}_terrain_origins"].astype(np.float32)
    s = TerrainSim(lib, N, table=table, origins=origins, setup=lambda ap: R.golden_terrain(ap, T))
    return s, R.params_from(s.ap, table, origins)


BITWISE = ("progress", "reset", "timeout", "root", "dof", "terrain_levels", "env_origins", "feet_air_time",
           "last_actions", "last_dof_vel")


# ------------------------------------------------------------------------------------------------ post
@pytest.mark.parametrize("N", SIZES)
def test_post_replays_the_reference(lib, N):
    """every recorded step through the state-injection path with the recorded draws: reset, progress, timeout, DOF
    state, root rows, commands x / y / heading, terrain levels, env origins, feet_air_time, last_actions and
    last_dof_vel bit-equal; commands[:, 2], observations, reward, episode sums and means by the 1e-4 rule; the reward
    clip falls on the same envs.  One step pushes; some roots lie outside the table.  Measured on the MI355X over both
    traces: max |obs - ref| 4.8e-7, |rew - ref| 4.7e-9, |commands[:, 2] - ref| 2.4e-7, |episode_sums - ref| 6.0e-8,
    |episode_out - ref| 1.2e-7 (printed per step)."""
    g = R.golden()
    s, p = golden_sim(lib, N)
    worst = {}
    for t in range(int(g["steps"])):
        pre = f"N{N}_s{t}_"
        s.load(R.golden_state(g, N, t))
        inj_root, inj_dof = dev(g[pre + "root_in"]), dev(g[pre + "dof_in"].reshape(N * 12, 2))
        inj_ncf = dev(g[pre + "ncf"].reshape(N * s.nb, 3))
        v = _abi.StateViews()
        v.root_states, v.dof_state, v.net_contact_forces = inj_root.data_ptr(), inj_dof.data_ptr(), inj_ncf.data_ptr()
        s.root.fill_(7.0)
        s.dof.fill_(7.0)
        s.actions.copy_(dev(g[pre + "actions"]))
        s.noise = dev(g[pre + "noise"])
        s.post(state=v, push=bool(g[pre + "push_now"]), step=t)
        torch.cuda.synchronize()
        got = s.state()
        got["root"], got["dof"] = inj_root.cpu().numpy(), inj_dof.view(N, 12, 2).cpu().numpy()
        for k in BITWISE:
            assert np.array_equal(got[k], g[pre + k]), f"step {t}: {k}"
        assert np.array_equal(got["commands"][:, [0, 1, 3]], g[pre + "commands"][:, [0, 1, 3]]), f"step {t}: commands"
        assert np.array_equal(s.measured.cpu().numpy(), g[pre + "measured_heights"]), f"step {t}: measured heights"
        obs, rew = s.obs.cpu().numpy(), s.rew.cpu().numpy()
        for name, x in (("commands", got["commands"]), ("obs", obs), ("rew", rew),
                        ("episode_sums", got["episode_sums"]), ("episode_out", got["episode_out"])):
            e = float(np.abs(x.astype(np.float64) - g[pre + name]).max())
            worst[name] = max(worst.get(name, 0.0), e)
            print(f"N={N} step {t}: max |{name} - ref| = {e:.3g}")
            PS.record(f"test_post_replays_the_reference[{N}] step {t}", name, x, g[pre + name], atol=1e-4, rtol=1e-4)
            assert R.close(x, g[pre + name]).all(), f"step {t}: {name} off by {e:.3g}"
        term = p["rew_term"] * ((g[pre + "reset"] != 0) & ~g[pre + "timeout_in"])
        assert np.array_equal((rew - term) == 0, g[pre + "clipped"]), f"step {t}: the clip at 0 falls on the same envs"
        assert np.array_equal(s.obs_clamped.cpu().numpy(), np.clip(obs, -p["clip_obs"], p["clip_obs"]))
        assert (s.root == 7.0).all() and (s.dof == 7.0).all(), "the sim's own state is not touched under injection"
        assert (s.mark == 0).all()
    print(f"N={N}: worst over the trace {worst}")
    s.close()


# ------------------------------------------------------------------------------------------------ pre
@pytest.mark.parametrize("N", SIZES)
def test_pre_equals_the_torch_expression_bitwise(lib, N):
    """actions_out = clamp(actions); torque = clip(Kp (action_scale a + default - q) - Kd qd, -80, 80): bit-equal to
    torch's evaluation of the reference's expression (anymal_terrain.py:444-445) on the device, and to the recorded
    torques; written to dof_actuation and to views.torques"""
    g = R.golden()
    s, p = golden_sim(lib, N)
    a, q = g[f"N{N}_s0_actions"], g[f"N{N}_s0_pre_dof"]
    s.actions.copy_(dev(a))
    s.dof.copy_(dev(q.reshape(N * 12, 2)))
    s.act.fill_(7.0)
    s.pre()
    torch.cuda.synchronize()
    actions = torch.clamp(s.actions, -1.0, 1.0)
    default = dev(np.tile(p["default"], (N, 1)))
    dof_pos, dof_vel = s.dof.view(N, 12, 2)[..., 0], s.dof.view(N, 12, 2)[..., 1]
    Kp, Kd, action_scale = float(s.ap.Kp), float(s.ap.Kd), float(s.ap.action_scale)
    want = torch.clip(Kp * (action_scale * actions + default - dof_pos) - Kd * dof_vel, -80., 80.)
    assert torch.equal(s.actions_out, actions) and (np.abs(a) > 1).any()
    assert torch.equal(s.torques, want) and torch.equal(s.act.view(N, 12), want)
    assert (want.abs() == 80.0).any() and (want.abs() < 80.0).any(), "some drives saturate, some do not"
    assert np.array_equal(s.torques.cpu().numpy(), g[f"N{N}_s0_torques_in"])
    s.close()


# ------------------------------------------------------------------------------------------------ the height columns
@pytest.mark.parametrize("N", SIZES)
def test_height_columns_equal_the_height_scan(lib, N):
    """noise off, a rough 17 x 17 field, actors inside and outside the grid with random yaw and tilt: the 140 height
    columns equal clip(z - 0.5 - height_scan(points), -1, 1) * scale evaluated in torch from the existing
    mg_height_scan, bit for bit; measured_heights is the scan itself"""
    rng = np.random.default_rng(17 + N)
    table = rng.uniform(-0.4, 0.4, (17, 17)).astype(np.float32)

    def setup(ap):
        ap.hf_nx, ap.hf_ny, ap.hf_dx, ap.hf_x0, ap.hf_y0 = 17, 17, 0.25, -1.5, -2.5
        ap.add_noise = 0

    s = TerrainSim(lib, N, cfg=R.golden_cfg(N, **{"learn.episodeLength_s": 20.0}), table=table, setup=setup,
                   physics_field=True)
    root = np.zeros((N, 13), np.float32)
    root[:, 0] = rng.uniform(-3.0, 4.0, N)      # the grid spans x in [-1.5, 2.5], y in [-2.5, 1.5]
    root[:, 1] = rng.uniform(-4.0, 3.0, N)
    root[:, 2] = np.linspace(-1.2, 2.0, N)      # both ends of the clip at +-1, and between
    quat = rng.normal(0, 1, (N, 4)) * np.array([0.3, 0.3, 1.0, 1.0])
    root[:, 3:7] = quat / np.linalg.norm(quat, axis=-1, keepdims=True)
    s.root.copy_(dev(root))
    pts = dev(np.array(list(s.ap.height_points), np.float32).reshape(140, 2))
    scan = torch.empty((N, 140), device=DEV)
    _abi.check(lib.mg_height_scan(s.sim, pts.data_ptr(), 140, scan.data_ptr(), s.stream()), lib)
    s.post()
    torch.cuda.synchronize()
    assert (s.reset == 0).all(), "no env resets: the scan sees the roots as set"
    want = torch.clip(s.root[:, 2].unsqueeze(1) - 0.5 - scan, -1, 1.) * float(s.ap.height_meas_scale)
    assert torch.equal(s.measured, scan), "measured_heights"
    assert torch.equal(s.obs[:, 36:176], want)
    inside = (np.abs(root[:, 0] - 0.5) < 2.0) & (np.abs(root[:, 1] + 0.5) < 2.0)
    assert (want == 5.0).any() and (want == -5.0).any() and (want.abs() < 5.0).any()
    assert inside.any() and (~inside).any() and len(np.unique(scan.cpu().numpy())) > 20
    s.close()


# ------------------------------------------------------------------------------------------------ the device RNG
@pytest.mark.parametrize("env_offset", [0, 5])
def test_device_rng_matches_its_host_twin(lib, env_offset):
    """tb.noise = NULL: a pushed step of 9 envs, 5 of which reset, equals the restatement fed pyoracle.uniform(seed,
    env_offset + e, step, column) in all 219 columns: state bit for bit, observations (noise columns included) by the
    1e-4 rule; mg_anymal_terrain_reset_idx draws from the | 2^62 stream, skips an id out of range and takes a repeated
    one once"""
    N, seed, step = 9, 20261021, 7
    s, p = golden_sim(lib, N, trace=67)
    g = R.golden()
    st0 = R.golden_state(g, 67, 0)
    st0 = {k: (v[:N].copy() if k != "episode_out" else v.copy()) for k, v in st0.items()}
    st0["progress"][:] = np.where(np.arange(N) % 2 == 0, p["max_episode_length"] - 2, 1)
    ncf = np.zeros((N, s.nb, 3), np.float32)
    actions = g["N67_s0_actions"][:N]
    for counter, manual in ((step, False), (step | (1 << 62), True)):
        noise = np.array([[O.uniform(seed, env_offset + e, counter, c) for c in range(R.COLS)] for e in range(N)],
                         np.float32)
        st = {k: v.copy() for k, v in st0.items()}
        s.load(st)
        if manual:
            ids = [8, 2, 2, 40, -1, 5]
            R.reset_envs(p, st, [2, 5, 8], noise, manual=True)
            s.reset_idx(ids, seed=seed, step=step, env_offset=env_offset)
        else:
            s.actions.copy_(dev(actions))
            out = R.post_step(p, st, ncf, actions, noise, push_now=True)
            s.post(push=True, seed=seed, step=step, env_offset=env_offset)
        torch.cuda.synchronize()
        got, who = s.state(), "reset_idx" if manual else "post"
        for k in BITWISE:
            assert np.array_equal(got[k], st[k]), f"{who}: {k}"
        assert np.array_equal(got["commands"][:, [0, 1, 3]], st["commands"][:, [0, 1, 3]]), who
        for k in ("commands", "episode_sums", "episode_out"):
            assert R.close(got[k], st[k]).all(), f"{who}: {k}"
        if not manual:
            assert (got["reset"] == (np.arange(N) % 2 == 0)).all() and R.close(s.obs.cpu().numpy(), out["obs"]).all()
            assert len(np.unique(got["root"][:, 7:9])) >= 2 * 4, "every pushed env has draws of its own"
        else:
            assert (got["progress"][[2, 5, 8]] == 0).all() and (got["reset"][[2, 5, 8]] == 1).all()
            assert (got["last_actions"][[2, 5, 8]] == 0).all() and (s.mark == 0).all()
    s.close()


# ------------------------------------------------------------------------------------------------ physics
_phys = {}


def effort_states():
    """the standing states of tests/anymal_ref.py under the effort-mode model: efforts from seeded random actions by
    the reference's PD law, the states without a discontinuity in their step (orc_step_flips == 0) first"""
    if _phys:
        return _phys["v"]
    _, _, _, root, dof, _, _ = AR.physics_states("standing")
    n = len(root)
    spec, mnp, sp, ap = R.task_model(R.task_cfg(n))
    p = R.params_from(ap)
    actions = np.random.default_rng(41).uniform(-1, 1, (n, 12)).astype(np.float32)
    _, eff = R.pre_step(p, actions, dof)

    def host(idx):
        h = AR.AnymalHost(spec, root[idx], dof[idx], np.zeros((len(idx), 12), np.float32))
        h.act_eff[:] = eff[idx]
        return h

    flags = PS.step_flags(mnp, sp, host(np.arange(n)))
    order = np.argsort(flags != 0, kind="stable")
    assert (flags[order[:AR.PHYS_SMALL]] == 0).all()
    root, dof, actions, eff = root[order], dof[order], actions[order], eff[order]   # host() reads these from here on
    ref = host(np.arange(n)).simulate(mnp, sp)
    _phys["v"] = spec, mnp, sp, root, dof, actions, eff, ref, host
    return _phys["v"]


@pytest.mark.parametrize("n", [AR.PHYS_SMALL, AR.PHYS_ACTORS])
def test_one_decimation_step_matches_the_oracle(lib, n):
    """mg_anymal_terrain_pre's efforts into one mg_sim_simulate of the effort-mode task model on the plane, at 6 and 66
    actors, against the fp64 oracle stepped with the same efforts: the one-step tolerances and the 5 % exemption cap of
    test_task_model_physics_matches_oracle (tests/anymal_ref.compare_step).  Measured: root pose 1.2e-7, dof pos
    6.0e-8, root twist 1.2e-6, dof vel 1.3e-5, net contact forces 9.0e-4 N; no env outside, none exempt."""
    spec, mnp, sp, root, dof, actions, eff, ref, host = effort_states()
    s = TerrainSim(lib, n, cfg=R.task_cfg(n, **{"terrain.terrainType": "plane"}))
    s.root.copy_(dev(root[:n]))
    s.dof.copy_(dev(dof[:n].reshape(n * 12, 2)))
    s.actions.copy_(dev(actions[:n]))
    s.ncf.fill_(float("nan"))   # every row must be written
    s.pre()
    s.simulate()
    torch.cuda.synchronize()
    assert np.array_equal(s.act.view(n, 12).cpu().numpy(), eff[:n]), "the kernel's efforts are the restatement's"
    got = types.SimpleNamespace(root=s.root.cpu().numpy(), dof=s.dof.view(n, 12, 2).cpu().numpy(),
                                ncf=s.ncf.view(n, s.nb, 3).cpu().numpy())
    s.close()
    for x in (got.root, got.dof, got.ncf):
        assert np.isfinite(x).all()
    assert np.abs(got.dof[..., 0] - dof[:n, :, 0]).max() > 1e-4, "the step moved nothing"
    c_h = ref.ncf[:n]
    test = f"test_one_decimation_step_matches_the_oracle[{n}]"
    checks = [("root pose", got.root[:, 0:7], ref.root[:n, 0:7], 2e-4, 0),
              ("dof pos", got.dof[..., 0], ref.dof[:n, :, 0], 2e-4, 0),
              ("root twist", got.root[:, 7:13], ref.root[:n, 7:13], 2e-3, 2e-3),
              ("dof vel", got.dof[..., 1], ref.dof[:n, :, 1], 2e-3, 2e-3),
              ("net contact forces", got.ncf, c_h, 1e-2 * max(1.0, np.abs(c_h).max()), 0)]
    bad = np.zeros(n, bool)
    for name, a, b, atol, rtol in checks:
        eb = PS.env_bad(a, b, atol, rtol)
        err = np.abs(a.astype(np.float64) - b)
        print(f"{test} {name}: max err {err.max():.3g} (atol {atol:.3g}), envs outside {int(eb.sum())} / {n}")
        PS.record(test, name, a, b, envs_outside=int(eb.sum()), atol=atol, rtol=rtol)
        bad |= eb
    flags = PS.step_flags(mnp, sp, host(np.arange(n)))
    PS.assert_steps_explained(test, bad[None], flags[None], sens=None, reach_cap=PS.REACH_CAP, allow_unexplained=0.0)


@pytest.mark.parametrize("origins", [False, True], ids=["world", "origins"])
def test_decimation_step_matches_the_oracle_on_generated_terrain(lib, origins):
    """The same on the ground the task is for: a terrain generated by migym.terrain.Terrain (heightfield_ref.terrain_case:
    the standing states on its slope, stairs and obstacle maps), in world coordinates as the task runs and once with
    each map's origin as the actors' env origins.  Four launches of (mg_anymal_terrain_pre, mg_sim_simulate), teacher-
    forced: after each the fp64 oracle is stepped on the same field from the state the launch started from with the
    kernel's own efforts, and compared by the rule above (heightfield_ref.terrain_compare; the CPU suite runs it with
    the oracle's fp32 twin in the kernel's place).  Measured (MI355X), worst err / tolerance over the four launches, world
    and origins: root pose 0.014, dof pos 0.18, root twist 0.19, dof vel 0.22 (first launch, the pressed feet pushed
    out; 0.045 by the fourth), net contact forces 0.050; no env flagged, none outside."""
    import heightfield_ref as HF
    c = HF.terrain_case(origins)
    n, fld = c["n"], c["fld"]
    s = TerrainSim(lib, n, cfg=R.task_cfg(n, **{"terrain.terrainType": "plane"}))
    tab = dev(fld.H)
    org = dev(fld.origins) if origins else None
    hf = _abi.Heightfield(heights=tab.data_ptr(), nx=fld.nx, ny=fld.ny, dx=fld.dx, x0=fld.x0, y0=fld.y0, hmax=fld.hmax,
                          env_origins=_abi.ptr(org))
    _abi.check(lib.mg_sim_set_heightfield(s.sim, C.byref(hf)), lib)
    try:
        s.root.copy_(dev(c["root"]))
        s.dof.copy_(dev(c["dof"].reshape(n * 12, 2)))
        s.actions.copy_(dev(c["actions"]))
        for k in range(4):
            root, dof = s.root.cpu().numpy(), s.dof.view(n, 12, 2).cpu().numpy()
            s.ncf.fill_(float("nan"))   # every row must be written
            s.pre()
            s.simulate()
            torch.cuda.synchronize()
            eff = s.act.view(n, 12).cpu().numpy()
            assert np.array_equal(eff, R.pre_step(c["p"], c["actions"], dof)[1]), "the kernel's efforts are the restatement's"
            got = types.SimpleNamespace(root=s.root.cpu().numpy(), dof=s.dof.view(n, 12, 2).cpu().numpy(),
                                        ncf=s.ncf.view(n, s.nb, 3).cpu().numpy())
            test = f"test_decimation_step_on_generated_terrain[{'origins' if origins else 'world'}-launch {k}]"
            _, _, worst = HF.terrain_compare(test, c, got, root, dof, eff)
            PS._REPORT.setdefault(test, {})["err_over_tol"] = worst
    finally:
        s.close()


# ------------------------------------------------------------------------------------------------ the task
def terrain_cfg(N, **env):
    """a generated 2 x 3 curriculum terrain, short episodes, the fixture model"""
    over = {"terrain.numLevels": 2, "terrain.numTerrains": 3, "terrain.maxInitMapLevel": 1,
            "learn.episodeLength_s": 0.3, "learn.pushInterval_s": 0.1, "clipObservations": 5.0, "clipActions": 1.0}
    over.update(env)
    return R.task_cfg(N, **over)


def make_env(N, seed=0, cfg=None):
    np.random.seed(seed)   # the terrain's draws
    return isaacgymenvs.make(seed=seed, task="AnymalTerrain", num_envs=N, sim_device=DEV, rl_device=DEV, headless=True,
                             cfg={"task": cfg or terrain_cfg(N)})


def test_whole_step_equals_the_launches_by_hand(lib):
    """isaacgymenvs.make(AnymalTerrain), 67 envs on a generated terrain: 7 steps of random actions with injected noise
    equal, bit for bit, (pre, simulate) x 4 and post driven by hand on a second sim with the same field; the push
    interval is 5 steps, episodes end after 15 steps (ten envs are moved to the end of theirs)"""
    N = 67
    env = make_env(N)
    assert env.num_obs == 188 and env.num_actions == 12 and env.obs_buf.shape == (N, 188) and env.decimation == 4
    assert (env.progress_buf == 0).all() and (env.reset_buf == 1).all(), "the constructor resets every env"
    assert env.commands.shape == (N, 4) and env.torques.shape == (N, 12) and env.feet_air_time.shape == (N, 4)
    assert env.height_points.shape == (N, 140, 3) and env.measured_heights.shape == (N, 140)
    assert env.terrain_origins.shape == (2, 3, 3) and env.env_origins.shape == (N, 3) and env.push_interval == 5
    assert env.knee_indices.tolist() == [2, 5, 8, 11] and env.feet_indices.tolist() == [3, 6, 9, 12]
    assert env.base_index == 0 and env.max_episode_length == 15 and set(env.episode_sums) == set(_abi.ANYMAL_TERRAIN_REWARDS)
    assert torch.equal(env.env_origins, env.terrain_origins[env.terrain_levels.long(), env.terrain_types.long()])
    assert (env.terrain_levels >= 0).all() and (env.terrain_levels < 2).all() and len(env.terrain_types.unique()) == 3
    t = env.terrain
    table = env._heightfield[0].cpu().numpy()

    def setup(ap):
        ap.hf_nx, ap.hf_ny, ap.hf_dx, ap.hf_x0, ap.hf_y0 = table.shape[0], table.shape[1], 0.1, -20.0, -20.0
        ap.env_length, ap.env_rows, ap.env_cols, ap.custom_origins = t.env_length, t.env_rows, t.env_cols, 1

    s = TerrainSim(lib, N, cfg=terrain_cfg(N), table=table, origins=t.env_origins.astype(np.float32), setup=setup,
                   physics_field=True)
    s.out_pack = torch.full((N, 190), float("nan"), device=DEV)
    pairs = ((s.root, env.root_states), (s.dof, env.dof_state), (s.commands, env.commands), (s.reset, env.reset_buf),
             (s.progress, env.progress_buf), (s.terrain_levels, env.terrain_levels),
             (s.terrain_types, env.terrain_types), (s.env_origins, env.env_origins),
             (s.episode_sums, env._episode_sums), (s.episode_out, env._episode_out))
    for a, b in pairs:
        a.copy_(b)
    rng = np.random.default_rng(9)
    saw_reset = saw_push = False
    for k in range(7):
        noise = rng.uniform(0, 1, (N, R.COLS)).astype(np.float32)
        a = rng.uniform(-1.3, 1.3, (N, 12)).astype(np.float32)
        if k == 2:
            for b in (env.progress_buf, s.progress):
                b[10:20] = 12    # these reach max_episode_length - 1 at the next step
        env.set_reset_noise(dev(noise))
        obs, rew, reset, extras = env.step(dev(a))
        s.noise = dev(noise)
        s.actions.copy_(dev(a))
        for _ in range(4):
            s.pre()
            s.simulate()
        push = (k + 1) % 5 == 0
        s.post(push=push, step=k)
        torch.cuda.synchronize()
        assert torch.equal(env.obs_buf, s.obs) and torch.equal(obs["obs"], s.obs_clamped), f"step {k}"
        assert torch.equal(env.rew_buf, s.rew) and torch.equal(env.reset_buf, s.reset)
        assert torch.equal(env.progress_buf, s.progress) and torch.equal(env.timeout_buf, s.timeout)
        assert torch.equal(env.dof_state, s.dof) and torch.equal(env.root_states, s.root)
        assert torch.equal(env.torques, s.torques) and torch.equal(env.dof_actuation, s.act)
        assert torch.equal(env.net_contact_force_tensor, s.ncf) and torch.equal(env.commands, s.commands)
        assert torch.equal(env.last_actions, s.last_actions) and torch.equal(env.last_dof_vel, s.last_dof_vel)
        assert torch.equal(env.feet_air_time, s.feet_air_time) and torch.equal(env._episode_sums, s.episode_sums)
        assert torch.equal(env.terrain_levels, s.terrain_levels) and torch.equal(env.env_origins, s.env_origins)
        assert torch.equal(env.measured_heights, s.measured) and torch.equal(env._episode_out, s.episode_out)
        assert torch.equal(env.actions, s.actions_out) and torch.equal(rew, s.rew) and torch.equal(reset, s.reset)
        assert torch.equal(extras["episode"]["terrain_level"], s.episode_out[NR])
        assert torch.equal(extras["episode"]["rew_lin_vel_xy"], s.episode_out[0])
        want_pack = torch.cat([s.obs_clamped, s.rew.view(N, 1), s.reset.view(N, 1).to(torch.float32)], 1)
        assert torch.equal(s.out_pack, want_pack), f"step {k}: out_pack is not [clamped obs | rew | reset]"
        assert torch.isfinite(env.obs_buf).all() and extras["time_outs"].dtype == torch.bool
        saw_reset |= bool(reset.any())
        saw_push |= push
    assert saw_reset and saw_push and env.common_step_counter == 7 and (env.progress_buf > 0).any()
    assert torch.equal(env.obs_buf[:, 176:188], env.actions) and env.torques.abs().max() > 1.0
    env.close()
    s.close()


def test_rollout_facts_through_make(lib):
    """64 envs on a generated 2 x 3 curriculum terrain, 40 steps of seeded random actions: everything finite; no
    robot's lowest point more than 5 cm under the lowest of its measured heights; terrain levels in range;
    extras["episode"] changes only on steps with a reset; two runs with the same seed are bit-equal"""
    import tree_physics_ref as TP
    N, steps = 64, 40

    def run():
        env = make_env(N, seed=5, cfg=terrain_cfg(N, **{"learn.episodeLength_s": 0.5}))
        g = torch.Generator().manual_seed(1)
        trace, last = [], None
        for k in range(steps):
            a = (torch.rand((N, 12), generator=g) * 2 - 1).to(DEV)
            obs, rew, reset, extras = env.step(a)
            ep = torch.stack([extras["episode"]["rew_" + n] for n in _abi.ANYMAL_TERRAIN_REWARDS] +
                             [extras["episode"]["terrain_level"]]).clone()
            assert torch.isfinite(obs["obs"]).all() and torch.isfinite(env.root_states).all(), f"step {k}"
            assert torch.isfinite(rew).all() and torch.isfinite(ep).all()
            assert (env.terrain_levels >= 0).all() and (env.terrain_levels < 2).all()
            if last is not None and not bool(reset.any()):
                assert torch.equal(ep, last), f"step {k}: extras['episode'] moved without a reset"
            last = ep
            trace.append((obs["obs"].clone(), rew.clone(), reset.clone(), env.root_states.clone(), ep))
            if k % 13 == 12:
                root, dof = env.root_states.cpu().numpy(), env.dof_pos.cpu().numpy()
                low = np.array([TP.lowest_point(env.model_spec, root[e], dof[e]) for e in range(0, N, 8)])
                floor = env.measured_heights.min(1).values.cpu().numpy()[::8]
                print(f"step {k}: lowest point - lowest measured height {np.min(low - floor):.3f} m")
                assert (low >= floor - 0.05).all(), "a robot is under the terrain"
        resets = sum(int(t[2].sum()) for t in trace)
        levels = env.terrain_levels.clone()
        env.close()
        return trace, resets, levels

    a, resets, levels = run()
    b, _, levels_b = run()
    assert resets >= N, "every episode ends on the way: each env resets at least once"
    assert torch.equal(levels, levels_b)
    for x, y in zip(a, b):
        for u, w in zip(x, y):
            assert torch.equal(u, w), "two runs with the same seed differ"


def test_reset_done_and_env_state_resume(lib):
    """reset_done resets the done envs now; get_env_state / set_env_state resume a rollout bit for bit; set_reset_noise
    takes (N, 219) only"""
    N = 67
    env = make_env(N, seed=3)
    rng = np.random.default_rng(4)
    acts = [dev(rng.uniform(-1, 1, (N, 12)).astype(np.float32)) for _ in range(6)]
    for a in acts[:2]:
        env.step(a)
    env.reset_buf.zero_()
    env.reset_buf[5] = 1
    env.reset_buf[66] = 1
    before = env.dof_state.clone()
    obs0 = env.obs_buf.clone()
    _, done = env.reset_done()
    torch.cuda.synchronize()
    assert done.cpu().tolist() == [5, 66]
    changed = (env.dof_state.view(N, 24) != before.view(N, 24)).any(1).cpu().numpy()
    assert np.array_equal(np.nonzero(changed)[0], [5, 66]) and (env.progress_buf[done] == 0).all()
    assert torch.equal(env.obs_buf, obs0) and (env.last_actions[done] == 0).all()
    assert torch.equal(env.root_states[done, 2], env.env_origins[done, 2] + 0.62)
    snap = env.get_env_state()
    for k in ("commands", "torques", "root_states", "dof_state", "net_contact_force_tensor", "last_actions",
              "last_dof_vel", "feet_air_time", "_episode_sums", "terrain_levels", "env_origins", "progress_buf",
              "reset_buf", "control_steps", "common_step_counter"):
        assert k in snap, k
    outs = []
    for a in acts[2:]:
        o, r, d, _ = env.step(a)
        outs.append((o["obs"].clone(), r.clone(), d.clone(), env.commands.clone(), env.dof_state.clone(),
                     env.terrain_levels.clone()))
    env.commands.zero_()
    env.terrain_levels.fill_(1)
    env.set_env_state(snap)
    assert torch.equal(env.commands, snap["commands"]) and env.common_step_counter == 2
    for a, want in zip(acts[2:], outs):
        o, r, d, _ = env.step(a)
        got = (o["obs"], r, d, env.commands, env.dof_state, env.terrain_levels)
        for x, y in zip(got, want):
            assert torch.equal(x, y), "the resumed rollout differs"
    with pytest.raises(ValueError, match="reset noise"):
        env.set_reset_noise(torch.zeros((N, 27), device=DEV))
    env.close()
