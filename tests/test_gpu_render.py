"""The HIP ray caster (csrc/render.hpp, mg_render) against the fp64 reference (tests/render_ref.py) on the scenes
test_render_host.py vets, plus the plumbing of migym/render.py and VecTask.render.

Compared on the pixels the reference does not mark ambiguous (at most 15 % of an image, asserted without a GPU):
ids equal; |t - t_ref| <= 1e-4 max(1, t_ref) (the project's 1e-4 rule: fp32 FK is off by 1e-6 .. 1e-5 m, divided by
|n . d| >= 0.1); RGB within 1 LSB (the rounding of a value itself within about 1e-4 x 255); sky, +inf and -1 agree.
The scratch records match dynamics_ref.node_frames within 1e-5."""
import ctypes as C

import numpy as np
import pytest
import torch

import render_ref as RR
import migym
from migym import _abi, configs, model as M, render as MR, taskdefs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEL = list(RR.ENV_IDS)


class Scene:
    """a sim handle on a scene's model with the scene's state on the device, and a Renderer on it (no task layer)"""

    def __init__(self, lib, sc):
        self.lib, self.sc = lib, sc
        spec, A = sc["spec"], sc["A"]
        n = RR.N_ENVS * A
        dof = np.stack([sc["q"], np.zeros_like(sc["q"])], -1).astype(np.float32)
        self.root = torch.from_numpy(np.array(sc["root"], np.float32)).to(DEV)
        self.dof = torch.from_numpy(dof.reshape(n * spec.num_dofs, 2)).to(DEV)
        self.act = torch.zeros(n * spec.num_dofs, device=DEV)
        self.boxes = None if sc["boxes"] is None else torch.from_numpy(np.array(sc["boxes"])).to(DEV)
        v = _abi.StateViews()
        v.root_states, v.dof_state, v.dof_actuation = self.root.data_ptr(), self.dof.data_ptr(), self.act.data_ptr()
        self.sensors = torch.zeros((n * max(len(spec.sensors), 1), 6), device=DEV)
        v.sensors = self.sensors.data_ptr()
        sp = taskdefs.sim_params(configs.task_config("Cartpole", 4), 8, A)
        self.mnp = M.pack_model(spec)
        self.sim = C.c_void_p()
        _abi.check(lib.mg_sim_create(self.mnp.ctypes.data, C.byref(sp), n, 0, C.byref(self.sim)), lib)
        self.views = v
        _abi.check(lib.mg_sim_bind(self.sim, C.byref(v)), lib)
        self.r = MR.Renderer(lib, self.sim, spec, RR.N_ENVS, A, DEV, sc["W"], sc["H"], fov_deg=sc["fov_deg"],
                             eye_offset=sc["eye"], target_offset=sc["target"], follow=sc["follow"])

    def render(self, env_ids=SEL, **kw):
        out = self.r.render(env_ids, boxes=self.boxes, **kw)
        torch.cuda.synchronize()
        return {k: v.cpu().numpy().copy() for k, v in out.items()}

    def close(self):
        if self.sim is not None:
            self.lib.mg_sim_destroy(self.sim)
            self.sim = None


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return _abi.lib()


@pytest.fixture(scope="module")
def scenes(lib):
    """name -> (Scene, its image of ENV_IDS with all three outputs, its records): built on first use, shared"""
    made = {}

    def get(name):
        if name not in made:
            s = Scene(lib, RR.scene(name))
            img = s.render(rgb=True, depth=True, ids=True)
            K = 0 if s.boxes is None else s.boxes.shape[1]
            made[name] = (s, img, s.r.scratch_records(len(SEL), K).cpu().numpy().copy())
        return made[name]

    yield get
    for s, _, _ in made.values():
        s.close()


# ------------------------------------------------------------------------------------------------ against the reference
@pytest.mark.parametrize("name", RR.SCENE_NAMES)
def test_image_matches_the_fp64_reference(scenes, name):
    _, img, _ = scenes(name)
    ref = RR.scene_reference(name)
    sc = RR.scene(name)
    assert img["rgb"].shape == (3, sc["H"], sc["W"], 3) and img["rgb"].dtype == np.uint8
    assert img["depth"].shape == (3, sc["H"], sc["W"]) and img["ids"].dtype == np.int32
    worst_t = worst_rgb = 0.0
    for k, r in enumerate(ref):
        ok = ~r["ambiguous"]
        ids, t, rgb = img["ids"][k], img["depth"][k].astype(np.float64), img["rgb"][k].astype(np.int64)
        bad = ok & (ids != r["ids"])
        assert not bad.any(), f"{name} env {SEL[k]}: ids differ at {np.argwhere(bad)[:5].tolist()}"
        sky = r["ids"] < 0
        assert np.isposinf(t[ok & sky]).all() and (ids[ok & sky] == -1).all()
        assert np.isfinite(t[ok & ~sky]).all()
        # everywhere, ambiguous or not: sky, +inf and -1 are one statement
        assert ((ids == -1) == np.isposinf(t)).all()
        m = ok & ~sky
        err = np.abs(t[m] - r["depth"][m]) / np.maximum(1.0, r["depth"][m])
        worst_t = max(worst_t, float(err.max()) if err.size else 0.0)
        drgb = np.abs(rgb - r["rgb"].astype(np.int64)).max(-1)
        worst_rgb = max(worst_rgb, float(drgb[ok].max()))
    print(f"render {name}: max |t - t_ref| / max(1, t_ref) = {worst_t:.2e}, max |rgb - rgb_ref| = {worst_rgb:.0f} LSB")
    assert worst_t <= 1e-4, f"{name}: depth off by {worst_t:.2e} (relative to max(1, t))"
    assert worst_rgb <= 1, f"{name}: rgb off by {worst_rgb:.0f} LSB"


@pytest.mark.parametrize("name", RR.SCENE_NAMES)
def test_scratch_records_match_node_frames(scenes, name):
    _, _, rec = scenes(name)
    ref = RR.scene_reference(name)
    worst = 0.0
    for k, r in enumerate(ref):
        prims = r["prims"]
        assert rec.shape[1] == len(prims)
        for p, row in zip(prims, rec[k]):
            word = int(row[15:16].view(np.uint32)[0])
            assert (word & 0xFF, word >> 8) == (p["type"], p["colour"])
            worst = max(worst, float(np.abs(row[0:9].reshape(3, 3) - p["R"]).max()), float(np.abs(row[9:12] - p["p"]).max()))
            np.testing.assert_array_equal(row[12:15], p["size"].astype(np.float32))
    print(f"render {name}: max |record - node_frames| = {worst:.2e}")
    assert worst <= 1e-5


# ------------------------------------------------------------------------------------------------ plumbing
def test_outputs_are_bit_identical_across_calls_streams_id_forms_and_bound_outputs(scenes):
    s, img, _ = scenes("Ant")
    again = s.render(rgb=True, depth=True, ids=True)
    for k in ("rgb", "depth", "ids"):
        np.testing.assert_array_equal(again[k], img[k])
    side = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        out = s.r.render(SEL, rgb=True, depth=True, ids=True, stream=side)
    side.synchronize()
    for k in ("rgb", "depth", "ids"):
        np.testing.assert_array_equal(out[k].cpu().numpy(), img[k])
    # a device id tensor is the host list
    dev_ids = s.render(torch.tensor(SEL, dtype=torch.int32, device=DEV), rgb=True, depth=True, ids=True)
    for k in ("rgb", "depth", "ids"):
        np.testing.assert_array_equal(dev_ids[k], img[k])
    # one output bound at a time
    for k in ("rgb", "depth", "ids"):
        one = s.render(**{"rgb": False, k: True})
        assert list(one) == [k]
        np.testing.assert_array_equal(one[k], img[k])
    # env_ids=None is the first envs in order
    first = s.render([0, 1, 2], rgb=True, depth=True, ids=True)
    every = s.render(None, rgb=True, depth=True, ids=True)
    assert every["rgb"].shape[0] == RR.N_ENVS
    for k in ("rgb", "depth", "ids"):
        np.testing.assert_array_equal(every[k][:3], first[k])
    # the selection [4, 0, 2] is rows 4, 0, 2 of the full render
    for k in ("rgb", "depth", "ids"):
        np.testing.assert_array_equal(every[k][SEL], img[k])


def test_argument_errors_return_einval_with_a_message_and_write_nothing(scenes, lib):
    s, _, _ = scenes("Ant")
    W, H = s.r.width, s.r.height
    rgb = torch.full((1, H, W, 3), 7, dtype=torch.uint8, device=DEV)
    depth = torch.full((1, H, W), 7.0, device=DEV)
    ids = torch.full((1, H, W), 7, dtype=torch.int32, device=DEV)
    scratch = torch.full((int(lib.mg_render_scratch_floats(s.sim, 1, 0)),), 7.0, device=DEV)
    assert scratch.numel() == MR.num_primitives(s.sc["spec"], 1, 0) * 16

    def args(**kw):
        a = _abi.RenderArgs()
        a.width, a.height, a.fov_y, a.follow, a.n_sel = W, H, 1.0, 1, 1
        a.eye_offset[:], a.target_offset[:] = (1.0, -1.0, 1.0), (0.0, 0.0, 0.0)
        a.scratch, a.rgb, a.depth, a.ids = scratch.data_ptr(), rgb.data_ptr(), depth.data_ptr(), ids.data_ptr()
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    cases = {"width": args(width=0), "height": args(height=-3), "fov": args(fov_y=0.0), "fov > pi": args(fov_y=3.5),
             "outputs": args(rgb=None, depth=None, ids=None), "n_sel": args(n_sel=0), "scratch": args(scratch=None),
             "n_sel > N": args(n_sel=RR.N_ENVS + 1), "boxes": args(num_boxes=2, boxes=None),
             "view along z": args(target_offset=(C.c_float * 3)(1.0, -1.0, 0.0))}
    for what, a in cases.items():
        rc = lib.mg_render(s.sim, C.byref(a), None)
        assert rc == -1, what
        assert lib.mg_last_error().startswith(b"mg_render:"), what
    # an unbound state
    other = C.c_void_p()
    sp = taskdefs.sim_params(configs.task_config("Cartpole", 4), 8, 1)
    _abi.check(lib.mg_sim_create(s.mnp.ctypes.data, C.byref(sp), RR.N_ENVS, 0, C.byref(other)), lib)
    try:
        a = args()
        assert lib.mg_render(other, C.byref(a), None) == -1 and b"not bound" in lib.mg_last_error()
    finally:
        lib.mg_sim_destroy(other)
    # more primitives than the LDS stage holds: MG_ECAPACITY
    a = args(num_boxes=600, boxes=scratch.data_ptr())
    assert lib.mg_render(s.sim, C.byref(a), None) == -4 and b"512" in lib.mg_last_error()
    torch.cuda.synchronize()
    assert (rgb == 7).all() and (depth == 7).all() and (ids == 7).all() and (scratch == 7).all()
    # the host list is checked in Python
    with pytest.raises(ValueError):
        s.r.render([0, RR.N_ENVS])
    # a device list cannot be (nothing synchronises): the id out of range renders as sky, its neighbours as they are
    out = s.render(torch.tensor([4, 99, -1, 2], dtype=torch.int32, device=DEV), rgb=True, depth=True, ids=True)
    _, img, _ = scenes("Ant")
    for k in ("rgb", "depth", "ids"):
        np.testing.assert_array_equal(out[k][0], img[k][0])
        np.testing.assert_array_equal(out[k][3], img[k][2])
    assert (out["ids"][1:3] == -1).all() and np.isposinf(out["depth"][1:3]).all()
    assert len(np.unique(out["rgb"][1:3].reshape(-1, 3), axis=0)) == 1


def make(task, n, **kw):
    return migym.make(seed=3, task=task, num_envs=n, sim_device=DEV, rl_device=DEV, headless=True, **kw)


def test_rendering_between_steps_leaves_the_rollout_bit_equal():
    n, steps = 16, 8
    g = torch.Generator().manual_seed(5)
    acts = [(torch.rand((n, 8), generator=g) * 2 - 1).to(DEV) for _ in range(steps)]
    runs = []
    for render in (False, True):
        env = make("Ant", n)
        rec = []
        for a in acts:
            obs, rew, reset, _ = env.step(a)
            rec.append((obs["obs"].clone(), rew.clone(), reset.clone()))
            if render:
                out = env.render_envs([1, 3], rgb=True, depth=True, ids=True)
                assert out["rgb"].shape[0] == 2 and out["rgb"].is_cuda
        torch.cuda.synchronize()
        runs.append(rec)
        env.close()
    for (o0, r0, d0), (o1, r1, d1) in zip(*runs):
        assert torch.equal(o0, o1) and torch.equal(r0, r1) and torch.equal(d0, d1)


def test_render_returns_a_frame_under_virtual_screen_capture_and_none_otherwise():
    env = make("Ant", 4, virtual_screen_capture=True)
    env.step(torch.zeros((4, 8), device=DEV))
    frame = env.render()
    st = taskdefs.render_settings("Ant", env.cfg)
    assert isinstance(frame, np.ndarray) and frame.dtype == np.uint8 and frame.shape == (st["height"], st["width"], 3)
    colours = np.unique(frame.reshape(-1, 3), axis=0)
    assert len(colours) > 1
    # the ant is in the picture: some pixel wears a body colour's hue (not a grey, not the sky)
    ids = env.render_envs([0], rgb=False, ids=True)["ids"][0].cpu().numpy()
    assert ((ids >= 0) & (ids < len(env.model_spec.geoms))).sum() > 50
    assert env.render(mode="human") is None
    env.close()
    env = make("Ant", 4)
    env.step(torch.zeros((4, 8), device=DEV))
    assert env.render() is None
    env.close()


@pytest.mark.parametrize("task,nact", [("Cartpole", 1), ("Humanoid", 21), ("ShadowHand", 20), ("MAAnt", 8)])
def test_default_cameras_show_the_model(task, nact):
    cfg = configs.task_config(task, 4, sim_device=DEV)
    cfg["env"]["render"] = {"width": 53, "height": 41}
    env = make(task, 4, virtual_screen_capture=True, cfg={"task": cfg})
    env.step(torch.zeros((env.num_actors, nact), device=DEV))
    frame = env.render()
    assert frame.shape == (41, 53, 3)
    ids = env.render_envs(None, rgb=False, ids=True)["ids"].cpu().numpy()
    assert ids.shape == (4, 41, 53)
    ngeom = env.num_agents * len(env.model_spec.geoms)
    for e in range(4):
        assert ((ids[e] >= 0) & (ids[e] < ngeom)).sum() >= 20, f"{task} env {e}: the model is not in the default view"
    if task == "ShadowHand":   # the object and the goal follow the hand's geoms
        assert (ids == ngeom).any() and (ids == ngeom + 1).any()
    env.close()


def test_franka_reach_cubes_are_drawn_as_extra_boxes():
    import franka_reach_ref as FR
    A, T, N = 3, 2, 4
    cfg = FR.golden_cfg(A, T, N)
    cfg["env"]["render"] = {"width": 160, "height": 120}
    env = make("FrankaReachMA", N, virtual_screen_capture=True, cfg={"task": cfg})
    env.step(torch.zeros((env.num_actors, 6), device=DEV))
    boxes = env.render_boxes()
    assert boxes.shape == (N, T, 10)
    assert torch.equal(boxes[..., 0:7], env._cubeA_state[..., 0:7]) and (boxes[..., 7:10] == 0.5 * env.cubeA_size).all()
    frame = env.render()
    assert frame.shape == (120, 160, 3) and frame.dtype == np.uint8
    ids = env.render_envs(None, rgb=False, ids=True)["ids"].cpu().numpy()
    first = A * len(env.model_spec.geoms)
    assert ids.max() == first + T                       # the ground, after the cubes
    for e in range(N):
        for k in range(T):
            assert (ids[e] == first + k).sum() >= 2, f"env {e}: cube {k} is not in the default view"
    env.close()


def test_anymal_default_camera_shows_the_robot():
    import anymal_ref as AR
    cfg = AR.task_cfg(4)
    cfg["env"]["render"] = {"width": 53, "height": 41}
    env = make("Anymal", 4, virtual_screen_capture=True, cfg={"task": cfg})
    env.step(torch.zeros((4, 12), device=DEV))
    assert env.render().shape == (41, 53, 3)
    ids = env.render_envs(None, rgb=False, ids=True)["ids"].cpu().numpy()
    ngeom = len(env.model_spec.geoms)
    for e in range(4):
        assert ((ids[e] >= 0) & (ids[e] < ngeom)).sum() >= 20, f"Anymal env {e}: the robot is not in the default view"
    env.close()
