"""Known-answer test of the polynomial sine / cosine (device_math.hpp ``poly_sincos``, the physics' pair outside the
16-lane instances) on the host, over the inputs the VERDICT r5 fault review names: NaN, +-Inf, +-1e30, denormals, and the angles a
Cartpole rollout actually visits ("the physics' sine / cosine").

Both forms are checked: the float-quadrant form (quadrant = k - 4 floor(k / 4) in floating point, picked by float
compares) and round 5's integer-quadrant form ((int)rint(x 2/pi) & 3).  The property that matters for a fault is that
no input, finite or not, can make the result depend on anything but selects of in-range values: finite inputs within
|x| <= 1e4 give sin / cos within 3e-7 + 2 ulp(|x|) of the fp64 values, |x| <= pi within 2.5e-7; NaN and +-Inf give
NaN; huge finite inputs give some value (the reduction has no precision left there) without faulting; denormals give
sin x = x (bit for bit; a signed zero may come out +0) and cos x = 1.  Compiled with hipcc for the host (--cuda-host-only): no GPU needed.
"""
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "isaacgymenvs-ma_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

SRC = r"""
#include "device_math.hpp"
#include <cstdio>
#include <cstring>
int main(int argc, char** argv) {
  const bool iq = argc > 1 && !strcmp(argv[1], "int");
  unsigned u;
  while (scanf("%x", &u) == 1) {
    float x;
    memcpy(&x, &u, 4);
    float s, c;
    mg::poly_sincos(x, &s, &c, iq);
    unsigned su, cu;
    memcpy(&su, &s, 4);
    memcpy(&cu, &c, 4);
    printf("%08x %08x\n", su, cu);
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def kat_bin():
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("hipcc not available")
    d = tempfile.mkdtemp(prefix="trig_kat_")
    src, exe = os.path.join(d, "kat.hip"), os.path.join(d, "kat")
    with open(src, "w") as f:
        f.write(SRC)
    subprocess.run([HIPCC, "-O2", "-std=c++17", "--cuda-host-only", "-I", CSRC, "-o", exe, src], check=True,
                   capture_output=True)
    yield exe
    shutil.rmtree(d, ignore_errors=True)


def _run(exe, xs, form):
    xs = np.asarray(xs, np.float32)
    inp = "\n".join(f"{u:08x}" for u in xs.view(np.uint32)) + "\n"
    out = subprocess.run([exe, form], input=inp, capture_output=True, text=True, check=True).stdout.split()
    v = np.array([int(w, 16) for w in out], np.uint32).view(np.float32).reshape(-1, 2)
    return v[:, 0], v[:, 1]


def _cartpole_angles():
    """the pole angles / velocities of a random-action Cartpole rollout on the CPU oracle (the inputs the faulting
    instance's FK saw), plus reset-range draws"""
    rng = np.random.default_rng(0)
    x = [rng.uniform(-0.2, 0.2, 4096), rng.uniform(-np.pi / 2 - 0.3, np.pi / 2 + 0.3, 4096)]
    import sys
    sys.path.insert(0, os.path.join(ROOT, "isaacgymenvs-ma_amd"))
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import pyoracle as O
    from migym import configs, model as M, taskdefs
    cfg = configs.task_config("Cartpole", 256)
    spec = M.load_builtin(taskdefs.TASK_INFO["Cartpole"][1])
    sp = taskdefs.sim_params(cfg, taskdefs.TASK_INFO["Cartpole"][5], 1)
    tp = taskdefs.task_params("Cartpole", cfg, spec)
    mnp = M.pack_model(spec)
    h = O.HostEnv(tp, spec, 256)
    for k in range(60):   # test_out_pack_rows_equal_step_outputs[Cartpole]'s actions: U(-1.2, 1.2)
        h.actions[:] = rng.uniform(-1.2, 1.2, h.actions.shape).astype(np.float32)
        h.env_step(mnp, sp, tp, 0, k, 1, fp32=True)
        x.append(np.asarray(h.dof, np.float32).reshape(-1))
    return np.concatenate(x).astype(np.float32)


@pytest.mark.parametrize("form", ["float", "int"])
def test_poly_sincos_known_answers(kat_bin, form):
    rng = np.random.default_rng(1)
    small = np.concatenate([np.linspace(-np.pi, np.pi, 20001), rng.uniform(-np.pi, np.pi, 20000)]).astype(np.float32)
    s, c = _run(kat_bin, small, form)
    x64 = small.astype(np.float64)
    assert np.max(np.abs(s - np.sin(x64))) <= 2.5e-7 and np.max(np.abs(c - np.cos(x64))) <= 2.5e-7
    wide = np.concatenate([rng.uniform(-1e4, 1e4, 20000), _cartpole_angles()]).astype(np.float32)
    s, c = _run(kat_bin, wide, form)
    x64 = wide.astype(np.float64)
    tol = 3e-7 + 2.0 * np.spacing(np.abs(wide)).astype(np.float64)
    assert np.all(np.abs(s - np.sin(x64)) <= tol) and np.all(np.abs(c - np.cos(x64)) <= tol)
    # non-finite inputs: NaN out (no exception, no garbage index: the quadrant only ever feeds selects)
    s, c = _run(kat_bin, [np.nan, -np.nan, np.inf, -np.inf], form)
    assert np.all(np.isnan(s)) and np.all(np.isnan(c))
    # huge finite inputs: the reduction has no precision left, but the call returns
    s, c = _run(kat_bin, [1e30, -1e30, 3.4e38, -3.4e38, 1e20, 8388609.0], form)
    assert s.shape == (6,) and c.shape == (6,)
    # denormals and signed zeros
    den = np.array([1e-45, -1e-45, 1e-40, -3e-39, 0.0, -0.0], np.float32)
    s, c = _run(kat_bin, den, form)
    assert np.array_equal(s[:4].view(np.uint32), den[:4].view(np.uint32)) and np.all(s[4:] == 0.0) and np.all(c == 1.0)
