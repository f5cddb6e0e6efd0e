"""GPU parity of the device dynamics registry (include/dqp.h dqp_dyn_*) against
the golden vectors of tests/golden/DYN_*.npz (the reference's CasADi-generated C for the robots,
its torch modules for the pendulums; make_golden_dyn.py) and against the reference's compiled C on 4000 of the
random states of a full-size call (tests/golden/DYNFULL_*.npz, make_golden_dynfull.py).  Tolerances (absolute, values O(1-10)):
states 1e-12, Jacobians 1e-11."""
import glob
import os

import numpy as np
import pytest
import torch

from oracle import dyn_ref

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ["pendulum1l", "cartpole1l", "cartpole2l", "pendulum_euler", "pendulum_dx", "rexquadrotor"]


def dev(a):
    return torch.tensor(np.asarray(a), dtype=torch.float64, device="cuda")


@pytest.fixture(scope="module")
def dynmod():
    assert torch.cuda.is_available()
    from diff_qp_mpc_amd import dynamics, _lib
    _lib.load()
    return dynamics


@pytest.mark.parametrize("name", NAMES)
def test_step_and_jacobian_vs_golden(dynmod, name):
    g = np.load(os.path.join(GOLDEN, "DYN_%s.npz" % name))
    dyn = dynmod.DeviceDynamics(name, dt=float(g["dt"]))
    assert (dyn.n_state, dyn.n_ctrl) == (g["x"].shape[1], g["u"].shape[1])
    x, u = dev(g["x"]), dev(g["u"])
    np.testing.assert_allclose(dyn(x, u).cpu().numpy(), g["x_next"], rtol=0, atol=1e-12)
    xn, (Jx, Ju) = dyn.jac(x, u)
    np.testing.assert_allclose(xn.cpu().numpy(), g["x_next"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(Jx.cpu().numpy(), g["Jx"], rtol=0, atol=1e-11)
    np.testing.assert_allclose(Ju.cpu().numpy(), g["Ju"], rtol=0, atol=1e-11)


@pytest.mark.parametrize("name", NAMES[:3])
def test_extension_interface_vs_golden(dynmod, name):
    """dynamics(q, qdot, tau, h) / derivatives(...) of deqmpc/my_envs/*: per-sample h, full tau,
    six raw blocks."""
    g = np.load(os.path.join(GOLDEN, "DYN_%s.npz" % name))
    dyn = dynmod.DeviceDynamics(name)
    q, qd, tau, h = dev(g["q"]), dev(g["qd"]), dev(g["tau"]), dev(g["h"])
    qo, qdo = dyn.forward_dynamics(q, qd, tau, h)
    np.testing.assert_allclose(qo.cpu().numpy(), g["q_out"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(qdo.cpu().numpy(), g["qd_out"], rtol=0, atol=1e-12)
    for i, b in enumerate(dyn.forward_derivatives(q, qd, tau, h)):
        np.testing.assert_allclose(b.cpu().numpy(), g["blk%d" % i], rtol=0, atol=1e-11, err_msg="block %d" % i)


@pytest.mark.parametrize("name", NAMES[:3])
def test_vs_compiled_reference_full_size(dynmod, name):
    """B x (T-1) = 4096 x 19 knots (the config-3 Jacobian call): 4000 sampled knots against the reference's compiled C
    (its outputs on exactly these states, stored by tests/golden/make_golden_dynfull.py)."""
    nq = dyn_ref.ROBOTS[name]
    N = 4096 * 19
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.uniform(-np.pi, np.pi, (N, nq)), rng.uniform(-8, 8, (N, nq))], 1)
    u = rng.uniform(-100, 100, (N, 1))
    dyn = dynmod.DeviceDynamics(name, dt=0.05)
    xn, (Jx, Ju) = dyn.jac(dev(x), dev(u))
    sub = rng.choice(N, 4000, replace=False)            # the knots the reference's outputs are stored for
    parts = [np.load(p) for p in sorted(glob.glob(os.path.join(GOLDEN, "DYNFULL_%s_*.npz" % name)))]
    g = {k: np.concatenate([p[k] for p in parts]) for k in ("sub", "x", "u", "x_next", "Jx", "Ju")}
    np.testing.assert_array_equal(g["sub"], sub)       # the same states as the stored reference outputs
    np.testing.assert_array_equal(g["x"], x[sub])
    np.testing.assert_array_equal(g["u"], u[sub])
    ref, rJx, rJu = g["x_next"], g["Jx"], g["Ju"]
    scale = 1.0 + np.abs(ref).max()
    np.testing.assert_allclose(xn.cpu().numpy()[sub], ref, rtol=0, atol=1e-12 * scale)
    np.testing.assert_allclose(Jx.cpu().numpy()[sub], rJx, rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(Ju.cpu().numpy()[sub], rJu, rtol=1e-10, atol=1e-10)
    assert bool(torch.isfinite(xn).all()) and bool(torch.isfinite(Jx).all())


@pytest.mark.parametrize("name", NAMES)
def test_autograd_through_the_step(dynmod, name):
    """DeviceDynamics.forward is differentiable (vector-Jacobian products from the Jacobian kernel):
    compare with central differences of the kernel itself."""
    dyn = dynmod.DeviceDynamics(name)
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn(16, dyn.n_state, dtype=torch.float64, device="cuda", generator=g)
    if name == "pendulum_dx":
        x[:, :2] = torch.nn.functional.normalize(x[:, :2], dim=1)
    u = torch.randn(16, dyn.n_ctrl, dtype=torch.float64, device="cuda", generator=g)
    if name == "rexquadrotor":
        x, u = 0.3 * x, 14.5 + u
    w = torch.randn(16, dyn.n_state, dtype=torch.float64, device="cuda", generator=g)
    xr, ur = x.clone().requires_grad_(), u.clone().requires_grad_()
    (dyn(xr, ur) * w).sum().backward()
    e = 1e-6
    for j in range(dyn.n_state):
        d = torch.zeros_like(x); d[:, j] = e
        fd = ((dyn(x + d, u) - dyn(x - d, u)) * w).sum(1) / (2 * e)
        np.testing.assert_allclose(xr.grad[:, j].cpu().numpy(), fd.cpu().numpy(), rtol=1e-6, atol=1e-7)
    for j in range(dyn.n_ctrl):
        d = torch.zeros_like(u); d[:, j] = e
        fd = ((dyn(x, u + d) - dyn(x, u - d)) * w).sum(1) / (2 * e)
        np.testing.assert_allclose(ur.grad[:, j].cpu().numpy(), fd.cpu().numpy(), rtol=1e-6, atol=1e-7)


def test_bad_arguments(dynmod):
    import ctypes
    from diff_qp_mpc_amd import _lib
    lib = _lib.load()
    assert lib.dqp_dyn_sizes(99, None, None) == -1
    assert lib.dqp_dyn_step(99, 4, None, None, 0.05, None, None) == -1
    assert lib.dqp_dyn_step(2, 4, None, None, 0.05, None, None) == -1       # null pointers
    assert lib.dqp_dyn_step(2, 0, None, None, 0.05, None, None) == 0        # empty batch
    assert lib.dqp_dyn_forward_dynamics(5, 4, *([None] * 7)) == -1          # not a robot
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dynmod.DeviceDynamics("cartpole1l")(torch.zeros(2, 4, dtype=torch.float64), torch.zeros(2, 1, dtype=torch.float64))
    with pytest.raises(ValueError):
        dynmod.DeviceDynamics("acrobot")


def test_recognise_a_callers_module():
    """dynamics.recognise: a caller's torch module that IS a registered model (here: the pendulum of deqmpc/envs.py
    restated in torch, and a registered model behind an opaque wrapper) is matched numerically and returned as the
    device model; a different map (another step size, a perturbed model) is not."""
    from diff_qp_mpc_amd.dynamics import DeviceDynamics, recognise
    from test_gpu_al import Pendulum

    m = recognise(Pendulum(), 2, 1)
    assert isinstance(m, DeviceDynamics) and m.name == "pendulum_euler" and m.dt == 0.05

    class Wrap(torch.nn.Module):
        def __init__(self, d, scale=1.0):
            super().__init__()
            self.d, self.dt, self.scale = d, d.dt, scale

        def forward(self, x, u):
            return self.d(x, u * self.scale)

    for name in ("cartpole1l", "cartpole2l", "rexquadrotor", "pendulum_dx"):
        d = DeviceDynamics(name, dt=0.03)
        got = recognise(Wrap(d), d.n_state, d.n_ctrl)
        assert got is not None and got.name == name and got.dt == 0.03
        assert recognise(Wrap(d, scale=1.01), d.n_state, d.n_ctrl) is None          # a different model
    assert recognise(Pendulum(), 2, 1, dt=0.04) is None                               # a different step
    assert recognise(torch.nn.Linear(3, 3), 3, 1) is None                             # not a dynamics callable at all


def test_tracking_mpc_recognises_env_module():
    """policies.Tracking_MPC handed the env's torch module (as the reference's policies.py:571-572 does) solves on the
    registered device model when the module is one: same trajectories as with the DeviceDynamics passed explicitly."""
    import argparse, types
    from diff_qp_mpc_amd import policies
    from diff_qp_mpc_amd.dynamics import DeviceDynamics
    from test_gpu_al import Pendulum, PendulumJac
    B, T = 16, 5
    outs = []
    for dyn, jac in ((Pendulum(), PendulumJac()), (DeviceDynamics("pendulum_euler"), None)):
        env = types.SimpleNamespace(nx=2, nu=1, nq=1, dt=0.05, dynamics=dyn, dynamics_derivatives=jac if jac is not None else dyn.jac,
                                    action_space=types.SimpleNamespace(high=np.array([2.0]), low=np.array([-2.0])))
        args = argparse.Namespace(T=T, nq=1, hdim=32, layer_type="mlp", deq_out_type=1, policy_out_type=1, deq_iter=2,
                                  solver_type="al", qp_iter=1, eps=1e-2, warm_start=True, bsz=B, Q=torch.ones(2),
                                  R=1e-2 * torch.ones(1), dtype="double", device="cuda")
        torch.manual_seed(0)
        trk = policies.Tracking_MPC(args, env)
        assert isinstance(trk.dyn, DeviceDynamics)
        gen = torch.Generator(device="cuda").manual_seed(1)
        x0 = torch.rand(B, 2, device="cuda", generator=gen) - 0.5
        x_ref = x0[:, None, :] * torch.linspace(1, 0, T, device="cuda")[None, :, None]
        u_ref = torch.zeros(B, T, 1, device="cuda")
        trk.reinitialize(x0, torch.ones(B, T, 1, device="cuda"))
        xs, us = trk(x0, torch.cat([x_ref, u_ref], -1), x_ref, u_ref)
        outs.append((xs.detach().cpu().numpy(), us.detach().cpu().numpy()))
    np.testing.assert_array_equal(outs[0][0], outs[1][0])
    np.testing.assert_array_equal(outs[0][1], outs[1][1])


def test_device_sincos_against_libm_over_ranges():
    """The models' device sin/cos (csrc/dqp_dyn_models.h sincos_) through the pendulum model, whose step is x' = [th + dt (w + dt (u + 10 sin th)), w + dt (u +
    10 sin th)]: against numpy's libm over six decades of angles, near multiples of pi/2, and at non-finite input."""
    from diff_qp_mpc_amd.dynamics import DeviceDynamics
    d = DeviceDynamics("pendulum_euler", dt=1.0)
    rng = np.random.default_rng(0)
    for scale in (1.0, 10.0, 1e3, 1e5, 1e7, 1e12):
        th = rng.uniform(-scale, scale, 20000)
        th[::5] = np.rint(th[::5] / (np.pi / 2)) * (np.pi / 2) + rng.uniform(-1e-9, 1e-9, th[::5].shape)
        x = torch.tensor(np.stack([th, np.zeros_like(th)], 1), device="cuda")
        u = torch.zeros(len(th), 1, dtype=torch.float64, device="cuda")
        w = d(x, u)[:, 1].cpu().numpy()                       # = 10 sin th
        np.testing.assert_allclose(w, 10.0 * np.sin(th), rtol=0, atol=4e-15)
        _, (Jx, _) = d.jac(x, u)                                # d w' / d th = 10 cos th
        np.testing.assert_allclose(Jx[:, 1, 0].cpu().numpy(), 10.0 * np.cos(th), rtol=0, atol=4e-15)
    bad = torch.tensor([[float("inf"), 0.0], [float("nan"), 0.0]], dtype=torch.float64, device="cuda")
    out = d(bad, torch.zeros(2, 1, dtype=torch.float64, device="cuda"))
    assert bool(torch.isnan(out[:, 1]).all())
