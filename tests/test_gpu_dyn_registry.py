"""The (entry point that takes a model) x (registered model) cells that no other GPU test runs, at the smallest shapes:
T = 4 and B = 3, or B = 5 where the kernel packs four problems into a wavefront, so that one group is partial.  Each is
checked the way its neighbours are: dqp_mpc_linearize against DeviceDynamics.jac (test_gpu_mpc_sqp.py, 1e-12), the fused
line search and rollout against their torch restatements (test_gpu_mpc.py: 1e-10 / 1e-12 and 1e-10), the true-dynamics
residual of the stage-wise kernels against that of the dense ones (test_gpu_ric.py: rtol 1e-5 / atol 1e-7), one round of
dqp_mpc_sqp_rounds against the Python round (test_gpu_mpc_sqp.py), dqp_al_outer_update and dqp_al_newton_solve against
oracle/al_solve_oracle.py on the device model's own Jacobians (test_gpu_al_bounds.py)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
F64 = dict(dtype=torch.float64, device="cuda")
T = 4


def setup(robot, B, seed):
    """the model, a generator of normal samples, and starting states / controls of test_gpu_mpc_sqp.problem"""
    from test_gpu_mpc_sqp import problem
    p = problem(robot, T, B)
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64).cuda()
    return p, rnd


def make_mpc(p, **kw):
    from diff_qp_mpc_amd import qp_wrapper
    return qp_wrapper.MPC(p["n"], p["m"], T, u_lower=p["lo"], u_upper=p["hi"], n_batch=p["B"], verbose=-1, **kw)


@pytest.mark.parametrize("robot", ["pendulum1l", "pendulum_euler"])
def test_linearize(robot):
    from diff_qp_mpc_amd import _lib
    from diff_qp_mpc_amd.qp_wrapper import bmv
    B = 3
    p, rnd = setup(robot, B, 11)
    dyn, n, m = p["dyn"], p["n"], p["m"]
    x = (p["x0"][None] + 0.2 * rnd(T, B, n)).contiguous()
    u = (p["u0"] + 0.3 * rnd(T, B, m)).contiguous()
    F = torch.full((T - 1, B, n, n + m), float("nan"), **F64)
    f = torch.full((T - 1, B, n), float("nan"), **F64)
    _lib.call("dqp_mpc_linearize", torch.device("cuda"), _lib.dqp_mpc_dims(B, n, m, T, 1, dyn.id), dyn.dt, x, u, F, f)
    xs, us = x[:-1].reshape(-1, n), u[:-1].reshape(-1, m)
    nxt, (Jx, Ju) = dyn.jac(xs, us)
    F_ref = torch.cat((Jx, Ju), dim=2)
    f_ref = nxt - bmv(F_ref, torch.cat((xs, us), dim=1))
    np.testing.assert_allclose(F.reshape(-1, n, n + m).cpu().numpy(), F_ref.cpu().numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(f.reshape(-1, n).cpu().numpy(), f_ref.cpu().numpy(), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("robot", ["pendulum1l"])
def test_line_search(robot, monkeypatch):
    """one sample accepts the full step, one backtracks, one exhausts max_linesearch_iter"""
    from diff_qp_mpc_amd import qp_wrapper
    B = 3
    p, rnd = setup(robot, B, 0)
    dyn, n, m = p["dyn"], p["n"], p["m"]
    mpc = make_mpc(p, max_linesearch_iter=4, linesearch_decay=0.3)
    u = p["u0"] + 0.3 * rnd(T, B, m)
    x = mpc.rollout(p["x0"], u, dyn)
    du = rnd(T, B, m) * torch.logspace(-3, 1.5, B, **F64)[None, :, None]
    outs = {}
    for fused in (True, False):
        monkeypatch.setattr(qp_wrapper, "FUSED_LINE_SEARCH", fused)
        with torch.no_grad():
            outs[fused] = mpc.line_search(x, u, torch.zeros_like(x), du, dyn, p["x0"], qp_wrapper.QuadCost(p["C"], p["c"]))
    for a, b, k in zip(outs[True], outs[False], ("x_new", "u_new", "alpha", "cost")):
        np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=1e-10, atol=1e-10, err_msg=k)


@pytest.mark.parametrize("robot", ["pendulum1l", "cartpole2l", "pendulum_euler", "rexquadrotor"])
def test_rollout_and_its_adjoint(robot, monkeypatch):
    from diff_qp_mpc_amd import qp_wrapper
    B = 3
    p, rnd = setup(robot, B, 4)
    dyn, n, m = p["dyn"], p["n"], p["m"]
    uv, w = p["u0"] + 0.5 * rnd(T, B, m), rnd(T, B, n)
    mpc = make_mpc(p)
    res = {}
    for fused in (True, False):
        monkeypatch.setattr(qp_wrapper, "FUSED_LINE_SEARCH", fused)
        x0, u = p["x0"].clone().requires_grad_(), uv.clone().requires_grad_()
        xs = mpc.rollout(x0, u, dyn)
        res[fused] = [xs.detach()] + list(torch.autograd.grad((xs * w).sum(), (x0, u)))
    np.testing.assert_allclose(res[True][0].cpu().numpy(), res[False][0].cpu().numpy(), rtol=1e-12, atol=1e-12)
    for a, b in zip(res[True][1:], res[False][1:]):
        np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=1e-10, atol=1e-10)


@pytest.mark.parametrize("robot", ["pendulum1l", "pendulum_euler", "integrator"])
def test_true_dynamics_residual_stagewise_equals_dense(robot, monkeypatch):
    """model_residuals of the stage-wise kernels (pendulum1l is run by no other test) and true_dyn_res of the dense ones
    (none of the three is): same trajectories and gradients"""
    from diff_qp_mpc_amd import _lib, qp_wrapper
    B = 5
    p, _ = setup(robot, B, 0)
    dyn = p["dyn"]
    outs = {}
    for fused in (True, False):
        monkeypatch.setattr(qp_wrapper, "FUSED_MPC_QP", fused)
        C, c = p["C"].clone().requires_grad_(), p["c"].clone().requires_grad_()
        mpc = make_mpc(p, single_qp_solve=True)
        with _lib.trace() as tr:
            x, u = mpc(p["x0"], qp_wrapper.QuadCost(C, c), dyn, dyn.jac)
        kernels = [k for k, _ in tr.records]
        assert any("ric::forward_kernel" in k for k in kernels) == fused, kernels
        # the dense route's generic kernel: with a model it is the only forward the library launches there
        assert any("qp_forward_kernel<" in k for k in kernels) == (not fused), kernels
        (x.sum() + 2.0 * u.sum()).backward()
        outs[fused] = [t.detach().cpu().numpy() for t in (x, u, C.grad, c.grad)]
    for a, b, k in zip(outs[True], outs[False], ("x", "u", "dC", "dc")):
        print(robot, k, "max |stage-wise - dense| = %.3e" % float(np.abs(a - b).max()))
    for a, b, k in zip(outs[True], outs[False], ("x", "u", "dC", "dc")):
        np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-7, err_msg=k)


@pytest.mark.parametrize("robot", ["pendulum1l", "pendulum_euler"])
def test_one_sqp_round_equals_the_python_round(robot):
    """B = 5: the stage-wise kernels pack four problems into a wavefront"""
    import test_gpu_mpc_sqp as sqp
    sqp.test_one_round_equals_the_python_round(robot, T, 5, False)


def al_case(robot, B, seed):
    """One AL iterate as test_gpu_al_bounds.step_data draws it (controls N(0, 0.5^2) in a box of +-0.3: rows active at
    some knots and inactive at others), the C-ABI caller of that file on the vector entries, and the model's step and
    Jacobians as the oracle takes them.  B = 5: the kernels give a problem 16 lanes, four problems to a wavefront."""
    from test_gpu_al_bounds import Call, dev
    from diff_qp_mpc_amd.dynamics import DeviceDynamics
    dyn = DeviceDynamics(robot)
    n, m = dyn.n_state, dyn.n_ctrl
    rng = np.random.default_rng(seed)
    xu = 0.5 * rng.standard_normal((B, T, n + m))
    if robot == "pendulum_dx":          # (cos, sin, rate)
        xu[..., :2] /= np.linalg.norm(xu[..., :2], axis=-1, keepdims=True)
    d = dict(xu=xu, x0=xu[:, 0, :n] + 0.1 * rng.standard_normal((B, n)), Qd=rng.random((B, T, n + m)) + 0.1,
             q=rng.standard_normal((B, T, n + m)), lam=rng.standard_normal((B, T * n + 2 * T * m)),
             rho=10.0 ** rng.integers(0, 3, (B, 1)).astype(np.float64))
    lo, hi = np.full(m, -0.3), np.full(m, 0.3)
    c = Call(robot, T, B, d, lo, hi, None)

    def step_np(x, u):
        xn, (Jx, Ju) = c.dyn.jac(dev(x), dev(u))
        return xn.cpu().numpy(), Jx.cpu().numpy(), Ju.cpu().numpy()

    return d, lo, hi, c, step_np


@pytest.mark.parametrize("robot", ["pendulum1l", "pendulum_dx"])
def test_al_outer_update_vs_oracle(robot):
    """multipliers, cost and residual norm at test_gpu_al_bounds.py::test_varying_bounds_kernels_vs_oracle's tolerance"""
    from oracle import al_solve_oracle as aso
    B = 5
    d, lo, hi, c, step_np = al_case(robot, B, 3 * T + B)
    n, m = c.n, c.m
    out, names = c.outer_update()
    assert len(names) == 1 and "al_outer_kernel<" in names[0] and "StridedBounds" not in names[0], names
    res, resc = aso.residuals(d["xu"], d["x0"], lo, hi, step_np)
    iq = res[:, T * n:].reshape(B, T, 2 * m)
    assert (iq > 0).any() and (iq.max(2) <= 0).any(), iq            # active rows and knots without one
    lam_new = d["lam"] + d["rho"] * res
    lam_new[:, T * n:] = np.maximum(lam_new[:, T * n:], 0.0)
    np.testing.assert_allclose(out["lam_new"], lam_new, rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(out["cost"], aso.compute_cost(d["xu"], d["Qd"], d["q"]), rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(out["resn"], np.linalg.norm(resc, axis=1), rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("robot", ["pendulum1l", "pendulum_dx"])
def test_al_newton_solve_vs_oracle(robot):
    """dqp_al_newton_solve (four Newton steps, each with the 20-candidate line search, block-tridiagonal factor) against
    al_solve_oracle.newton_al: the iterate at the tolerance AL_mpc.MPC's x, u have against the oracle for states of this
    magnitude (test_gpu_al.py: rtol 1e-4 / atol 1e-5), the acceptance of the last step exactly."""
    from oracle import al_solve_oracle as aso
    B = 5
    d, lo, hi, c, step_np = al_case(robot, B, 7 * T + B)
    out, names = c.newton_solve()
    assert sum("al_banded_newton_kernel<" in k for k in names) == aso.NEWTON_STEPS, names
    x_est, _, status, chol_fail = aso.newton_al(d["xu"], d["x0"], d["lam"], d["rho"], d["Qd"], d["q"], lo, hi, step_np)
    assert not chol_fail and not out["fail"].any()
    print(robot, "max |gpu - oracle| = %.3e" % float(np.abs(out["xu"] - x_est).max()))
    np.testing.assert_allclose(out["xu"], x_est, rtol=1e-4, atol=1e-5)
    np.testing.assert_array_equal(out["status"] != 0.0, status)
