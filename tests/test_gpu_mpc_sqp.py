"""The SQP rounds of qp_wrapper.MPC for a registered device model as one enqueueing call (include/dqp.h:
dqp_mpc_linearize, dqp_mpc_sqp_rounds; csrc/dqp_mpc_sqp.hip; qp_wrapper.ONE_CALL_SQP) against the Python loop they
replace, the reference's config-2 golden, and their own contract: chunked calls, the stop rule, hipGraphs, launch count.

Tolerances are the project's for the same quantities: the linearisation against dyn.jac rtol / atol 1e-12 (the fused
rollout's figure), trajectories of the loop rtol 1e-5 / atol 1e-7, gradients rtol 1e-4 / atol 1e-6."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F64 = dict(dtype=torch.float64, device="cuda")


def load(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False))


def dev(a, grad=False):
    t = torch.tensor(np.asarray(a), **F64)
    return t.requires_grad_() if grad else t


@pytest.fixture
def flag_on(monkeypatch):
    from diff_qp_mpc_amd import qp_wrapper
    monkeypatch.setattr(qp_wrapper, "ONE_CALL_SQP", True)


@functools.lru_cache(maxsize=None)
def problem(robot, T, B):
    """x0, cost, bounds and starting controls of a small problem on a registered model (never modified by a test)"""
    from diff_qp_mpc_amd.dynamics import DeviceDynamics
    dyn = DeviceDynamics(robot)
    n, m = dyn.n_state, dyn.n_ctrl
    if robot == "rexquadrotor":
        rng = np.random.default_rng(0)
        x0 = dev(rng.uniform(-1, 1, (B, n)) * np.array([1.0] * 3 + [0.15] * 3 + [0.5] * 3 + [0.25] * 3))
        Qw = torch.tensor([10.0] * 3 + [0.01] * 3 + [1.0] * 3 + [0.01] * 3 + [1e-4] * m, **F64)
        hover = (2.0 * 9.81 + 4 * 30.48576) / (4 * 0.0244101 * 100.0)
        C = torch.diag(Qw).repeat(T, B, 1, 1)
        ref = torch.cat([torch.zeros(n, **F64), torch.full((m,), hover, **F64)])
        c = (-(Qw * ref)).repeat(T, B, 1)
        lo, hi = torch.full((m,), 11.5, **F64), torch.full((m,), 18.3, **F64)
        u0 = torch.full((T, B, m), hover, **F64)
    else:
        gen = torch.Generator().manual_seed(T)
        rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64).cuda()
        x0 = 0.3 * rnd(B, n)
        if robot == "pendulum_dx":
            x0[:, :2] = torch.nn.functional.normalize(x0[:, :2] + torch.tensor([1.0, 0.0]).cuda(), dim=1)
        L = 0.3 * rnd(T, B, n + m, n + m)
        C = L @ L.transpose(2, 3) + torch.eye(n + m, **F64)
        c = 0.2 * torch.ones(T, B, n + m, **F64)
        lo, hi = -torch.ones(m, **F64), torch.ones(m, **F64)
        u0 = torch.zeros(T, B, m, **F64)
    return dict(dyn=dyn, n=n, m=m, T=T, B=B, x0=x0, C=C.contiguous(), c=c.contiguous(), lo=lo, hi=hi, u0=u0)


def make_mpc(p, lo=None, hi=None, **kw):
    from diff_qp_mpc_amd import qp_wrapper
    mpc = qp_wrapper.MPC(p["n"], p["m"], p["T"], u_lower=p["lo"] if lo is None else lo, u_upper=p["hi"] if hi is None else hi,
                         n_batch=p["B"], verbose=-1, **kw)
    mpc.dx_true = p["dyn"]
    return mpc


class Rounds:
    """dqp_mpc_sqp_rounds on buffers of its own, started at u0 and its rollout, with the options of `mpc`"""
    NAMES = ("x", "u", "keep_x", "keep_u", "keep_cost", "state")

    def __init__(self, p, mpc):
        from diff_qp_mpc_amd import _lib, qp_wrapper
        from diff_qp_mpc_amd.al_utils import mpc_bounds_layout
        self.p, self.mpc = p, mpc
        B, T, n, m = p["B"], p["T"], p["n"], p["m"]
        with torch.no_grad():
            self.x = mpc.rollout(p["x0"], p["u0"], p["dyn"]).clone()
        self.u = p["u0"].clone()
        self.start = (self.x.clone(), self.u.clone())
        self.keep_x, self.keep_u = torch.full((T, B, n), 7.0, **F64), torch.full((T, B, m), 7.0, **F64)
        self.keep_cost = torch.full((B,), -1e300, **F64)        # round 0 must not compare with it
        self.state = torch.full((4,), 5, dtype=torch.int32, device="cuda")      # round 0 must clear it
        self.dims = _lib.dqp_mpc_dims(B, n, m, T, 1, p["dyn"].id)
        self.opts = qp_wrapper._mpc_qp_opts(p["dyn"].dt)
        nbytes = int(_lib.load().dqp_mpc_sqp_workspace_bytes(ctypes.byref(self.dims), ctypes.byref(self.opts)))
        assert nbytes > 0
        self.ws = torch.empty(nbytes // 8, **F64)
        self.bounds = mpc_bounds_layout(*mpc._bounds(torch.device("cuda")), B, T, m)

    def run(self, begin, end):
        from diff_qp_mpc_amd import _lib
        p, mpc = self.p, self.mpc
        _lib.call("dqp_mpc_sqp_rounds", torch.device("cuda"), self.dims, self.opts, p["C"], p["c"], p["x0"], self.bounds.ref(),
                  float(mpc.linesearch_decay), int(mpc.max_linesearch_iter), float(mpc.best_cost_eps), float(mpc.eps),
                  begin, end, self.x, self.u, self.keep_x, self.keep_u, self.keep_cost, self.state, self.ws)
        return self

    def snapshot(self):
        return {k: getattr(self, k).clone() for k in self.NAMES}


def assert_same_bits(a, b):
    for k in Rounds.NAMES:
        assert torch.equal(a[k], b[k]), k


# ---------------------------------------------------------------------------------------------- 1. linearisation
@pytest.mark.parametrize("robot", ["pendulum_dx", "cartpole1l", "cartpole2l", "integrator", "rexquadrotor"])
def test_linearize_equals_the_models_jacobians(robot):
    from diff_qp_mpc_amd import _lib
    from diff_qp_mpc_amd.qp_wrapper import bmv
    T, B = 4, 5
    p = problem(robot, T, B)
    dyn, n, m = p["dyn"], p["n"], p["m"]
    gen = torch.Generator().manual_seed(11)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64).cuda()
    x = (p["x0"][None] + 0.2 * rnd(T, B, n)).contiguous()
    u = (p["u0"] + 0.3 * rnd(T, B, m)).contiguous()
    F = torch.full((T - 1, B, n, n + m), float("nan"), **F64)
    f = torch.full((T - 1, B, n), float("nan"), **F64)
    dims = _lib.dqp_mpc_dims(B, n, m, T, 1, dyn.id)
    _lib.call("dqp_mpc_linearize", torch.device("cuda"), dims, dyn.dt, x, u, F, f)
    xs, us = x[:-1].reshape(-1, n), u[:-1].reshape(-1, m)
    nxt, (Jx, Ju) = dyn.jac(xs, us)
    F_ref = torch.cat((Jx, Ju), dim=2)
    f_ref = nxt - bmv(F_ref, torch.cat((xs, us), dim=1))
    np.testing.assert_allclose(F.reshape(-1, n, n + m).cpu().numpy(), F_ref.cpu().numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(f.reshape(-1, n).cpu().numpy(), f_ref.cpu().numpy(), rtol=1e-12, atol=1e-12)


# ---------------------------------------------------------------------------------------------- 2. one round
def python_round(p, mpc, x, u):
    """one round of solve_nonlin's loop: (x_new, u_new, cost_new)"""
    from diff_qp_mpc_amd import qp_wrapper
    cost = qp_wrapper.QuadCost(p["C"], p["c"])
    with torch.no_grad():
        sx, su, _ = mpc.single_qp(x, u, p["dyn"], p["dyn"].jac, p["x0"], cost, need_cost=False)
        xn, un, _, cn = mpc.line_search(x, u, sx, su, p["dyn"], p["x0"], cost)
    return xn, un, cn


@pytest.mark.parametrize("robot,T,B,per_sample", [
    ("pendulum_dx", 10, 6, False), ("cartpole1l", 5, 5, False), ("cartpole1l", 12, 5, False), ("cartpole1l", 12, 5, True),
    ("cartpole2l", 4, 3, False), ("rexquadrotor", 6, 3, False)])
def test_one_round_equals_the_python_round(robot, T, B, per_sample):
    p = problem(robot, T, B)
    lo = hi = None
    if per_sample:      # (1, B, m): every sample its own limit, some of them active
        hi = (0.05 + 0.3 * torch.arange(B, **F64)).reshape(1, B, 1).repeat(1, 1, p["m"]).contiguous()
        lo = -hi
    mpc = make_mpc(p, lo, hi)
    r = Rounds(p, mpc)
    xn, un, cn = python_round(p, mpc, *r.start)
    r.run(0, 1)
    assert r.state.tolist() == [0, 1, 0, 0]
    tol = dict(rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(r.x.cpu().numpy(), xn.cpu().numpy(), **tol)
    np.testing.assert_allclose(r.u.cpu().numpy(), un.cpu().numpy(), **tol)
    np.testing.assert_allclose(r.keep_cost.cpu().numpy(), cn.cpu().numpy(), **tol)
    assert torch.equal(r.keep_x, r.x) and torch.equal(r.keep_u, r.u)       # round 0 stores unconditionally
    if per_sample:
        assert float((r.u.abs() - hi).max()) <= 1e-9 and float(r.u.abs().max()) > 0.05 + 1e-6


# ---------------------------------------------------------------------------------------------- 3. chunking
@pytest.mark.parametrize("robot,T,B", [("pendulum_dx", 10, 6), ("cartpole1l", 12, 70)])
def test_one_call_of_three_rounds_equals_three_calls(robot, T, B):
    p = problem(robot, T, B)
    mpc = make_mpc(p)
    one = Rounds(p, mpc).run(0, 3).snapshot()
    r = Rounds(p, mpc)
    for k in range(3):
        r.run(k, k + 1)
    assert_same_bits(one, r.snapshot())
    assert one["state"].tolist()[1:] == [3, 0, 0]          # every round ran (the third may be the one that stops)
    assert Rounds(p, mpc).run(0, 0).state.tolist() == [0, 0, 0, 0]         # an empty range from 0 still resets


# ---------------------------------------------------------------------------------------------- 4. the reference
def _cfg2_problem(B, T):
    from diff_qp_mpc_amd.dynamics import DeviceDynamics
    g = load("CFG2_pendulumdx_T10_b6")
    dx = DeviceDynamics("pendulum_dx", dt=float(g["dt"]))
    C = torch.diag(dev(g["q"]))[None, None].repeat(T, B, 1, 1).requires_grad_()
    c = dev(g["p"])[None, None].repeat(T, B, 1).requires_grad_()
    lo = torch.tensor([float(g["u_lower"])], **F64)
    hi = torch.tensor([float(g["u_upper"])], **F64)
    return g, dx, C, c, lo, hi


def _check_cfg2_gradients(ctrl, C, c, g, tag):
    """d(x, u)/d(C, c) of the differentiable last step is proportional to the line search's factor alpha, and at a
    converged iterate the accept test compares two costs equal up to round-off, so a sample may come out with another
    power of the decay than the reference's: every sample is compared after scaling by alpha_ref / alpha."""
    alpha = ctrl.last_alpha.reshape(-1).cpu().numpy()
    a_ref = g[tag + "_alpha"]
    k = np.log(alpha / a_ref) / np.log(0.2)
    assert np.allclose(k, np.round(k), atol=1e-9), alpha          # a power of the decay
    scale = (a_ref / alpha)[None, :, None]
    np.testing.assert_allclose(C.grad.cpu().numpy() * scale[..., None], g[tag + "_dC"], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(c.grad.cpu().numpy() * scale, g[tag + "_dc"], rtol=1e-4, atol=1e-6)


def count_calls(monkeypatch, name):
    from diff_qp_mpc_amd import _lib
    seen, real = [], _lib.call

    def call(entry, *a):
        if entry == name:
            seen.append(a)
        return real(entry, *a)
    monkeypatch.setattr(_lib, "call", call)
    return seen


def test_config2_pendulumdx_vs_reference_on_the_device_rounds(flag_on, monkeypatch):
    from diff_qp_mpc_amd import qp_wrapper
    seen = count_calls(monkeypatch, "dqp_mpc_sqp_rounds")
    g0 = load("CFG2_pendulumdx_T10_b6")
    B, T = g0["x0"].shape[0], 10
    g, dx, C, c, lo, hi = _cfg2_problem(B, T)
    ctrl = qp_wrapper.MPC(3, 1, T, u_lower=lo, u_upper=hi, n_batch=B, max_linesearch_iter=5, linesearch_decay=0.2, qp_iter=3)
    x, u = ctrl(dev(g["x0"]), qp_wrapper.QuadCost(C, c), dx, dx.jac)
    assert 1 <= len(seen) <= 3
    np.testing.assert_allclose(x.detach().cpu().numpy(), g["sqp3_x"], rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(u.detach().cpu().numpy(), g["sqp3_u"], rtol=1e-5, atol=1e-7)
    (x.sum() + 2.0 * u.sum()).backward()
    _check_cfg2_gradients(ctrl, C, c, g, "sqp3")


# ---------------------------------------------------------------------------------------------- 5. the existing loop
def test_forward_equals_the_python_loop(monkeypatch):
    from diff_qp_mpc_amd import qp_wrapper
    p = problem("cartpole1l", 12, 5)
    cost = qp_wrapper.QuadCost(p["C"], p["c"])
    outs = {}
    for on in (False, True):
        monkeypatch.setattr(qp_wrapper, "ONE_CALL_SQP", on)
        mpc = make_mpc(p, qp_iter=3)
        assert mpc._sqp_on_device(p["dyn"], p["dyn"].jac, cost, p["x0"]) is on
        with torch.no_grad():
            outs[on] = mpc(p["x0"], cost, p["dyn"], p["dyn"].jac)
    for a, b, k in zip(outs[True], outs[False], "xu"):
        np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=1e-5, atol=1e-7, err_msg=k)


# ---------------------------------------------------------------------------------------------- 6. the stop rule
def test_stop_rule_freezes_the_later_rounds(monkeypatch):
    """Linear dynamics: the second QP already repeats the first one's solution, so the loop stops early.  The device
    rounds stop at the round the Python loop stops at, rounds behind the stop change nothing, and solve_nonlin enqueues
    exactly the rounds that ran."""
    from diff_qp_mpc_amd import qp_wrapper
    p = problem("integrator", 5, 4)
    cost = qp_wrapper.QuadCost(p["C"], p["c"])
    kw = dict(qp_iter=6, eps=1e-3)
    eager = make_mpc(p, **kw)
    solves, real = [], eager.single_qp
    eager.single_qp = lambda *a, **k: (solves.append(1), real(*a, **k))[1]
    with torch.no_grad():
        xe, ue = eager(p["x0"], cost, p["dyn"], p["dyn"].jac)
    k = len(solves) - 1                     # the last one is the differentiable step's
    assert 1 <= k < 6
    r = Rounds(p, make_mpc(p, **kw)).run(0, 6)
    assert r.state.tolist() == [1, k, 0, 0]
    before = r.snapshot()
    r.run(k, 6)
    assert_same_bits(before, r.snapshot())
    monkeypatch.setattr(qp_wrapper, "ONE_CALL_SQP", True)
    seen = count_calls(monkeypatch, "dqp_mpc_sqp_rounds")
    with torch.no_grad():
        x, u = make_mpc(p, **kw)(p["x0"], cost, p["dyn"], p["dyn"].jac)
    assert len(seen) == k
    np.testing.assert_allclose(x.cpu().numpy(), xe.cpu().numpy(), rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(u.cpu().numpy(), ue.cpu().numpy(), rtol=1e-5, atol=1e-7)


# ---------------------------------------------------------------------------------------------- 7. hipGraphs
def test_device_rounds_captured_in_hipgraphs(flag_on, monkeypatch):
    """graphed_mpc with the flag on: every round enqueued by one call inside the forward graph, replayed bitwise equal
    to the eager flag-on call (which reads the stop flag after every round) on the capture inputs and on new ones."""
    from diff_qp_mpc_amd import qp_wrapper
    from diff_qp_mpc_amd.dynamics import DeviceDynamics
    seen = count_calls(monkeypatch, "dqp_mpc_sqp_rounds")
    B, T, n, m = 64, 10, 3, 1
    dyn = DeviceDynamics("pendulum_dx")
    factory = lambda: (dyn, dyn.jac)
    C = (torch.eye(n + m, dtype=torch.float64).repeat(T, B, 1, 1).cuda() * 0.5).requires_grad_()

    def inputs(seed):
        g2 = torch.Generator().manual_seed(seed)
        x0 = torch.randn(B, n, generator=g2, dtype=torch.float64).cuda()
        x0[:, :2] = torch.nn.functional.normalize(x0[:, :2], dim=1)
        c = torch.randn(T, B, n + m, generator=g2, dtype=torch.float64).cuda()
        return x0.requires_grad_(), c.requires_grad_()

    one = torch.full((m,), 2.0, **F64)
    make = lambda: qp_wrapper.MPC(n, m, T, u_lower=-one, u_upper=one, n_batch=B, verbose=-1, qp_iter=3,
                                  max_linesearch_iter=5, eps=1e-3)
    mpc, mpc_eager = make(), make()
    x0a, ca = inputs(2)
    g = qp_wrapper.graphed_mpc(mpc, (x0a, C, ca), factory)
    assert seen and all(a[-9:-7] == (0, 3) for a in seen)         # captured: one call for all three rounds
    for seed in (2, 3):
        x0, c = inputs(seed)
        del seen[:]
        xe, ue = mpc_eager(x0, qp_wrapper.QuadCost(C, c), dyn, dyn.jac)
        assert 1 <= len(seen) <= 3
        ge = torch.autograd.grad((xe * 1.5).sum() + ue.sum(), (x0, c))
        xg, ug = g(x0, C, c)
        gg = torch.autograd.grad((xg * 1.5).sum() + ug.sum(), (x0, c))
        assert torch.equal(xg, xe) and torch.equal(ug, ue)
        for a, b in zip(gg, ge):
            assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------- 8. launches
def test_launches_of_a_three_round_call():
    from diff_qp_mpc_amd import _lib
    p = problem("cartpole1l", 12, 5)
    mpc = make_mpc(p)
    r = Rounds(p, mpc)
    # what the QP and the line search launch on their own at this shape: a Python round without the two dqp_dyn_*
    # launches of its linearisation
    with _lib.trace() as own:
        python_round(p, mpc, *r.start)
    own = [k for k, _ in own.records if "jac_kernel" not in k and "step_kernel" not in k]
    assert sum("line_search_kernel" in k for k in own) == 1 and len(own) >= 2
    with _lib.trace() as t:
        r.run(0, 3)
    names = [k for k, _ in t.records]
    assert sum("sqp_linearize_kernel" in k for k in names) == 3
    assert sum("line_search_kernel" in k for k in names) == 3
    new = [k for k in names if "sqp::" in k]
    assert len(new) <= 12 and len(names) - 3 * len(own) <= 12
    for kernel in ("sqp_linearize_kernel", "sqp_step_kernel", "sqp_keep_kernel", "sqp_finish_kernel"):
        assert sum(kernel in k for k in new) == 3, kernel
