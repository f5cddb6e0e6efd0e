"""The block-tridiagonal NewtonAL kernels for caller-linearised dynamics (csrc/dqp_al_banded.hip: Given<n, m>, reached
through dqp_al_banded_newton_step_jac and dqp_al_banded_solve(dims, 0, ...)) at every compiled (n_state, n_ctrl) pair.

Each pair compiles into the 16-lane kernels; pairs with nt = n + m <= 8 also into the half-row (8-lane) kernels, and
those with 6 <= nt <= 8 into an 8-lane Newton kernel that keeps the factor in LDS (LF) for short horizons.  The pairs
are parsed out of DQP_BAND_SIZES (test_al_banded_cpu.band_sizes), so a pair added to the kernel is tested here too.

  * kernel vs the dense numpy oracle (oracle/al_oracle.py, pinned to the reference by AL_*.npz): update and factor
    solve rtol 1e-8 / atol 1e-10, with the launched instantiation checked through the library's trace;
  * non-positive pivots reported per problem and per knot (include/dqp.h: info = 1 + the knot of the first one),
    neighbours in the same DPP row unaffected;
  * position independence: the batch rolled by one gives bit-identical results;
  * registered device models against the same linearisation fed in by the caller;
  * AL_mpc.MPC end to end with a caller's nonlinear module against oracle/al_solve_oracle.py.
"""
import contextlib
import ctypes
import re

import numpy as np
import pytest
import torch

from oracle import al_oracle
from oracle import al_solve_oracle as aso
from test_al_banded_cpu import band_sizes

pytestmark = pytest.mark.gpu
PAIRS = band_sizes()
UT = dict(rtol=1e-8, atol=1e-10)            # as test_gpu_al.py::test_banded_newton_step_vs_dense_oracle
LF_LDS_BYTES = 34 * 1024                    # run_newton: the factor stays in LDS up to this many bytes per workgroup
NEWTON_RE = re.compile(r"al_banded_newton_kernel<[^<>]*Given<(\d+), (\d+)>, (\d+), (true|false)>")
SOLVE_RE = re.compile(r"al_banded_solve_kernel<[^<>]*Given<(\d+), (\d+)>, (\d+)>")


@pytest.fixture(autouse=True)
def _auto_lane_group():
    yield
    from diff_qp_mpc_amd import _lib
    _lib.load().dqp_al_lane_group(0)


def _pin_lane_group(group):
    from diff_qp_mpc_amd import _lib
    assert _lib.load().dqp_al_lane_group(int(group)) == 0


def groups(n, m):
    """lane groups a pair is compiled for: one problem per 16-lane DPP row, or per half row where a knot fits"""
    return (16, 8) if n + m <= 8 else (16,)


def lds_factor(n, m, T, group):
    """the dispatch's LF rule: 8-lane group, 6 <= nt <= 8, T (ROW + 1) 8 nt doubles of LDS at most 34 KiB"""
    nt = n + m
    row = nt + 1 + n
    return group == 8 and 6 <= nt <= 8 and T * (row + 1) * 8 * nt * 8 <= LF_LDS_BYTES


def given_launches(tr):
    """-> ({(n, m, group, lf)} of the Newton kernels, {(n, m, group)} of the solve kernels) in a trace"""
    newton, solve = set(), set()
    for k, _ in tr.records:
        a = NEWTON_RE.search(k)
        if a:
            newton.add((int(a.group(1)), int(a.group(2)), int(a.group(3)), a.group(4) == "true"))
        a = SOLVE_RE.search(k)
        if a:
            solve.add((int(a.group(1)), int(a.group(2)), int(a.group(3))))
    return newton, solve


def dev(a, grad=False):
    t = torch.tensor(np.asarray(a), dtype=torch.float64, device="cuda")
    return t.requires_grad_() if grad else t


def problem(n, m, T, B=37, seed=0):
    """One Newton step's data with a caller's linearisation: x_next, Jx = I + 0.1 randn, Ju, shaped (B, T - 1, ...);
    controls around the box [-0.3, 0.3], so that some box rows are active and some not."""
    rng = np.random.default_rng(seed)
    nt = n + m
    p = dict(xu=0.5 * rng.standard_normal((B, T, nt)), Qd=rng.random((B, T, nt)) + 0.1, q=rng.standard_normal((B, T, nt)),
             lam=rng.standard_normal((B, T * n + 2 * T * m)), rho=rng.choice([1.0, 10.0, 100.0], size=(B, 1)),
             xn=rng.standard_normal((B, T - 1, n)), Jx=np.eye(n) + 0.1 * rng.standard_normal((B, T - 1, n, n)),
             Ju=rng.standard_normal((B, T - 1, n, m)), rhs=rng.standard_normal((B, T, nt)))
    p["x0"] = p["xu"][:, 0, :n] + 0.1 * rng.standard_normal((B, n))
    p["lo"], p["hi"] = np.full(m, -0.3), np.full(m, 0.3)
    return p


def oracle_step(p):
    """al_oracle.newton_update on the dense formulation of the same linearisation -> (update, L, info) (B, T nt)"""
    B, T, nt = p["xu"].shape
    n = p["x0"].shape[1]
    m = nt - n

    def step(x, u):         # the caller's linearisation, in constraint_jacobian's b-major row order
        return (p["xn"].reshape(B * (T - 1), n), p["Jx"].reshape(B * (T - 1), n, n), p["Ju"].reshape(B * (T - 1), n, m))

    res, resc, J, Jc = al_oracle.constraint_jacobian(p["xu"], p["x0"], p["lo"], p["hi"], step=step)
    iq = res[:, T * n:]
    assert (iq > 0).any() and (iq <= 0).any()            # some box rows active, some inactive
    grad = al_oracle.merit_grad(p["xu"], p["Qd"], p["q"], p["lam"], p["rho"], resc, J, Jc)
    return al_oracle.newton_update(Jc, p["Qd"].reshape(B, -1), p["rho"], grad)


def run_given(p, group, trace=False):
    """dqp_al_banded_newton_step_jac then dqp_al_banded_solve(dims, 0, factor, rhs) -> numpy (update, info, solve, trace)"""
    from diff_qp_mpc_amd import _lib
    lib = _lib.load()
    _pin_lane_group(group)
    B, T, nt = p["xu"].shape
    n = p["x0"].shape[1]
    t = {k: dev(v).contiguous() for k, v in p.items()}
    dims = _lib.dqp_al_mpc_dims(B, n, nt - n, T)
    nbytes = int(lib.dqp_al_banded_factor_bytes(ctypes.byref(dims), 0))
    assert nbytes == B * T * nt * (nt + 1 + n) * 8
    fac = torch.empty(nbytes // 8, dtype=torch.float64, device="cuda")
    upd = torch.full((B, T, nt), np.nan, dtype=torch.float64, device="cuda")
    out = torch.full((B, T, nt), np.nan, dtype=torch.float64, device="cuda")
    info = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    P = lambda x: ctypes.c_void_p(x.data_ptr())
    with _lib.trace(16) if trace else contextlib.nullcontext() as tr:
        rc = lib.dqp_al_banded_newton_step_jac(ctypes.byref(dims), P(t["xu"]), P(t["x0"]), P(t["Qd"]), P(t["q"]),
                                               P(t["lam"]), P(t["rho"].reshape(B).contiguous()), P(t["lo"]), P(t["hi"]),
                                               P(t["xn"]), P(t["Jx"]), P(t["Ju"]), P(upd), P(fac), P(info), None)
        assert rc == 0
        assert lib.dqp_al_banded_solve(ctypes.byref(dims), 0, P(fac), P(t["rhs"]), P(out), None) == 0
        torch.cuda.synchronize()
    return upd.cpu().numpy(), info.cpu().numpy(), out.cpu().numpy(), tr


CASES = [(n, m, g, T) for n, m in PAIRS for g in groups(n, m) for T in (2, 4, 11)]


def test_cases_cover_every_instantiation():
    """46 Newton and 38 solve instantiations exist for the 24 pairs; the kernel-vs-oracle cases below pick each one."""
    newton = {(n, m, g, lds_factor(n, m, T, g)) for n, m, g, T in CASES}
    solve = {(n, m, g) for n, m, g, _ in CASES}
    small = [(n, m) for n, m in PAIRS if n + m <= 8]
    lf = [(n, m) for n, m in small if n + m >= 6]
    assert (len(PAIRS), len(small), len(lf)) == (24, 14, 8)
    assert len(newton) == len(PAIRS) + len(small) + len(lf) == 46
    assert len(solve) == len(PAIRS) + len(small) == 38
    for n, m in lf:                 # T = 4 keeps the factor in LDS, T = 11 does not: both paths at every LF pair
        assert lds_factor(n, m, 4, 8) and not lds_factor(n, m, 11, 8), (n, m)


@pytest.mark.parametrize("n,m,group,T", CASES)
def test_given_newton_step_vs_dense_oracle(n, m, group, T):
    """B = 37: the last wavefront is ragged in both group widths.  The trace names the launched kernels: Given<n, m>
    in the pinned group, with the LDS factor exactly where the dispatch's byte rule says."""
    p = problem(n, m, T, seed=1000 * n + 10 * m + T)
    upd_ref, L_ref, info_ref = oracle_step(p)
    assert not info_ref.any()
    upd, info, out, tr = run_given(p, group, trace=True)
    newton, solve = given_launches(tr)
    assert newton == {(n, m, group, lds_factor(n, m, T, group))}, tr.records
    assert solve == {(n, m, group)}, tr.records
    assert (info == 0).all(), info
    B = p["xu"].shape[0]
    np.testing.assert_allclose(upd.reshape(B, -1), upd_ref, **UT)
    np.testing.assert_allclose(out.reshape(B, -1), al_oracle.chol_solve_neg(L_ref, p["rhs"].reshape(B, -1)), **UT)


PIVOT_CASES = [(n, m, g, T) for n, m in [(1, 1), (5, 2), (6, 2), (8, 2), (9, 3), (12, 4)] for g in groups(n, m)
               for T in (4, 11)]


@pytest.mark.parametrize("n,m,group,T", PIVOT_CASES)
def test_given_pivot_failure_is_per_problem_and_knot(n, m, group, T):
    """Two problems get a control cost of -1e3 at knot t0 = T // 2 (rho 1, so that no penalty term can outweigh it):
    one at an even and one at an odd batch index, i.e. on both halves of a DPP row in the 8-lane kernels.  Their info
    is 1 + t0, as the oracle's cholesky_ex info says; every other problem, its row neighbours included, keeps info 0
    and the oracle's update and factor solve."""
    p = problem(n, m, T, seed=77 + 1000 * n + 10 * m + T)
    B, nt, t0 = p["xu"].shape[0], n + m, T // 2
    bad = [10, 35]
    for b in bad:
        p["Qd"][b, t0, n:] = -1e3
        p["rho"][b] = 1.0
    upd_ref, L_ref, info_ref = oracle_step(p)
    good = np.setdiff1d(np.arange(B), bad)
    assert (info_ref[bad] > 0).all() and not info_ref[good].any()
    np.testing.assert_array_equal(1 + (info_ref[bad] - 1) // nt, 1 + t0)
    upd, info, out, _ = run_given(p, group)
    np.testing.assert_array_equal(info[bad], 1 + t0)
    np.testing.assert_array_equal(info[good], 0)
    np.testing.assert_allclose(upd.reshape(B, -1)[good], upd_ref[good], **UT)
    np.testing.assert_allclose(out.reshape(B, -1)[good],
                               al_oracle.chol_solve_neg(L_ref[good], p["rhs"].reshape(B, -1)[good]), **UT)


@pytest.mark.parametrize("n,m,group,T", [(n, m, g, T) for n, m in PAIRS for g in groups(n, m) for T in (4, 11)])
def test_given_results_do_not_depend_on_batch_position(n, m, group, T):
    """The batch rolled by one moves every problem to the other half of its DPP row and to another wavefront slot:
    after un-rolling, update, info and factor solve are bit for bit those of the unrolled batch.  This catches
    leakage between neighbouring problems too small for a tolerance."""
    p = problem(n, m, T, seed=5 + 1000 * n + 10 * m + T)
    rolled = {k: (v if k in ("lo", "hi") else np.roll(v, 1, axis=0)) for k, v in p.items()}
    upd, info, out, _ = run_given(p, group)
    upd_r, info_r, out_r, _ = run_given(rolled, group)
    assert (info == 0).all()
    np.testing.assert_array_equal(np.roll(info_r, -1, axis=0), info)
    np.testing.assert_array_equal(np.roll(upd_r, -1, axis=0), upd)
    np.testing.assert_array_equal(np.roll(out_r, -1, axis=0), out)


# (n_state, n_ctrl) of the registered models (checked against dqp_dyn_sizes in the test): all of them compiled pairs
REGISTERED = {"pendulum1l": (2, 1), "cartpole1l": (4, 1), "cartpole2l": (6, 1), "pendulum_euler": (2, 1),
              "pendulum_dx": (3, 1), "rexquadrotor": (12, 4)}


def _registered_cases():
    from diff_qp_mpc_amd.dynamics import NAMES
    return [(name, g, T) for name in NAMES for g in groups(*REGISTERED[name]) for T in (4, 11)]


@pytest.mark.parametrize("name,group,T", _registered_cases())
def test_registered_model_equals_given_linearisation(name, group, T):
    """dqp_al_banded_newton_step(dyn.id) evaluates the model with forward-mode seeds inside the kernel; the same model's
    DeviceDynamics.jac on the same trajectory, passed to dqp_al_banded_newton_step_jac, is the same linearisation
    (both are the dqp_dyn_models.h templates in fp64), so update and factor solve agree to rtol 1e-10 / atol 1e-12:
    only the compiler's contraction of the model arithmetic may differ between the two kernels."""
    from diff_qp_mpc_amd import _lib
    from diff_qp_mpc_amd.dynamics import DeviceDynamics
    lib = _lib.load()
    dyn = DeviceDynamics(name)
    n, m, nt = dyn.n_state, dyn.n_ctrl, dyn.n_state + dyn.n_ctrl
    assert (n, m) == REGISTERED[name] and (n, m) in PAIRS
    p = problem(n, m, T, seed=31 + T)
    B = p["xu"].shape[0]
    if name == "rexquadrotor":
        p["xu"][..., n:] = 14.5 + 0.3 * np.random.default_rng(T).standard_normal((B, T, m))    # around hover
        p["lo"], p["hi"] = np.full(m, 14.2), np.full(m, 14.8)
    if name == "pendulum_dx":
        p["xu"][..., :2] /= np.linalg.norm(p["xu"][..., :2], axis=-1, keepdims=True)
    xu = dev(p["xu"])
    xn, (Jx, Ju) = dyn.jac(xu[:, :-1, :n].reshape(-1, n).contiguous(), xu[:, :-1, n:].reshape(-1, m).contiguous())
    p["xn"], p["Jx"], p["Ju"] = (a.reshape((B, T - 1) + a.shape[1:]).cpu().numpy() for a in (xn, Jx, Ju))
    upd_g, info_g, out_g, _ = run_given(p, group)

    _pin_lane_group(group)
    t = {k: dev(v).contiguous() for k, v in p.items()}
    dims = _lib.dqp_al_mpc_dims(B, n, m, T)
    fac = torch.empty(int(lib.dqp_al_banded_factor_bytes(ctypes.byref(dims), dyn.id)) // 8, dtype=torch.float64, device="cuda")
    upd = torch.empty(B, T, nt, dtype=torch.float64, device="cuda")
    out = torch.empty_like(upd)
    info = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    P = lambda x: ctypes.c_void_p(x.data_ptr())
    rc = lib.dqp_al_banded_newton_step(ctypes.byref(dims), dyn.id, dyn.dt, P(t["xu"]), P(t["x0"]), P(t["Qd"]), P(t["q"]),
                                       P(t["lam"]), P(t["rho"].reshape(B).contiguous()), P(t["lo"]), P(t["hi"]), P(upd),
                                       P(fac), P(info), None)
    assert rc == 0
    assert lib.dqp_al_banded_solve(ctypes.byref(dims), dyn.id, P(fac), P(t["rhs"]), P(out), None) == 0
    torch.cuda.synchronize()
    assert (info.cpu().numpy() == 0).all() and (info_g == 0).all()
    np.testing.assert_allclose(upd_g, upd.cpu().numpy(), rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(out_g, out.cpu().numpy(), rtol=1e-10, atol=1e-12)


class CallerToy(torch.nn.Module):
    """x+ = x + dt (A x + 0.3 sin(x) + B u) with analytic Jacobians (test_gpu_ric_wide.WideToy's map): a caller's module
    that is no registered model, so AL_mpc.MPC sends its own linearisation to the Given<n, m> kernels."""

    def __init__(self, n, m, dt=0.05):
        super().__init__()
        g = torch.Generator().manual_seed(100 * n + m)
        self.dt = dt
        self.A = 0.3 * torch.randn(n, n, generator=g, dtype=torch.float64)
        self.Bm = torch.randn(n, m, generator=g, dtype=torch.float64)

    def forward(self, x, u):
        A, Bm = self.A.to(x), self.Bm.to(x)
        return x + self.dt * (x @ A.T + 0.3 * torch.sin(x) + u @ Bm.T)

    def jac(self, x, u):
        A, Bm = self.A.to(x), self.Bm.to(x)
        eye = torch.eye(x.shape[1], dtype=x.dtype, device=x.device)
        R = eye + self.dt * (A + 0.3 * torch.diag_embed(torch.cos(x)))
        S = (self.dt * Bm).expand(x.shape[0], -1, -1)
        return self.forward(x, u), (R, S)

    def step_np(self, x, u):
        A, Bm = self.A.numpy(), self.Bm.numpy()
        xn = x + self.dt * (x @ A.T + 0.3 * np.sin(x) + u @ Bm.T)
        R = np.eye(x.shape[1]) + self.dt * (A + 0.3 * np.cos(x)[:, :, None] * np.eye(x.shape[1]))
        return xn, R, np.broadcast_to(self.dt * Bm, (x.shape[0],) + Bm.shape).copy()


MPC_CASES = [(n, m, 6, 5, g) for n, m in [(1, 1), (3, 3), (6, 2), (7, 1), (9, 3), (10, 4), (12, 2)] for g in groups(n, m)]
MPC_CASES += [(9, 3, 12, 5, 16), (7, 2, 6, 5, 16)]


@pytest.mark.parametrize("n,m,T,B,group", MPC_CASES)
def test_al_mpc_caller_module_vs_al_solve_oracle(n, m, T, B, group):
    """AL_mpc.MPC with CallerToy against oracle/al_solve_oracle.py on the same map in numpy: a cold call and the
    warm-started second call (history), x, u (float32 in AL_mpc.MPC) rtol 1e-4 / atol 1e-5, multipliers rtol 1e-5,
    rho exact, dC and dc of both calls rtol 1e-4 / atol 1e-6 -- the tolerances of
    test_gpu_al.py::test_al_mpc_two_calls_vs_reference.  The forward runs Given<n, m> and the backward its solve;
    (7, 2) has no instantiation, runs no Given kernel and must agree all the same."""
    from diff_qp_mpc_amd import AL_mpc, _lib, al_utils
    from diff_qp_mpc_amd.dynamics import recognise
    _pin_lane_group(group)
    nt = n + m
    rng = np.random.default_rng(10 * n + m + T)
    mod = CallerToy(n, m)
    x0 = rng.standard_normal((B, n))
    u_init = 0.2 * rng.standard_normal((B, T, m))
    x_init = np.empty((B, T, n))
    x_init[:, 0] = x0
    for t in range(T - 1):
        x_init[:, t + 1] = mod.step_np(x_init[:, t], u_init[:, t])[0]
    Qd = rng.random((B, T, nt)) + 0.1
    c = rng.standard_normal((B, T, nt))
    lo, hi = np.full(m, -0.5), np.full(m, 0.5)
    assert recognise(mod, n, m) is None

    ctrl = AL_mpc.MPC(n, m, T, u_lower=dev(lo), u_upper=dev(hi), n_batch=B, verbose=0, solver_type="dense",
                      dtype=torch.float64, eps=1e-5, exit_unconverged=False, backprop=False)
    ctrl.reinitialize(dev(x0), torch.ones(B, T, 1, device="cuda"))
    ctrl.x_init, ctrl.u_init = dev(x_init), dev(u_init)
    gxu = np.concatenate((np.ones((B, T, n)), 2.0 * np.ones((B, T, m))), 2)
    lam, rho, history = np.zeros((B, T * n + 2 * T * m)), np.ones((B, 1)), None
    xs, us = x_init, u_init
    listed = (n, m) in PAIRS
    for call in range(2):
        C = torch.diag_embed(dev(Qd)).requires_grad_()
        cc = dev(c, grad=True)
        with _lib.trace(4096) as tr:
            x, u = ctrl(dev(x0), al_utils.QuadCost(C, cc), mod, mod.jac)
            (x.double().sum() + 2.0 * u.double().sum()).backward()
            torch.cuda.synchronize()
        newton, solve = given_launches(tr)
        if listed:
            assert newton and {k[:3] for k in newton} == {(n, m, group)}, tr.records
            assert solve == {(n, m, group)}, tr.records
        else:
            assert not any("Given<" in k for k, _ in tr.records), tr.records
        o = aso.al_solve(xs, us, x0, Qd, c, lo, hi, mod.step_np, lam, rho, history=history)
        assert not o["chol_fail"]
        np.testing.assert_allclose(x.detach().cpu().numpy(), o["x"], rtol=1e-4, atol=1e-5, err_msg="x%d" % call)
        np.testing.assert_allclose(u.detach().cpu().numpy(), o["u"], rtol=1e-4, atol=1e-5, err_msg="u%d" % call)
        np.testing.assert_allclose(ctrl.lamda_prev.cpu().numpy(), o["lam"], rtol=1e-5, atol=1e-7, err_msg="lam%d" % call)
        np.testing.assert_array_equal(ctrl.rho_prev.cpu().numpy(), o["rho"])
        dQ, dq = aso.backward(o["L"], o["xu"], gxu)
        np.testing.assert_allclose(C.grad.diagonal(dim1=-2, dim2=-1).cpu().numpy(), dQ, rtol=1e-4, atol=1e-6,
                                   err_msg="dC%d" % call)
        np.testing.assert_allclose(cc.grad.cpu().numpy(), dq, rtol=1e-4, atol=1e-6, err_msg="dc%d" % call)
        # the warm-started second call starts from the float32 solution of the first (AL_mpc.py:250-251)
        xs, us = (o[k].astype(np.float32).astype(np.float64) for k in ("x", "u"))
        lam, rho, history = o["lam"], o["rho"], o["history"]
