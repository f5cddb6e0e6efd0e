"""The block-tridiagonal NewtonAL kernels for caller-linearised dynamics at the WIDE pairs (16 < n + m <= 32:
DQP_BAND_WIDE_SIZES, csrc/dqp_al_banded_wide.hip): Given<n, m> on a 32-lane half-wavefront, two problems per wavefront,
reached through dqp_al_banded_newton_step_jac and dqp_al_banded_solve(dims, 0, ...) with a factor buffer of
dqp_al_banded_jac_factor_bytes.

  * kernel vs the dense numpy oracle (oracle/al_oracle.py): update and factor solve rtol 1e-8 / atol 1e-10, B = 37
    (ragged at two problems per wavefront) and B = 1, the launched instantiation checked through the library's trace;
  * non-positive pivots per problem and per knot, on both halves of a wavefront, the partner unaffected;
  * the batch rolled by one gives bit-identical results;
  * (13, 4) with a decoupled dummy state against the 16-lane Given<12, 4> kernel;
  * AL_mpc.MPC end to end with a caller's module against oracle/al_solve_oracle.py, and against the reference's own
    AL_mpc.MPC (tests/golden/ALW_n13_m4_T6_b3.npz, make_golden_alw.py), to which the oracle is pinned here too;
  * one Newton step at T = 30, B = 1024: residual of the block-tridiagonal system.
"""
import contextlib
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import al_oracle
from oracle import al_solve_oracle as aso
from test_al_banded_wide_cpu import band_wide_sizes
from test_gpu_al_given import CallerToy, UT, dev, given_launches, oracle_step, problem, run_given

pytestmark = pytest.mark.gpu
WIDE = band_wide_sizes()
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ALW_n13_m4_T6_b3.npz")


def run_wide(p, trace=False, solve=True):
    """dqp_al_banded_newton_step_jac then dqp_al_banded_solve(dims, 0, factor, rhs) -> numpy (update, info, solve, trace)"""
    from diff_qp_mpc_amd import _lib
    lib = _lib.load()
    B, T, nt = p["xu"].shape
    n = p["x0"].shape[1]
    t = {k: dev(v).contiguous() for k, v in p.items()}
    dims = _lib.dqp_al_mpc_dims(B, n, nt - n, T)
    nbytes = int(lib.dqp_al_banded_jac_factor_bytes(ctypes.byref(dims)))
    assert nbytes == B * T * nt * (nt + 1 + n) * 8
    assert lib.dqp_al_banded_factor_bytes(ctypes.byref(dims), 0) == 0
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
        if solve:
            assert lib.dqp_al_banded_solve(ctypes.byref(dims), 0, P(fac), P(t["rhs"]), P(out), None) == 0
        torch.cuda.synchronize()
    return upd.cpu().numpy(), info.cpu().numpy(), out.cpu().numpy(), tr


CASES = [(n, m, T, B) for n, m in WIDE for T in (2, 4, 11) for B in (37, 1)]
CASES += [(n, m, 30, B) for n, m in [(13, 4), (24, 8)] for B in (37, 1)]


def test_wide_pairs():
    assert sorted(WIDE) == [(13, 4), (14, 7), (24, 8)]


@pytest.mark.parametrize("n,m,T,B", CASES)
def test_wide_newton_step_vs_dense_oracle(n, m, T, B):
    p = problem(n, m, T, B=B, seed=1000 * n + 10 * m + T)
    upd_ref, L_ref, info_ref = oracle_step(p)
    assert not info_ref.any()
    upd, info, out, tr = run_wide(p, trace=True)
    newton, solve = given_launches(tr)
    assert newton == {(n, m, 32, False)}, tr.records
    assert solve == {(n, m, 32)}, tr.records
    assert (info == 0).all(), info
    np.testing.assert_allclose(upd.reshape(B, -1), upd_ref, **UT)
    np.testing.assert_allclose(out.reshape(B, -1), al_oracle.chol_solve_neg(L_ref, p["rhs"].reshape(B, -1)), **UT)


@pytest.mark.parametrize("n,m,T", [(n, m, T) for n, m in WIDE for T in (4, 11)])
def test_wide_pivot_failure_is_per_problem_and_knot(n, m, T):
    """Two problems get a control cost of -1e3 at knot t0 = T // 2 (rho 1): one at an even and one at an odd batch
    index, i.e. on the first and on the second half of a wavefront.  Their info is 1 + t0; every other problem, the
    wavefront partners (11 and 34) included, keeps info 0 and the oracle's update and factor solve."""
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
    upd, info, out, _ = run_wide(p)
    np.testing.assert_array_equal(info[bad], 1 + t0)
    np.testing.assert_array_equal(info[good], 0)
    np.testing.assert_allclose(upd.reshape(B, -1)[good], upd_ref[good], **UT)
    np.testing.assert_allclose(out.reshape(B, -1)[good],
                               al_oracle.chol_solve_neg(L_ref[good], p["rhs"].reshape(B, -1)[good]), **UT)


@pytest.mark.parametrize("n,m,T", [(n, m, T) for n, m in WIDE for T in (4, 11)])
def test_wide_results_do_not_depend_on_batch_position(n, m, T):
    """The batch rolled by one moves every problem to the other half of its wavefront: after un-rolling, update, info
    and factor solve are bit for bit those of the unrolled batch."""
    p = problem(n, m, T, seed=5 + 1000 * n + 10 * m + T)
    rolled = {k: (v if k in ("lo", "hi") else np.roll(v, 1, axis=0)) for k, v in p.items()}
    upd, info, out, _ = run_wide(p)
    upd_r, info_r, out_r, _ = run_wide(rolled)
    assert (info == 0).all()
    np.testing.assert_array_equal(np.roll(info_r, -1, axis=0), info)
    np.testing.assert_array_equal(np.roll(upd_r, -1, axis=0), upd)
    np.testing.assert_array_equal(np.roll(out_r, -1, axis=0), out)


@pytest.mark.parametrize("T", [4, 11])
def test_wide_equals_narrow_with_a_decoupled_dummy_state(T):
    """A (12, 4) problem extended to (13, 4) by one state that nothing couples to (unit cost, zero linear cost, zero
    Jx / Ju rows and columns, x_next = 0, zero start, zero multipliers): the 32-lane kernel's update on the real
    variables is the Given<12, 4>, 16 kernel's to rtol 1e-10 / atol 1e-12 (summation order only), the dummy's is
    exactly zero."""
    n, m, B = 12, 4, 37
    p = problem(n, m, T, B=B, seed=400 + T)
    upd16, info16, out16, _ = run_given(p, 16)
    assert (info16 == 0).all()
    real = np.r_[0:n, n + 1:n + 1 + m]

    def widen(a, axis, fill=0.0):            # a zero (or `fill`) inserted at state index 12
        return np.insert(a, n, fill, axis=axis)

    w = dict(xu=widen(p["xu"], 2), Qd=widen(p["Qd"], 2, 1.0), q=widen(p["q"], 2), rhs=widen(p["rhs"], 2),
             rho=p["rho"], lo=p["lo"], hi=p["hi"], x0=widen(p["x0"], 1), xn=widen(p["xn"], 2),
             Jx=widen(widen(p["Jx"], 2), 3), Ju=widen(p["Ju"], 2))
    w["lam"] = np.concatenate((widen(p["lam"][:, :T * n].reshape(B, T, n), 2).reshape(B, -1), p["lam"][:, T * n:]), 1)
    upd, info, out, tr = run_wide(w, trace=True)
    newton, solve = given_launches(tr)
    assert newton == {(13, 4, 32, False)} and solve == {(13, 4, 32)}, tr.records
    assert (info == 0).all()
    np.testing.assert_allclose(upd[:, :, real], upd16, rtol=1e-10, atol=1e-12)
    np.testing.assert_array_equal(upd[:, :, n], 0.0)
    np.testing.assert_allclose(out[:, :, real], out16, rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(out[:, :, n], -w["rhs"][:, :, n] / (1.0 + p["rho"][:, :1]), rtol=1e-10, atol=1e-12)


def _mpc(n, m, T, B, lo, hi, x0, x_init, u_init):
    from diff_qp_mpc_amd import AL_mpc
    ctrl = AL_mpc.MPC(n, m, T, u_lower=dev(lo), u_upper=dev(hi), n_batch=B, verbose=0, solver_type="dense",
                      dtype=torch.float64, eps=1e-5, exit_unconverged=False, backprop=False)
    ctrl.reinitialize(dev(x0), torch.ones(B, T, 1, device="cuda"))
    ctrl.x_init, ctrl.u_init = dev(x_init), dev(u_init)
    return ctrl


def _call(ctrl, mod, x0, Qd, c, n, m):
    """one AL_mpc.MPC call with the loss sum(x) + 2 sum(u) -> x, u, dC diagonal, dc; the trace must show the wide
    Newton and solve kernels and no other Given kernel"""
    from diff_qp_mpc_amd import _lib, al_utils
    C = torch.diag_embed(dev(Qd)).requires_grad_()
    cc = dev(c, grad=True)
    with _lib.trace(4096) as tr:
        x, u = ctrl(dev(x0), al_utils.QuadCost(C, cc), mod, mod.jac)
        (x.double().sum() + 2.0 * u.double().sum()).backward()
        torch.cuda.synchronize()
    newton, solve = given_launches(tr)
    assert newton == {(n, m, 32, False)}, tr.records
    assert solve == {(n, m, 32)}, tr.records
    return (x.detach().cpu().numpy(), u.detach().cpu().numpy(), C.grad.diagonal(dim1=-2, dim2=-1).cpu().numpy(),
            cc.grad.cpu().numpy())


@pytest.mark.parametrize("n,m,T,B", [(13, 4, 6, 5), (24, 8, 4, 3)])
def test_al_mpc_caller_module_wide_vs_al_solve_oracle(n, m, T, B):
    """AL_mpc.MPC with CallerToy at a wide pair against oracle/al_solve_oracle.py: a cold call and the warm-started
    second call, with the tolerances of test_gpu_al_given.py::test_al_mpc_caller_module_vs_al_solve_oracle."""
    from diff_qp_mpc_amd.dynamics import recognise
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
    ctrl = _mpc(n, m, T, B, lo, hi, x0, x_init, u_init)
    gxu = np.concatenate((np.ones((B, T, n)), 2.0 * np.ones((B, T, m))), 2)
    lam, rho, history = np.zeros((B, T * n + 2 * T * m)), np.ones((B, 1)), None
    xs, us = x_init, u_init
    for call in range(2):
        x, u, dC, dc = _call(ctrl, mod, x0, Qd, c, n, m)
        o = aso.al_solve(xs, us, x0, Qd, c, lo, hi, mod.step_np, lam, rho, history=history)
        assert not o["chol_fail"]
        np.testing.assert_allclose(x, o["x"], rtol=1e-4, atol=1e-5, err_msg="x%d" % call)
        np.testing.assert_allclose(u, o["u"], rtol=1e-4, atol=1e-5, err_msg="u%d" % call)
        np.testing.assert_allclose(ctrl.lamda_prev.cpu().numpy(), o["lam"], rtol=1e-5, atol=1e-7, err_msg="lam%d" % call)
        np.testing.assert_array_equal(ctrl.rho_prev.cpu().numpy(), o["rho"])
        dQ, dq = aso.backward(o["L"], o["xu"], gxu)
        np.testing.assert_allclose(dC, dQ, rtol=1e-4, atol=1e-6, err_msg="dC%d" % call)
        np.testing.assert_allclose(dc, dq, rtol=1e-4, atol=1e-6, err_msg="dc%d" % call)
        xs, us = (o[k].astype(np.float32).astype(np.float64) for k in ("x", "u"))
        lam, rho, history = o["lam"], o["rho"], o["history"]


def _golden_toy(g):
    mod = CallerToy(13, 4, dt=float(g["in_dt"]))
    np.testing.assert_array_equal(mod.A.numpy(), g["in_A"])          # the fixture's map is CallerToy's
    np.testing.assert_array_equal(mod.Bm.numpy(), g["in_Bm"])
    return mod


def test_al_mpc_wide_vs_reference():
    """The reference's own AL_mpc.MPC (CPU, dense Jacobian and Hessian) on CallerToy's map at (13, 4), T 6, B 3: cold
    and warm-started call, with the tolerances of test_gpu_al.py::test_al_mpc_two_calls_vs_reference (gradients of the
    second call as those of the first)."""
    g = np.load(GOLDEN)
    mod = _golden_toy(g)
    B, T = g["in_Qd"].shape[:2]
    ctrl = _mpc(13, 4, T, B, g["in_u_lower"], g["in_u_upper"], g["in_x0"], g["in_x_init"], g["in_u_init"])
    x, u, dC, dc = _call(ctrl, mod, g["in_x0"], g["in_Qd"], g["in_c"], 13, 4)
    np.testing.assert_allclose(x, g["x1"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(u, g["u1"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(ctrl.lamda_prev.cpu().numpy(), g["lam1"], rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(ctrl.rho_prev.cpu().numpy(), g["rho1"], rtol=0, atol=0)
    np.testing.assert_allclose(dC, g["dC1"], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(dc, g["dc1"], rtol=1e-4, atol=1e-6)
    x, u, dC, dc = _call(ctrl, mod, g["in_x0"], g["in_Qd"], g["in_c"], 13, 4)
    np.testing.assert_allclose(x, g["x2"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(u, g["u2"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(ctrl.lamda_prev.cpu().numpy(), g["lam2"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(ctrl.rho_prev.cpu().numpy(), g["rho2"], rtol=0, atol=0)
    np.testing.assert_allclose(dC, g["dC2"], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(dc, g["dc2"], rtol=1e-4, atol=1e-6)


def test_al_solve_oracle_vs_reference_at_a_wide_pair():
    """oracle/al_solve_oracle.py against the same fixture (numpy only): ties the oracle the kernels are tested against
    to the reference at a wide shape, with the same tolerances."""
    g = np.load(GOLDEN)
    mod = _golden_toy(g)
    B, T = g["in_Qd"].shape[:2]
    n, m = 13, 4
    gxu = np.concatenate((np.ones((B, T, n)), 2.0 * np.ones((B, T, m))), 2)
    lam, rho, history = np.zeros((B, T * n + 2 * T * m)), np.ones((B, 1)), None
    xs, us = g["in_x_init"], g["in_u_init"]
    for call, lam_atol in ((1, 1e-7), (2, 1e-6)):
        o = aso.al_solve(xs, us, g["in_x0"], g["in_Qd"], g["in_c"], g["in_u_lower"], g["in_u_upper"], mod.step_np, lam, rho,
                         history=history)
        assert not o["chol_fail"]
        np.testing.assert_allclose(o["x"], g["x%d" % call], rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(o["u"], g["u%d" % call], rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(o["lam"], g["lam%d" % call], rtol=1e-5, atol=lam_atol)
        np.testing.assert_array_equal(o["rho"], g["rho%d" % call])
        dQ, dq = aso.backward(o["L"], o["xu"], gxu)
        np.testing.assert_allclose(dQ, g["dC%d" % call], rtol=1e-4, atol=1e-6)
        np.testing.assert_allclose(dq, g["dc%d" % call], rtol=1e-4, atol=1e-6)
        xs, us = (o[k].astype(np.float32).astype(np.float64) for k in ("x", "u"))
        lam, rho, history = o["lam"], o["rho"], o["history"]


def band_system(p, b):
    """Hessian (T nt, T nt) and merit gradient (T nt) of problem b of `problem()`'s data, assembled from the
    block-tridiagonal blocks as the kernel header describes them (numpy, independent of oracle/al_oracle.py)"""
    T, nt = p["xu"].shape[1:]
    n = p["x0"].shape[1]
    m = nt - n
    rho = p["rho"][b, 0]
    xu, lam = p["xu"][b], p["lam"][b]
    lam_dyn = lam[:T * n].reshape(T, n)                  # rows t < T - 1: dynamics of knot t; row T - 1: x_0 rows
    lam_box = lam[T * n:].reshape(T, 2, m)
    H = np.zeros((T * nt, T * nt))
    grad = (p["Qd"][b] * xu + p["q"][b]).copy()          # (T, nt)
    for t in range(T):
        s = slice(t * nt, (t + 1) * nt)
        D = p["Qd"][b, t].copy()
        D[:n] += rho                                     # identity block of the rows that give x_t
        up, lo = xu[t, n:] - p["hi"], p["lo"] - xu[t, n:]
        D[n:] += rho * ((up > 0) * 1.0 + (lo > 0) * 1.0)
        grad[t, n:] += (lam_box[t, 0] + rho * np.maximum(up, 0.0)) - (lam_box[t, 1] + rho * np.maximum(lo, 0.0))
        H[s, s] += np.diag(D)
        if t == 0:
            grad[0, :n] += lam_dyn[T - 1] + rho * (xu[0, :n] - p["x0"][b])
        if t < T - 1:
            J = np.concatenate((p["Jx"][b, t], p["Ju"][b, t]), 1)            # (n, nt)
            mu = lam_dyn[t] + rho * (xu[t + 1, :n] - p["xn"][b, t])
            grad[t] -= J.T @ mu
            grad[t + 1, :n] += mu
            H[s, s] += rho * J.T @ J
            sx = slice((t + 1) * nt, (t + 1) * nt + n)
            H[sx, s] -= rho * J
            H[s, sx] -= rho * J.T
    return H, grad.reshape(-1)


def test_wide_newton_step_at_scale():
    """(13, 4), T = 30, B = 1024, one Newton step: every info 0, and for 32 sampled problems the residual of the
    block-tridiagonal system assembled in numpy, max |H upd + grad| / max |grad| < 1e-9 (cond(H) ~ 1e4 x fp64 round-off,
    three decades of margin)."""
    n, m, T, B = 13, 4, 30, 1024
    p = problem(n, m, T, B=B, seed=2024)
    upd, info, _, _ = run_wide(p, solve=False)
    assert (info == 0).all(), np.flatnonzero(info)
    worst = 0.0
    for b in np.linspace(0, B - 1, 32).astype(int):
        H, gv = band_system(p, b)
        worst = max(worst, np.abs(H @ upd[b].reshape(-1) + gv).max() / np.abs(gv).max())
    print("scale: worst residual %.3e" % worst)
    assert worst < 1e-9, worst
