"""State bounds on the caller-linearised block-tridiagonal NewtonAL step (dqp_al_banded_newton_step_jac_xbounds:
al_banded_newton_kernel<BoxBounds<Given<n, m>>, G, LF> at every pair of DQP_BAND_SIZES and DQP_BAND_WIDE_SIZES), in the
merit kernel (dqp_al_merit_xbounds) and through AL_mpc.MPC / policies.Tracking_MPC with a caller's own dynamics module.

The yardstick is the pinned numpy oracle (oracle/al_oracle.py, oracle/al_solve_oracle.py) with the state rows appended
by tests/al_xbounds_oracle.py.  Tolerances: kernel against the dense oracle rtol 1e-8 / atol 1e-10
(test_gpu_al_given.UT); AL_mpc.MPC against al_solve: x, u 1e-4 / 1e-5, multipliers rtol 1e-5 (atol 1e-7), rho exact,
dC / dc 1e-4 / 1e-6 (test_gpu_al_given.test_al_mpc_caller_module_vs_al_solve_oracle); the merit kernel against the torch
merit on the same fp64 inputs rtol 1e-12 (summation order only).
"""
import contextlib
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import al_xbounds_oracle as xo
from oracle import al_oracle
from oracle import al_solve_oracle as aso
from test_al_banded_cpu import band_sizes
from test_al_banded_wide_cpu import band_wide_sizes
from test_gpu_al_given import CASES as NARROW_CASES, CallerToy, UT, dev, groups, lds_factor, problem
from test_gpu_al_wide import CASES as WIDE_CASES

pytestmark = pytest.mark.gpu
PAIRS, WIDE = band_sizes(), band_wide_sizes()
BOX_NEWTON_RE = re.compile(r"al_banded_newton_kernel<dqp::BoxBounds<[^<>]*Given<(\d+), (\d+)>\s*>, (\d+), (true|false)>")
SOLVE_RE = re.compile(r"al_banded_solve_kernel<[^<>]*Given<(\d+), (\d+)>, (\d+)>")
MERIT_X = "al_merit_kernel<true, true>"
KINK = 1e-6             # no |x - bound| below this: a row on its kink may clamp either way within rounding
# The dense oracle of a T = 30 wide case at B = 37 (nz up to 960, 2640 rows: its einsum Hessian) takes minutes: its two
# results are recorded by tests/golden/make_golden_al_given_xbounds.py, which runs oracle_xstep below on xproblem's data.
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ALGX_n%d_m%d_T%d_b%d.npz")
RECORDED = [(13, 4, 30, 37), (24, 8, 30, 37)]


@pytest.fixture(autouse=True)
def _auto_lane_group():
    yield
    from diff_qp_mpc_amd import _lib
    _lib.load().dqp_al_lane_group(0)


def P(t):
    return ctypes.c_void_p(t.data_ptr())


def xproblem(n, m, T, B=37, seed=0):
    """test_gpu_al_given.problem plus a state box of -+0.4, jittered per element, as (B, T, n) arrays (the states are
    0.5 N(0, 1): a good part of the rows is active), and random multipliers on the state rows"""
    p = problem(n, m, T, B=B, seed=seed)
    rng = np.random.default_rng(seed + 123457)
    p["xl"] = -0.4 + 0.05 * rng.uniform(-1.0, 1.0, (B, T, n))
    p["xh"] = 0.4 + 0.05 * rng.uniform(-1.0, 1.0, (B, T, n))
    p["lam"] = np.concatenate((p["lam"], rng.standard_normal((B, 2 * T * n))), 1)
    return p


def oracle_xstep(p, lo=None, hi=None, xl=None, xh=None):
    """al_oracle.newton_update over the extended rows -> (update, L, info); asserts on the oracle's rows that some state
    rows are active, some are not, and none sits on its kink.  lo / hi / xl / xh: the expanded arrays of another layout."""
    B, T, nt = p["xu"].shape
    n = p["x0"].shape[1]
    m = nt - n
    lo, hi = (p["lo"], p["hi"]) if lo is None else (lo, hi)
    xl, xh = (p["xl"], p["xh"]) if xl is None else (xl, xh)

    def step(x, u):
        return (p["xn"].reshape(B * (T - 1), n), p["Jx"].reshape(B * (T - 1), n, n), p["Ju"].reshape(B * (T - 1), n, m))

    with xo.extended(xl, xh):
        res, resc, J, Jc = al_oracle.constraint_jacobian(p["xu"], p["x0"], lo, hi, step=step)
    assert res.shape == (B, xo.ncon_x(n, m, T)) == p["lam"].shape
    check_rows(res, n, m, T)
    grad = al_oracle.merit_grad(p["xu"], p["Qd"], p["q"], p["lam"], p["rho"], resc, J, Jc)
    return al_oracle.newton_update(Jc, p["Qd"].reshape(B, -1), p["rho"], grad)


def check_rows(res, n, m, T):
    """on the oracle's rows: control and state rows both active and inactive somewhere, no state row on its kink"""
    iq, sx = res[:, T * n:T * n + 2 * T * m], res[:, T * n + 2 * T * m:]
    assert (iq > 0).any() and (iq <= 0).any()
    assert (sx > 0).any() and (sx <= 0).any()
    assert np.abs(sx).min() >= KINK, np.abs(sx).min()


def step_reference(p):
    """(update, factor solve of p["rhs"], info) of the extended dense oracle; for the RECORDED cases read from the file
    the generator wrote, after checking that the file belongs to these inputs and the conditions on the rows"""
    B, T, nt = p["xu"].shape
    n = p["x0"].shape[1]
    key = (n, nt - n, T, B)
    if key not in RECORDED:
        upd, L, info = oracle_xstep(p)
        return upd, al_oracle.chol_solve_neg(L, p["rhs"].reshape(B, -1)), info
    g = np.load(GOLDEN % key)
    for k in ("xu", "lam", "xl", "xh", "Jx", "rhs"):
        assert float(p[k].sum()) == float(g["sum_" + k]), k
    step = lambda x, u: (p["xn"].reshape(-1, n), None, None)
    with xo.extended(p["xl"], p["xh"]):
        res, _ = aso.residuals(p["xu"], p["x0"], p["lo"], p["hi"], step)
    check_rows(res, n, nt - n, T)
    return g["upd"], g["sol"], g["info"]


def run_box(p, group, trace=False, lo=None, hi=None, xl=None, xh=None, entry="xbounds"):
    """dqp_al_banded_newton_step_jac_xbounds (or, entry="bounds", its twin without the state box) then
    dqp_al_banded_solve(dims, 0, factor, rhs) -> numpy (update, info, solve, factor, trace).  lo / hi / xl / xh: bounds
    in any of the four shapes; default the problem's."""
    from diff_qp_mpc_amd import _lib, al_utils
    lib = _lib.load()
    assert lib.dqp_al_lane_group(0 if group == 32 else int(group)) == 0
    B, T, nt = p["xu"].shape
    n = p["x0"].shape[1]
    m = nt - n
    t = {k: dev(v).contiguous() for k, v in p.items()}
    lo, hi = (p["lo"], p["hi"]) if lo is None else (lo, hi)
    xl, xh = (p["xl"], p["xh"]) if xl is None else (xl, xh)
    bd = al_utils.bounds_layout(dev(lo), dev(hi), B, T, m)
    xbd = al_utils.bounds_layout(dev(xl), dev(xh), B, T, n)
    dims = _lib.dqp_al_mpc_dims(B, n, m, T)
    nbytes = int(lib.dqp_al_banded_jac_factor_bytes(ctypes.byref(dims)))
    assert nbytes == B * T * nt * (nt + 1 + n) * 8
    fac = torch.full((nbytes // 8,), np.nan, dtype=torch.float64, device="cuda")
    upd = torch.full((B, T, nt), np.nan, dtype=torch.float64, device="cuda")
    out = torch.full((B, T, nt), np.nan, dtype=torch.float64, device="cuda")
    info = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    head = (ctypes.byref(dims), P(t["xu"]), P(t["x0"]), P(t["Qd"]), P(t["q"]), P(t["lam"]), P(t["rho"].reshape(B).contiguous()))
    tail = (P(t["xn"]), P(t["Jx"]), P(t["Ju"]), P(upd), P(fac), P(info), None)
    with _lib.trace(16) if trace else contextlib.nullcontext() as tr:
        if entry == "xbounds":
            rc = lib.dqp_al_banded_newton_step_jac_xbounds(*head, bd.ref(), xbd.ref(), *tail)
        else:
            rc = lib.dqp_al_banded_newton_step_jac_bounds(*head, bd.ref(), *tail)
        assert rc == 0
        assert lib.dqp_al_banded_solve(ctypes.byref(dims), 0, P(fac), P(t["rhs"]), P(out), None) == 0
        torch.cuda.synchronize()
    return upd.cpu().numpy(), info.cpu().numpy(), out.cpu().numpy(), fac.cpu().numpy(), tr


def box_launches(tr):
    """-> ({(n, m, group, lf)} of the BoxBounds<Given<>> Newton kernels, {(n, m, group)} of the Given solve kernels)"""
    newton, solve = set(), set()
    for k, _ in tr.records:
        a = BOX_NEWTON_RE.search(k)
        if a:
            newton.add((int(a.group(1)), int(a.group(2)), int(a.group(3)), a.group(4) == "true"))
        a = SOLVE_RE.search(k)
        if a:
            solve.add((int(a.group(1)), int(a.group(2)), int(a.group(3))))
    return newton, solve


# ------------------------------------------------------------------ 1
# every narrow pair x its lane groups x T in (2, 4, 11) at B = 37; the wide pairs at the shapes of test_gpu_al_wide
STEP_CASES = [(n, m, g, T, 37) for n, m, g, T in NARROW_CASES] + [(n, m, 32, T, B) for n, m, T, B in WIDE_CASES]


def step_seed(n, m, T):
    return 1000 * n + 10 * m + T + 3


def test_step_cases_cover_every_instantiation():
    newton = {(n, m, g, lds_factor(n, m, T, g)) for n, m, g, T, _ in STEP_CASES}
    assert len(newton) == 46 + 3 and {k[:2] for k in newton} == set(PAIRS) | set(WIDE)
    assert {(n, m) for n, m, g, lf in newton if lf} == {(n, m) for n, m in PAIRS if 6 <= n + m <= 8}


@pytest.mark.parametrize("n,m,group,T,B", STEP_CASES)
def test_box_newton_step_vs_extended_dense_oracle(n, m, group, T, B):
    p = xproblem(n, m, T, B=B, seed=step_seed(n, m, T))
    upd_ref, sol_ref, info_ref = step_reference(p)
    assert not info_ref.any()
    upd, info, out, _, tr = run_box(p, group, trace=True)
    newton, solve = box_launches(tr)
    assert newton == {(n, m, group, lds_factor(n, m, T, group))}, tr.records
    assert solve == {(n, m, group)}, tr.records
    assert sum("al_banded_newton_kernel" in k for k, _ in tr.records) == 1, tr.records
    assert (info == 0).all(), info
    np.testing.assert_allclose(upd.reshape(B, -1), upd_ref, **UT)
    np.testing.assert_allclose(out.reshape(B, -1), sol_ref, **UT)


# ------------------------------------------------------------------ 2
def layouts_of(full, shape_kind):
    """a (B, T, w) array reduced to one of the four shapes, and that shape expanded again (what the kernel must read)"""
    B, T, w = full.shape
    a = {"vec": full[0, 0], "T": full[0], "B1": full[:, :1], "BT": full}[shape_kind]
    return np.ascontiguousarray(a), np.ascontiguousarray(np.broadcast_to(a, (B, T, w)))


@pytest.mark.parametrize("n,m,group", [(3, 1, 8), (12, 4, 16), (13, 4, 32)])
@pytest.mark.parametrize("ukind", ["vec", "BT"])
@pytest.mark.parametrize("xkind", ["vec", "T", "B1", "BT"])
def test_box_layouts(n, m, group, ukind, xkind):
    """every state-box shape with the vector and the (B, T, m) control box: the kernel's update and factor solve against
    the oracle that is given the expanded arrays"""
    T, B = 5, 37
    p = xproblem(n, m, T, B=B, seed=31 + 1000 * n + m)
    rng = np.random.default_rng(n + m)
    ufull_lo = -0.3 + 0.1 * rng.uniform(-1.0, 1.0, (B, T, m))
    ufull_hi = 0.3 + 0.1 * rng.uniform(-1.0, 1.0, (B, T, m))
    (lo, lo_e), (hi, hi_e) = layouts_of(ufull_lo, ukind), layouts_of(ufull_hi, ukind)
    (xl, xl_e), (xh, xh_e) = layouts_of(p["xl"], xkind), layouts_of(p["xh"], xkind)
    upd_ref, L_ref, info_ref = oracle_xstep(p, lo_e, hi_e, xl_e, xh_e)
    assert not info_ref.any()
    upd, info, out, _, tr = run_box(p, group, trace=True, lo=lo, hi=hi, xl=xl, xh=xh)
    assert box_launches(tr)[0] == {(n, m, group, False)}, tr.records
    assert (info == 0).all()
    np.testing.assert_allclose(upd.reshape(B, -1), upd_ref, **UT)
    np.testing.assert_allclose(out.reshape(B, -1), al_oracle.chol_solve_neg(L_ref, p["rhs"].reshape(B, -1)), **UT)


# ------------------------------------------------------------------ 3
# one pair per group width (and the LDS-resident factor): (n, m, group, T)
WIDTH_CASES = [(3, 1, 8, 4), (6, 2, 8, 4), (12, 4, 16, 4), (13, 4, 32, 4)]


@pytest.mark.parametrize("n,m,group,T", WIDTH_CASES)
def test_inactive_box_step_is_the_bounds_step_bit_for_bit(n, m, group, T):
    """A box of -+1e30 with zero state multipliers adds exact zeros to the gradient and to the diagonal: update, info
    and the kept factor are those of dqp_al_banded_newton_step_jac_bounds bit for bit."""
    B = 37
    p = xproblem(n, m, T, B=B, seed=9 + 1000 * n + m)
    p["xl"], p["xh"] = np.full(n, -1e30), np.full(n, 1e30)
    p["lam"][:, T * n + 2 * T * m:] = 0.0
    upd, info, out, fac, tr = run_box(p, group, trace=True)
    assert box_launches(tr)[0] == {(n, m, group, lds_factor(n, m, T, group))}, tr.records
    q = dict(p, lam=p["lam"][:, :T * n + 2 * T * m].copy())
    upd0, info0, out0, fac0, tr0 = run_box(q, group, trace=True, entry="bounds")
    assert not box_launches(tr0)[0] and any("al_banded_newton_kernel" in k for k, _ in tr0.records), tr0.records
    assert (info0 == 0).all() and np.isfinite(fac0).all()
    np.testing.assert_array_equal(info, info0)
    np.testing.assert_array_equal(upd, upd0)
    np.testing.assert_array_equal(fac, fac0)
    np.testing.assert_array_equal(out, out0)


# ------------------------------------------------------------------ 4
@pytest.mark.parametrize("n,m,group,T", [(n, m, g, T) for n, m, g, _ in WIDTH_CASES for T in (4, 11)])
def test_box_results_do_not_depend_on_batch_position(n, m, group, T):
    B = 37
    p = xproblem(n, m, T, B=B, seed=5 + 1000 * n + 10 * m + T)
    rolled = {k: (v if k in ("lo", "hi") else np.roll(v, 1, axis=0)) for k, v in p.items()}
    upd, info, out, _, _ = run_box(p, group)
    upd_r, info_r, out_r, _, _ = run_box(rolled, group)
    assert (info == 0).all()
    np.testing.assert_array_equal(np.roll(info_r, -1, axis=0), info)
    np.testing.assert_array_equal(np.roll(upd_r, -1, axis=0), upd)
    np.testing.assert_array_equal(np.roll(out_r, -1, axis=0), out)


# ------------------------------------------------------------------ 5
@pytest.mark.parametrize("n,m,group,T", [(n, m, g, T) for n, m, g in [(5, 2, 16), (5, 2, 8), (12, 4, 16), (13, 4, 32)]
                                         for T in (4, 11)])
def test_box_pivot_failure_is_per_problem_and_knot(n, m, group, T):
    """test_gpu_al_given's construction with a state box: a control cost of -1e3 at knot t0 = T // 2 and rho 1 on two
    problems.  Their info is 1 + t0; every other problem keeps info 0 and the oracle's update and factor solve."""
    p = xproblem(n, m, T, seed=77 + 1000 * n + 10 * m + T)
    B, nt, t0 = p["xu"].shape[0], n + m, T // 2
    bad = [10, 35]
    for b in bad:
        p["Qd"][b, t0, n:] = -1e3
        p["rho"][b] = 1.0
    upd_ref, L_ref, info_ref = oracle_xstep(p)
    good = np.setdiff1d(np.arange(B), bad)
    assert (info_ref[bad] > 0).all() and not info_ref[good].any()
    np.testing.assert_array_equal(1 + (info_ref[bad] - 1) // nt, 1 + t0)
    upd, info, out, _, _ = run_box(p, group)
    np.testing.assert_array_equal(info[bad], 1 + t0)
    np.testing.assert_array_equal(info[good], 0)
    np.testing.assert_allclose(upd.reshape(B, -1)[good], upd_ref[good], **UT)
    np.testing.assert_allclose(out.reshape(B, -1)[good],
                               al_oracle.chol_solve_neg(L_ref[good], p["rhs"].reshape(B, -1)[good]), **UT)


# ------------------------------------------------------------------ 6
@pytest.mark.parametrize("T", [2, 17, 33])
@pytest.mark.parametrize("n,m", [(3, 1), (12, 4), (24, 8), (7, 2)])
def test_merit_kernel_vs_torch_merit(n, m, T):
    """dqp_al_merit_xbounds against al_utils.merit_function's torch ops (taken with autograd enabled) on the same fp64
    inputs, 20 candidates, every layout of both boxes; (7, 2) is a pair without a Newton kernel."""
    from diff_qp_mpc_amd import _lib, al_utils
    lib = _lib.load()
    K, B, nt = 20, 5, n + m
    rng = np.random.default_rng(100 * n + m + T)
    mod = CallerToy(n, m)
    xu = dev(0.5 * rng.standard_normal((K, B, T, nt)))
    x0 = dev(xu[0, :, 0, :n].cpu().numpy() + 0.1 * rng.standard_normal((B, n)))
    Qd, q = dev(rng.random((B, T, nt)) + 0.1), dev(rng.standard_normal((B, T, nt)))
    lam, rho = dev(rng.standard_normal((B, xo.ncon_x(n, m, T)))), dev(rng.choice([1.0, 10.0, 100.0], size=(B, 1)))
    ufull = (-0.3 + 0.1 * rng.uniform(-1, 1, (B, T, m)), 0.3 + 0.1 * rng.uniform(-1, 1, (B, T, m)))
    xfull = (-0.4 + 0.05 * rng.uniform(-1, 1, (B, T, n)), 0.4 + 0.05 * rng.uniform(-1, 1, (B, T, n)))
    flat = xu.reshape(K * B, T, nt)
    xn = mod(flat[:, :-1, :n].reshape(-1, n), flat[:, :-1, n:].reshape(-1, m)).reshape(K * B, T - 1, n).contiguous()
    dims = _lib.dqp_al_mpc_dims(B, n, m, T)
    worst = 0.0
    for ukind in ("vec", "T", "B1", "BT"):
        lo, hi = (dev(layouts_of(a, ukind)[0]) for a in ufull)
        for xkind in ("vec", "T", "B1", "BT"):
            xl, xh = (dev(layouts_of(a, xkind)[0]) for a in xfull)
            with torch.enable_grad():
                want = al_utils.merit_function(xu, Qd, q, mod, x0, lam, rho, xl, xh, lo, hi)
            bd, xbd = al_utils.bounds_layout(lo, hi, B, T, m), al_utils.bounds_layout(xl, xh, B, T, n)
            got = torch.full((K * B,), np.nan, dtype=torch.float64, device="cuda")
            with _lib.trace(8) as tr:
                rc = lib.dqp_al_merit_xbounds(ctypes.byref(dims), K, P(flat), P(xn), P(x0), P(Qd), P(q), P(lam),
                                              P(rho.reshape(B).contiguous()), bd.ref(), xbd.ref(), P(got), None)
                torch.cuda.synchronize()
            assert rc == 0 and [MERIT_X in k for k, _ in tr.records] == [True], tr.records
            rel = float(((got - want).abs() / want.abs()).max())
            worst = max(worst, rel)
            np.testing.assert_allclose(got.cpu().numpy(), want.detach().cpu().numpy(), rtol=1e-12, atol=0,
                                       err_msg="%s %s" % (ukind, xkind))
            # and through merit_function itself, which takes the kernel without autograd
            with torch.no_grad(), _lib.trace(8) as tr2:
                via = al_utils.merit_function(xu, Qd, q, mod, x0, lam, rho, xl, xh, lo, hi)
                torch.cuda.synchronize()
            assert [MERIT_X in k for k, _ in tr2.records] == [True], tr2.records
            np.testing.assert_array_equal(via.cpu().numpy(), got.cpu().numpy())
    print("merit (%d, %d) T %d: max rel |kernel - torch| = %.3e" % (n, m, T, worst))


# ------------------------------------------------------------------ 7
# (n, m, T, B, group, control bounds): the last one has per-sample, per-knot control bounds at a wide pair
MPC_CASES = [(1, 1, 6, 5, 16, "vec"), (1, 1, 6, 5, 8, "vec"), (6, 2, 6, 5, 16, "vec"), (6, 2, 6, 5, 8, "vec"),
             (9, 3, 6, 5, 16, "vec"), (12, 2, 6, 5, 16, "vec"), (13, 4, 6, 5, 32, "vec"), (24, 8, 4, 3, 32, "vec"),
             (13, 4, 6, 5, 32, "BT")]
XU_TOL, LAM_TOL, GRAD_TOL = dict(rtol=1e-4, atol=1e-5), dict(rtol=1e-5, atol=1e-7), dict(rtol=1e-4, atol=1e-6)


def mpc_problem(n, m, T, B, ukind):
    """test_al_mpc_caller_module_vs_al_solve_oracle's problem and a (B, T, n) state box of about -+0.5 that the
    trajectories leave (x0 is N(0, 1))"""
    nt = n + m
    rng = np.random.default_rng(10 * n + m + T)
    mod = CallerToy(n, m)
    x0 = rng.standard_normal((B, n))
    u_init = 0.2 * rng.standard_normal((B, T, m))
    x_init = np.empty((B, T, n))
    x_init[:, 0] = x0
    for t in range(T - 1):
        x_init[:, t + 1] = mod.step_np(x_init[:, t], u_init[:, t])[0]
    p = dict(mod=mod, x0=x0, u_init=u_init, x_init=x_init, Qd=rng.random((B, T, nt)) + 0.1, c=rng.standard_normal((B, T, nt)))
    p["lo"], p["hi"] = np.full(m, -0.5), np.full(m, 0.5)
    if ukind == "BT":
        p["lo"] = -0.5 + 0.2 * rng.uniform(-1.0, 1.0, (B, T, m))
        p["hi"] = 0.5 + 0.2 * rng.uniform(-1.0, 1.0, (B, T, m))
    p["xl"] = -0.5 + 0.1 * rng.uniform(-1.0, 1.0, (B, T, n))
    p["xh"] = 0.5 + 0.1 * rng.uniform(-1.0, 1.0, (B, T, n))
    return p


_ORACLE = {}


def mpc_case(n, m, T, B, ukind):
    """the problem and the extended oracle's cold and warm call with their backward, computed once and left unchanged"""
    key = (n, m, T, B, ukind)
    if key not in _ORACLE:
        p = mpc_problem(n, m, T, B, ukind)
        gxu = np.concatenate((np.ones((B, T, n)), 2.0 * np.ones((B, T, m))), 2)
        lam, rho, history = np.zeros((B, xo.ncon_x(n, m, T))), np.ones((B, 1)), None
        xs, us, calls = p["x_init"], p["u_init"], []
        with xo.extended(p["xl"], p["xh"]):
            for _ in range(2):
                o = aso.al_solve(xs, us, p["x0"], p["Qd"], p["c"], p["lo"], p["hi"], p["mod"].step_np, lam, rho, history=history)
                assert not o["chol_fail"]
                o["dQ"], o["dq"] = aso.backward(o["L"], o["xu"], gxu)
                calls.append(o)
                # the warm-started second call starts from the float32 solution of the first (AL_mpc.py:250-251)
                xs, us = (o[k].astype(np.float32).astype(np.float64) for k in ("x", "u"))
                lam, rho, history = o["lam"], o["rho"], o["history"]
        lx = calls[0]["lam"][:, T * n + 2 * T * m:].reshape(B, T, 2 * n)
        assert (lx[:, 1:] > 0).any() and (lx == 0).any()        # a state row beyond the pinned knot 0 ends active; some never
        _ORACLE[key] = (p, calls)
    return _ORACLE[key]


def run_mpc(p, n, m, T, B, group):
    """two calls of AL_mpc.MPC with the caller's module, forward + backward -> [(dict of numpy arrays, kernel names)]"""
    from diff_qp_mpc_amd import AL_mpc, _lib, al_utils
    from diff_qp_mpc_amd.dynamics import recognise
    lib = _lib.load()
    assert lib.dqp_al_lane_group(0 if group == 32 else int(group)) == 0
    mod = p["mod"]
    assert recognise(mod, n, m) is None
    ctrl = AL_mpc.MPC(n, m, T, u_lower=dev(p["lo"]), u_upper=dev(p["hi"]), n_batch=B, verbose=0, solver_type="dense",
                      dtype=torch.float64, eps=1e-5, exit_unconverged=False, backprop=False, x_lower=dev(p["xl"]),
                      x_upper=dev(p["xh"]))
    ctrl.reinitialize(dev(p["x0"]), torch.ones(B, T, 1, device="cuda"))
    ctrl.x_init, ctrl.u_init = dev(p["x_init"]), dev(p["u_init"])
    outs = []
    for call in range(2):
        C = torch.diag_embed(dev(p["Qd"])).requires_grad_()
        cc = dev(p["c"], grad=True)
        with _lib.trace(4096) as tr:
            x, u = ctrl(dev(p["x0"]), al_utils.QuadCost(C, cc), mod, mod.jac)
            (x.double().sum() + 2.0 * u.double().sum()).backward()
            torch.cuda.synchronize()
        outs.append((dict(x=x.detach().cpu().numpy(), u=u.detach().cpu().numpy(), lam=ctrl.lamda_prev.cpu().numpy(),
                          rho=ctrl.rho_prev.cpu().numpy(), dQ=C.grad.diagonal(dim1=-2, dim2=-1).cpu().numpy().copy(),
                          dq=cc.grad.cpu().numpy().copy()), [k for k, _ in tr.records]))
    return outs


@pytest.mark.parametrize("n,m,T,B,group,ukind", MPC_CASES)
def test_al_mpc_caller_module_with_state_box_vs_extended_oracle(n, m, T, B, group, ukind):
    p, calls = mpc_case(n, m, T, B, ukind)
    got = run_mpc(p, n, m, T, B, group)
    for call, ((g, names), o) in enumerate(zip(got, calls)):
        tr = types.SimpleNamespace(records=[(k, 0) for k in names])
        newton, solve = box_launches(tr)
        assert newton and {k[:3] for k in newton} == {(n, m, group)}, names
        assert all(BOX_NEWTON_RE.search(k) for k in names if "al_banded_newton_kernel" in k), names
        assert solve == {(n, m, group)}, names
        assert any(MERIT_X in k for k in names) and all(MERIT_X in k for k in names if "al_merit_kernel" in k), names
        assert not any("al_newton_kernel" in k for k in names), names          # the dense route
        assert g["lam"].shape == (B, xo.ncon_x(n, m, T))
        assert (g["lam"][:, T * n + 2 * T * m:] > 0).any()
        for k in ("x", "u", "lam", "dQ", "dq"):
            print((n, m, T, B, group, ukind), "call", call, k, "max |gpu - oracle| = %.3e" % float(np.abs(g[k] - o[k]).max()))
        np.testing.assert_allclose(g["x"], o["x"], err_msg="x%d" % call, **XU_TOL)
        np.testing.assert_allclose(g["u"], o["u"], err_msg="u%d" % call, **XU_TOL)
        np.testing.assert_allclose(g["lam"], o["lam"], err_msg="lam%d" % call, **LAM_TOL)
        np.testing.assert_array_equal(g["rho"], o["rho"])
        np.testing.assert_allclose(g["dQ"], o["dQ"], err_msg="dC%d" % call, **GRAD_TOL)
        np.testing.assert_allclose(g["dq"], o["dq"], err_msg="dc%d" % call, **GRAD_TOL)


@pytest.mark.parametrize("n,m,T,B,group,ukind", MPC_CASES)
def test_al_mpc_general_route_agrees_with_the_device_route(n, m, T, B, group, ukind, monkeypatch):
    """AL_mpc.BANDED_USER_DYNAMICS = False sends the same call down the general route (no BoxBounds<Given<>> kernel);
    both routes agree within the tolerances of the oracle comparison"""
    from diff_qp_mpc_amd import AL_mpc
    p, _ = mpc_case(n, m, T, B, ukind)
    got = run_mpc(p, n, m, T, B, group)
    monkeypatch.setattr(AL_mpc, "BANDED_USER_DYNAMICS", False)
    ref = run_mpc(p, n, m, T, B, group)
    for call, ((g, _), (r, names)) in enumerate(zip(got, ref)):
        assert not any("BoxBounds<" in k and "Given<" in k for k in names), names
        np.testing.assert_allclose(g["x"], r["x"], err_msg="x%d" % call, **XU_TOL)
        np.testing.assert_allclose(g["u"], r["u"], err_msg="u%d" % call, **XU_TOL)
        np.testing.assert_allclose(g["lam"], r["lam"], err_msg="lam%d" % call, **LAM_TOL)
        np.testing.assert_array_equal(g["rho"], r["rho"])
        np.testing.assert_allclose(g["dQ"], r["dQ"], err_msg="dC%d" % call, **GRAD_TOL)
        np.testing.assert_allclose(g["dq"], r["dq"], err_msg="dc%d" % call, **GRAD_TOL)


# ------------------------------------------------------------------ 8
def test_tracking_mpc_with_a_state_box_and_an_unregistered_module():
    """policies.Tracking_MPC hands the box to AL_mpc.MPC; the env's module is no registered model, so the forward runs
    the BoxBounds<Given<n, m>> Newton kernel and the backward the Given solve kernel."""
    from diff_qp_mpc_amd import _lib, policies
    from diff_qp_mpc_amd.dynamics import recognise
    n, m, T, B = 6, 2, 5, 4
    mod = CallerToy(n, m)
    assert policies.RECOGNISE_ENV_DYNAMICS and recognise(mod, n, m, dt=mod.dt, device="cuda") is None
    env = types.SimpleNamespace(nx=n, nu=m, nq=n // 2, dt=mod.dt, dynamics=mod, dynamics_derivatives=mod.jac,
                                action_space=types.SimpleNamespace(low=-0.5 * np.ones(m), high=0.5 * np.ones(m)))
    args = types.SimpleNamespace(T=T, nq=n // 2, device="cuda", dtype="double", qp_iter=1, eps=1e-5, warm_start=True,
                                 bsz=B, Q=None, R=None, solver_type="al")
    rng = np.random.default_rng(4)
    xl, xh = dev(-0.5 + 0.1 * rng.uniform(-1, 1, (B, T, n))), dev(0.5 + 0.1 * rng.uniform(-1, 1, (B, T, n)))
    pol = policies.Tracking_MPC(args, env, x_lower=xl, x_upper=xh)
    assert pol.dyn is mod and pol.ctrl.nineq == 2 * T * m + 2 * T * n
    x0 = dev(rng.standard_normal((B, n)))
    x_ref = dev(0.5 * rng.standard_normal((B, T, n)), grad=True)
    u_ref = dev(np.zeros((B, T, m)))
    pol.reinitialize(x0, torch.ones(B, T, 1, device="cuda", dtype=torch.float64))
    with _lib.trace(4096) as tr:
        xs, us = pol(x0, None, x_ref, u_ref)
        (xs.double().sum() + us.double().sum()).backward()
        torch.cuda.synchronize()
    newton, solve = box_launches(tr)
    assert newton and {k[:2] for k in newton} == {(n, m)}, tr.records
    assert solve and {k[:2] for k in solve} == {(n, m)}, tr.records
    assert xs.shape == (B, T, n) and us.shape == (B, T, m)
    assert torch.isfinite(xs).all() and torch.isfinite(us).all()
    assert x_ref.grad is not None and torch.isfinite(x_ref.grad).all() and float(x_ref.grad.abs().max()) > 0.0
    assert (pol.ctrl.lamda_prev[:, T * n + 2 * T * m:] > 0).any()
