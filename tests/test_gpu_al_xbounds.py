"""State bounds (x_lower / x_upper) on the device AL_mpc paths (include/dqp.h: the `_xbounds` entry points), against the
numpy oracle over extended rows (tests/al_xbounds_oracle.py wraps the row builders of oracle/al_solve_oracle.py and
oracle/al_oracle.py; the algorithm stays the pinned one).

 1. one Newton step, merit-free, on the device model's own Jacobians          5. the integrator under a binding velocity box
 2. the outer update                                                               against the QP optimum (C oracle's PDIPM)
 3. AL_mpc.MPC cold and warm call, al_iter = 2                                 6. backward against the general torch path
 4. an inactive box: the `_bounds` step bit for bit, zero state multipliers    7. the Cholesky-failure route (LU fallback)
                                                                               8. GraphedMPC replay

Shapes: pendulum_euler (2, 1) T 5 B 6 (8-lane half rows, knots-at-once model evaluation); cartpole2l (6, 1) T 5 B 3 and
T 6 (the LDS-resident factor holds T (ROW + 1) 8 nt doubles <= 34 KB: T <= 5 at nt 7, ROW 14 -- csrc/dqp_al_banded.hip,
run_newton -- so T 5 keeps the factor in LDS and T 6 in memory); cartpole1l (4, 1) T 6 B 3; rexquadrotor (12, 4) T 4 B 3
(the 16-lane sweep, 12 of 16 lanes with state rows); integrator (2, 1) T 8 B 4.  B is never a multiple of the problems
per wavefront (4 or 8).
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import al_xbounds_oracle as xo
from oracle import al_oracle, al_solve_oracle as aso, dyn_host, oracle

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

SIZES = {"pendulum_euler": (2, 1), "cartpole1l": (4, 1), "cartpole2l": (6, 1), "rexquadrotor": (12, 4), "integrator": (2, 1)}
HOVER = 14.5            # the quadrotor's motor command around which the tests put its bounds (test_gpu_al.py:400,409)
# (robot, T, B, lane group): both groups of the half-row models; cartpole2l at 8 lanes on both sides of the LDS-factor
# threshold
STEP_CASES = [("pendulum_euler", 5, 6, 8), ("pendulum_euler", 5, 6, 16), ("cartpole2l", 5, 3, 8), ("cartpole2l", 6, 3, 8),
              ("cartpole2l", 5, 3, 16), ("cartpole1l", 6, 3, 8), ("cartpole1l", 6, 3, 16), ("rexquadrotor", 4, 3, 16)]
MPC_CASES = [("pendulum_euler", 5, 6), ("cartpole2l", 5, 3), ("cartpole1l", 6, 3), ("rexquadrotor", 4, 3)]
# half-width of the widest state box of the Newton-step inputs (states N(0, 0.5^2)): the box fades to 20 % along the
# horizon, so that a sample has knots with an active state row and knots with none (asserted in the test)
STEP_WIDTH = {"pendulum_euler": 1.2, "cartpole1l": 1.5, "cartpole2l": 1.6, "rexquadrotor": 2.0, "integrator": 1.2}


@pytest.fixture(autouse=True)
def _auto_lane_group():
    yield
    from diff_qp_mpc_amd import _lib
    _lib.load().dqp_al_lane_group(0)


def dev(a, grad=False):
    t = torch.tensor(np.asarray(a), dtype=torch.float64, device="cuda")
    return t.requires_grad_() if grad else t


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def varying(mid, width, B, T, k, seed=None):
    """(lo, hi) of shape (B, T, k): mid -+ width * scale[b] * fade[b, t] * (1 + 0.1 j), scale from 30 % to 100 % over the
    samples, the box fading to 20 % along the horizon on the even samples and growing from 20 % on the odd ones (the
    construction of test_gpu_al_bounds.py:60-72)"""
    scale = np.linspace(0.3, 1.0, B)[:, None, None]
    fade = np.tile(np.linspace(1.0, 0.2, T)[None, :, None], (B, 1, 1))
    fade[1::2] = fade[1::2, ::-1]
    w = width * scale * fade * (1.0 + 0.1 * np.arange(k))[None, None, :]
    return np.ascontiguousarray(mid - w), np.ascontiguousarray(mid + w)


def integrator_step(dt):
    def step(x, u):
        N = x.shape[0]
        v = x[:, 1] + u[:, 0] * dt
        Jx = np.tile(np.array([[1.0, dt], [0.0, 1.0]]), (N, 1, 1))
        Ju = np.tile(np.array([[dt * dt], [dt]]), (N, 1, 1))
        return np.stack((x[:, 0] + v * dt, v), 1), Jx, Ju
    return step


def host_step(robot, dt):
    """the oracle's dynamics on the host: numpy for the two closed-form models, the host build of the model templates
    (oracle/dyn_host.py) for the others"""
    if robot == "pendulum_euler":
        assert dt == al_oracle.DT
        return al_oracle.pendulum_step
    if robot == "integrator":
        return integrator_step(dt)
    step = dyn_host.stepper(robot, dt)
    assert step is not None, "the host build of the dynamics needs hipcc"
    return step


# ------------------------------------------------------------------ one Newton step's data (C ABI level)
def step_data(robot, T, B, seed):
    """the inputs of test_gpu_al_bounds.py::step_data with multipliers for the state rows too, a per-sample / per-knot
    control box and a per-sample / per-knot state box"""
    n, m = SIZES[robot]
    nt = n + m
    rng = np.random.default_rng(seed)
    xu = 0.5 * rng.standard_normal((B, T, nt))
    mid = HOVER if robot == "rexquadrotor" else 0.0
    if robot == "rexquadrotor":
        xu[..., n:] = HOVER + 0.3 * rng.standard_normal((B, T, m))
    d = dict(xu=xu, x0=xu[:, 0, :n] + 0.1 * rng.standard_normal((B, n)), Qd=rng.random((B, T, nt)) + 0.1,
             q=rng.standard_normal((B, T, nt)), lam=rng.standard_normal((B, xo.ncon_x(n, m, T))),
             rho=10.0 ** rng.integers(0, 3, (B, 1)).astype(np.float64))
    lo, hi = varying(mid, 1.5 if robot == "rexquadrotor" else 0.45, B, T, m)
    xl, xh = varying(0.0, STEP_WIDTH[robot], B, T, n)
    return d, lo, hi, xl, xh


def mixed_state_rows(res, n, m, T):
    """samples with an active state row at some knot and a knot without any"""
    sx = res[:, T * n + 2 * T * m:].reshape(res.shape[0], T, 2 * n)
    return (sx > 0).any(2).any(1) & (sx.max(2) <= 0).any(1)


def step_reference(d, lo, hi, xl, xh, step):
    """(update of the extended oracle, update without the state rows and their multipliers, res)"""
    B, T, nt = d["xu"].shape
    n = d["x0"].shape[1]
    m = nt - n
    ncu = T * n + 2 * T * m
    with xo.extended(xl, xh):
        res, resc, J, Jc = al_oracle.constraint_jacobian(d["xu"], d["x0"], lo, hi, step=step)
    grad = al_oracle.merit_grad(d["xu"], d["Qd"], d["q"], d["lam"], d["rho"], resc, J, Jc)
    upd, _, info = al_oracle.newton_update(Jc, d["Qd"].reshape(B, -1), d["rho"], grad)
    assert not info.any()
    res0, resc0, J0, Jc0 = al_oracle.constraint_jacobian(d["xu"], d["x0"], lo, hi, step=step)
    grad0 = al_oracle.merit_grad(d["xu"], d["Qd"], d["q"], d["lam"][:, :ncu], d["rho"], resc0, J0, Jc0)
    upd0 = al_oracle.newton_update(Jc0, d["Qd"].reshape(B, -1), d["rho"], grad0)[0]
    return upd, upd0, res


def check_step_inputs(robot, T, B, upd, upd0, res):
    """the conditions on the inputs, on the oracle alone: at least two samples with an active state row at some knots and
    none at others; ignoring the state rows moves the update by >= 100 x the tolerance somewhere"""
    n, m = SIZES[robot]
    assert mixed_state_rows(res, n, m, T).sum() >= 2, res[:, T * n + 2 * T * m:]
    assert (np.abs(upd0 - upd) >= 100.0 * (1e-10 + 1e-8 * np.abs(upd))).any()


class Call:
    """the `_xbounds` entry points of one problem at the C ABI (xbox = None: the `_bounds` twin, lam cut to its rows)"""

    def __init__(self, robot, T, B, d, lo, hi, xl, xh):
        from diff_qp_mpc_amd import _lib, al_utils
        from diff_qp_mpc_amd.dynamics import DeviceDynamics
        self.lib, self._lib = _lib.load(), _lib
        self.dyn = DeviceDynamics(robot)
        self.n, self.m, self.T, self.B = self.dyn.n_state, self.dyn.n_ctrl, T, B
        self.nt = self.n + self.m
        self.dims = _lib.dqp_al_mpc_dims(B, self.n, self.m, T)
        self.ncon = int(self.lib.dqp_al_ncon_xbounds(ctypes.byref(self.dims))) if xl is not None else T * self.n + 2 * T * self.m
        self.t = {k: dev(v).contiguous() for k, v in d.items()}
        self.t["rho"] = self.t["rho"].reshape(B).contiguous()
        self.t["lam"] = self.t["lam"][:, :self.ncon].contiguous()
        self.bd = al_utils.bounds_layout(dev(lo), dev(hi), B, T, self.m)
        self.xbd = None if xl is None else al_utils.bounds_layout(dev(xl), dev(xh), B, T, self.n)
        self.kw = dict(dtype=torch.float64, device="cuda")

    def _run(self, fn, outs):
        with self._lib.trace(256) as tr:
            rc = fn()
            torch.cuda.synchronize()
        assert rc == 0, rc
        return {k: v.cpu().numpy() for k, v in outs.items()}, [k for k, _ in tr.records]

    def _boxes(self):
        return (self.bd.ref(),) if self.xbd is None else (self.bd.ref(), self.xbd.ref())

    def _entry(self, name):
        return getattr(self.lib, name + ("_bounds" if self.xbd is None else "_xbounds"))

    def newton_step(self):
        t, B, T, nt = self.t, self.B, self.T, self.nt
        fac = torch.full((int(self.lib.dqp_al_banded_factor_bytes(ctypes.byref(self.dims), self.dyn.id)) // 8,), np.nan, **self.kw)
        o = dict(upd=torch.full((B, T, nt), np.nan, **self.kw), fac=fac, info=torch.full((B,), -7, dtype=torch.int32, device="cuda"))
        return self._run(lambda: self._entry("dqp_al_banded_newton_step")(
            ctypes.byref(self.dims), self.dyn.id, self.dyn.dt, P(t["xu"]), P(t["x0"]), P(t["Qd"]), P(t["q"]), P(t["lam"]),
            P(t["rho"]), *self._boxes(), P(o["upd"]), P(o["fac"]), P(o["info"]), None), o)

    def outer_update(self):
        t, B = self.t, self.B
        o = dict(lam_new=torch.full((B, self.ncon), np.nan, **self.kw), cost=torch.full((B,), np.nan, **self.kw),
                 resn=torch.full((B,), np.nan, **self.kw))
        return self._run(lambda: self._entry("dqp_al_outer_update")(
            ctypes.byref(self.dims), self.dyn.id, self.dyn.dt, P(t["xu"]), P(t["x0"]), P(t["lam"]), P(t["rho"]), P(t["Qd"]),
            P(t["q"]), *self._boxes(), P(o["lam_new"]), P(o["cost"]), P(o["resn"]), None), o)


def device_step_np(dyn):
    def step_np(x, u):
        xn, (Jx, Ju) = dyn.jac(dev(x), dev(u))
        return xn.cpu().numpy(), Jx.cpu().numpy(), Ju.cpu().numpy()
    return step_np


# ------------------------------------------------------------------ 1, 2
@pytest.mark.parametrize("robot,T,B,group", STEP_CASES)
def test_newton_step_and_outer_update_vs_extended_oracle(robot, T, B, group):
    """dqp_al_banded_newton_step_xbounds under per-sample, per-knot boxes against the extended oracle on the device
    model's own Jacobians (as test_gpu_al_bounds.py:487-501), rtol 1e-8 / atol 1e-10 (test_gpu_al.py:433);
    dqp_al_outer_update_xbounds against the extended residuals -- multipliers with the clamp of the new block, cost,
    |res_clamp| -- at rtol 1e-5 / atol 1e-7 (test_gpu_al.py:250)."""
    from diff_qp_mpc_amd import _lib
    n, m = SIZES[robot]
    assert _lib.load().dqp_al_lane_group(group) == 0
    d, lo, hi, xl, xh = step_data(robot, T, B, seed=3 * T + B)
    c = Call(robot, T, B, d, lo, hi, xl, xh)
    assert c.ncon == xo.ncon_x(n, m, T)
    step_np = device_step_np(c.dyn)
    upd_ref, upd_nobox, res = step_reference(d, lo, hi, xl, xh, step_np)
    check_step_inputs(robot, T, B, upd_ref, upd_nobox, res)
    out, names = c.newton_step()
    assert len(names) == 1 and "al_banded_newton_kernel<dqp::BoxBounds<" in names[0], names
    if n + m <= 8:          # the lane group, and the factor's home: LDS where T (ROW + 1) 8 nt doubles fit 34 KB
        lf = n + m >= 6 and group == 8 and T * (2 * n + m + 2) * 8 * (n + m) * 8 <= 34 * 1024
        assert ("%d, %s>" % (group, "true" if lf else "false")) in names[0].replace(" >", ">"), names
        assert (robot, T, group) not in (("cartpole2l", 5, 8),) or lf
        assert (robot, T, group) not in (("cartpole2l", 6, 8),) or not lf
    assert not out["info"].any()
    print("newton step: max |gpu - oracle| = %.3e" % float(np.abs(out["upd"].reshape(B, -1) - upd_ref).max()))
    np.testing.assert_allclose(out["upd"].reshape(B, -1), upd_ref, rtol=1e-8, atol=1e-10)
    # outer update
    out, names = c.outer_update()
    assert len(names) == 1 and "al_outer_kernel<dqp::BoxBounds<" in names[0], names
    with xo.extended(xl, xh):
        res, resc = aso.residuals(d["xu"], d["x0"], lo, hi, step_np)
    lam_new = d["lam"] + d["rho"] * res
    lam_new[:, T * n:] = np.maximum(lam_new[:, T * n:], 0.0)
    ncu = T * n + 2 * T * m
    assert (lam_new[:, ncu:] == 0).any() and (lam_new[:, ncu:] > 0).any()             # the clamp of the new block acts
    np.testing.assert_allclose(out["lam_new"], lam_new, rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(out["cost"], aso.compute_cost(d["xu"], d["Qd"], d["q"]), rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(out["resn"], np.linalg.norm(resc, axis=1), rtol=1e-5, atol=1e-7)


# ------------------------------------------------------------------ 4 (C ABI)
@pytest.mark.parametrize("robot,T,B,group", STEP_CASES)
def test_inactive_box_step_is_the_bounds_step_bit_for_bit(robot, T, B, group):
    """Both state bounds at -+1e30 and zero state multipliers: update and info of dqp_al_banded_newton_step_bounds to the
    last bit (adding exact zeros does not round: a difference means an existing term moved); the factor too."""
    from diff_qp_mpc_amd import _lib
    n, m = SIZES[robot]
    assert _lib.load().dqp_al_lane_group(group) == 0
    d, lo, hi, _, _ = step_data(robot, T, B, seed=5 * T + B)
    d["lam"][:, T * n + 2 * T * m:] = 0.0
    ref, ref_names = Call(robot, T, B, d, lo, hi, None, None).newton_step()
    assert "StridedBounds<" in ref_names[0] and not ref["info"].any() and np.isfinite(ref["upd"]).all()
    for shape in ((n,), (B, T, n)):
        out, names = Call(robot, T, B, d, lo, hi, np.full(shape, -1e30), np.full(shape, 1e30)).newton_step()
        assert "BoxBounds<" in names[0]
        for k in ("upd", "info", "fac"):
            assert out[k].tobytes() == ref[k].tobytes(), (k, shape)


# ------------------------------------------------------------------ AL_mpc.MPC problems (numpy)
def mpc_problem(robot, T, B, seed=0):
    """test_gpu_al_bounds.py::mpc_problem (x0, diagonal cost towards a straight line to the origin, the initial guess, a
    per-sample / per-knot control box) plus a per-sample / per-knot state box that the unconstrained trajectory leaves
    on some samples"""
    n, m = SIZES[robot]
    r = np.random.default_rng(seed)
    if robot == "pendulum_euler":
        x0 = np.stack([3.0 * (r.random(B) - 0.5), r.random(B) - 0.5], 1)
        Qd = np.broadcast_to(np.array([10.0, 1.0, 0.01]), (B, T, 3)).copy()
        mid, width = 0.0, 5.0
    else:
        x0 = r.uniform(-0.5, 0.5, (B, n))
        Qd = np.broadcast_to(np.concatenate([np.ones(n), 1e-3 * np.ones(m)]), (B, T, n + m)).copy()
        mid, width = (HOVER if robot == "rexquadrotor" else 0.0), 6.0
    x0[-1] *= 0.01                              # one sample next to the target: no bound becomes active
    x_ref = x0[:, None, :] * np.linspace(1.0, 0.0, T)[None, :, None]
    u_ref = np.full((B, T, m), mid)
    c = -(Qd * np.concatenate([x_ref, u_ref], -1))
    lo, hi = varying(mid, width, B, T, m)
    # the state box: around the reference line, 60 % of |x0| wide at least -- knot 0 (pinned) stays inside, later knots
    # are cut where the solution swings past the line
    w = 0.6 * np.abs(x0).max(1)[:, None, None] * np.linspace(1.0, 0.25, T)[None, :, None] * np.ones(n) + 0.02
    w[:, 0] = np.abs(x0).max(1)[:, None] + 0.05
    return dict(x0=x0, Qd=Qd, c=c, x_init=x_ref, u_init=u_ref, lo=lo, hi=hi, xl=np.ascontiguousarray(x_ref - w),
                xh=np.ascontiguousarray(x_ref + 0.3 * w), dt=0.05, width=width)


# x, u, multipliers of AL_mpc.MPC against the oracle: test_gpu_al_bounds.py::mpc_tol, i.e. test_gpu_al.py:248-260 (pendulum:
# x, u rtol 1e-4 / atol 1e-5, multipliers rtol 1e-5 / atol 1e-7 cold and 1e-6 warm) and test_gpu_al.py:290-301 (the others:
# x, u rtol 1e-4 / atol 1e-4, multipliers rtol 1e-5 / atol 1e-5); rho exact (:251, :293)
def mpc_tol(robot):
    if robot == "pendulum_euler":
        return dict(xu=(1e-4, 1e-5), lam=((1e-5, 1e-7), (1e-5, 1e-6)))
    return dict(xu=(1e-4, 1e-4), lam=((1e-5, 1e-5), (1e-5, 1e-5)))


def oracle_two_calls(robot, T, B, p, xl, xh, al_iter=2):
    """cold and warm call of the (extended, where xl is given) oracle"""
    n, m = SIZES[robot]
    step = host_step(robot, p["dt"])
    ncon = xo.ncon_x(n, m, T) if xl is not None else T * n + 2 * T * m
    lam0, rho0 = np.zeros((B, ncon)), np.ones((B, 1))

    def both():
        o1 = aso.al_solve(p["x_init"], p["u_init"], p["x0"], p["Qd"], p["c"], p["lo"], p["hi"], step, lam0, rho0, al_iter=al_iter)
        # AL_mpc.py:250-251: the warm call starts from the float32 solution of the first
        o2 = aso.al_solve(o1["x"].astype(np.float32).astype(np.float64), o1["u"].astype(np.float32).astype(np.float64), p["x0"],
                          p["Qd"], p["c"], p["lo"], p["hi"], step, o1["lam"], o1["rho"], al_iter=al_iter, history=o1["history"])
        return o1, o2
    if xl is None:
        return both()
    with xo.extended(xl, xh):
        return both()


_ORACLE = {}


def mpc_case(robot, T, B):
    """problem and the extended oracle's two calls, computed once per case and left unchanged"""
    key = (robot, T, B)
    if key not in _ORACLE:
        p = mpc_problem(robot, T, B)
        _ORACLE[key] = (p,) + oracle_two_calls(robot, T, B, p, p["xl"], p["xh"])
    return _ORACLE[key]


def check_mpc_inputs(robot, T, B, p, o1):
    """on the oracle alone: a state row is active (a positive state multiplier) on >= 2 samples, none on >= 1, and the
    solution without the state box is >= 100 x the tolerance away"""
    n, m = SIZES[robot]
    lx = o1["lam"][:, T * n + 2 * T * m:]
    assert ((lx > 0).any(1)).sum() >= 2 and ((lx == 0).all(1)).sum() >= 1, lx
    free = oracle_two_calls(robot, T, B, p, None, None)[0]
    rtol, atol = mpc_tol(robot)["xu"]
    assert (np.abs(free["xu"] - o1["xu"]) >= 100.0 * (atol + rtol * np.abs(o1["xu"]))).any()


def run_mpc(robot, T, B, p, xl, xh, grads=False, calls=2, al_iter=2):
    """AL_mpc.MPC on the device, `calls` calls -> list of (dict of numpy arrays, launch list)"""
    from diff_qp_mpc_amd import AL_mpc, _lib, al_utils
    from diff_qp_mpc_amd.dynamics import DeviceDynamics
    n, m = SIZES[robot]
    dyn = DeviceDynamics(robot, dt=p["dt"])
    x0 = dev(p["x0"])
    C = torch.diag_embed(dev(p["Qd"])).requires_grad_(grads)
    c = dev(p["c"], grad=grads)
    box = {} if xl is None else dict(x_lower=dev(xl), x_upper=dev(xh))
    ctrl = AL_mpc.MPC(n, m, T, u_lower=dev(p["lo"]), u_upper=dev(p["hi"]), n_batch=B, verbose=0, al_iter=al_iter,
                      solver_type="dense", dtype=torch.float64, eps=1e-5, exit_unconverged=False, backprop=False, **box)
    ctrl.reinitialize(x0, torch.ones(B, T, 1, device="cuda"))
    ctrl.x_init, ctrl.u_init = dev(p["x_init"]), dev(p["u_init"])
    outs = []
    for k in range(calls):
        with _lib.trace(1024) as tr:
            x, u = ctrl(x0, al_utils.QuadCost(C if k == 0 else C.detach(), c if k == 0 else c.detach()), dyn, dyn.jac)
        o = dict(x=x.detach().cpu().numpy(), u=u.detach().cpu().numpy(), lam=ctrl.lamda_prev.cpu().numpy(),
                 rho=ctrl.rho_prev.cpu().numpy())
        o["fail"] = any(bool(f.any()) for f in ctrl.fail_log)
        if k == 0 and grads:
            (x.double().sum() + 2.0 * u.double().sum()).backward()
            o.update(dC=C.grad.diagonal(dim1=-2, dim2=-1).cpu().numpy().copy(), dc=c.grad.cpu().numpy().copy())
        outs.append((o, [kn for kn, _ in tr.records]))
    return outs


# ------------------------------------------------------------------ 3
@pytest.mark.parametrize("robot,T,B", MPC_CASES)
def test_al_mpc_cold_and_warm_vs_extended_oracle(robot, T, B):
    """x, u, multipliers and rho after al_iter = 2, cold and warm call, against the extended al_solve; the launches are
    the BoxBounds<> instantiations and no Cholesky flag is set."""
    p, o1, o2 = mpc_case(robot, T, B)
    check_mpc_inputs(robot, T, B, p, o1)
    n, m = SIZES[robot]
    tol = mpc_tol(robot)
    got = run_mpc(robot, T, B, p, p["xl"], p["xh"])
    for g, names in got:
        assert not g["fail"]
        newton = [k for k in names if "al_banded_newton_kernel" in k]
        assert len(newton) == 8 and all("al_banded_newton_kernel<dqp::BoxBounds<" in k for k in newton), names
        assert any("al_start_xbounds_kernel" in k for k in names)
        assert sum("al_outer_kernel<dqp::BoxBounds<" in k for k in names) == 2, names
        assert all("BoxBounds<" in k for k in names if "al_ls_" in k) and any("al_ls_" in k for k in names), names
    for (g, _), o, lam_tol, call in zip(got, (o1, o2), tol["lam"], ("cold", "warm")):
        assert g["lam"].shape == (B, xo.ncon_x(n, m, T))
        for k in ("x", "u", "lam"):
            print(robot, call, k, "max |gpu - oracle| = %.3e" % float(np.abs(g[k] - o[k]).max()))
        for k in ("x", "u"):
            np.testing.assert_allclose(g[k], o[k], rtol=tol["xu"][0], atol=tol["xu"][1], err_msg=call + " " + k)
        np.testing.assert_allclose(g["lam"], o["lam"], rtol=lam_tol[0], atol=lam_tol[1], err_msg=call)
        np.testing.assert_array_equal(g["rho"], o["rho"], err_msg=call)


# ------------------------------------------------------------------ 4 (AL_mpc.MPC)
@pytest.mark.parametrize("robot,T,B", MPC_CASES)
def test_al_mpc_inactive_box_equals_the_call_without(robot, T, B):
    """Both state bounds at -+1e30: x, u and the multipliers of the old rows equal the call without state bounds within
    test 3's tolerance, the state multipliers are exactly 0, and the call without them launches no BoxBounds<> kernel."""
    n, m = SIZES[robot]
    p = mpc_problem(robot, T, B)
    ref = run_mpc(robot, T, B, p, None, None)
    got = run_mpc(robot, T, B, p, np.full(n, -1e30), np.full(n, 1e30))
    tol = mpc_tol(robot)
    ncu = T * n + 2 * T * m
    for (g, gn), (r, rn), lam_tol in zip(got, ref, tol["lam"]):
        assert not any("BoxBounds<" in k or "xbounds" in k for k in rn) and any("BoxBounds<" in k for k in gn)
        assert not g["fail"] and not r["fail"]
        assert (g["lam"][:, ncu:] == 0.0).all() and r["lam"].shape == (B, ncu)
        for k in ("x", "u"):
            np.testing.assert_allclose(g[k], r[k], rtol=tol["xu"][0], atol=tol["xu"][1])
        np.testing.assert_allclose(g["lam"][:, :ncu], r["lam"], rtol=lam_tol[0], atol=lam_tol[1])
        np.testing.assert_array_equal(g["rho"], r["rho"])


# ------------------------------------------------------------------ 5
INTEGRATOR = dict(T=8, B=4, dt=0.5, al_iter=6, margin=0.05)


def integrator_problem():
    """The double integrator from rest at the origin; the cost pulls the position to a target (0.8 .. 1.4 over the
    samples) that T - 1 = 7 steps of dt = 0.5 cannot reach inside the velocity box |v| <= 0.2 (0.7 at most).  The
    position is boxed loosely (-+ 2: no position leaves it); the control box (-+ 2) binds at the first knot of one sample
    without the state box and nowhere with it -- the control-box-only problem is the yardstick e_u."""
    T, B, dt = INTEGRATOR["T"], INTEGRATOR["B"], INTEGRATOR["dt"]
    n, m = 2, 1
    target = np.linspace(0.8, 1.4, B)
    x0 = np.zeros((B, n))
    Qd = np.broadcast_to(np.array([1.0, 0.1, 0.05]), (B, T, 3)).copy()
    ref = np.zeros((B, T, 3))
    ref[:, :, 0] = target[:, None]
    vmax = np.full((B, 1, 1), 0.2) * np.linspace(1.0, 0.8, B)[:, None, None]
    xh = np.concatenate((np.full((B, 1, 1), 2.0), vmax), 2)              # (B, 1, n): the packed per-sample layout
    return dict(x0=x0, Qd=Qd, c=-(Qd * ref), x_init=np.zeros((B, T, n)), u_init=np.zeros((B, T, m)), lo=np.full(m, -2.0),
                hi=np.full(m, 2.0), xl=np.ascontiguousarray(-xh), xh=np.ascontiguousarray(xh), dt=dt, vmax=vmax[:, 0, 0])


def integrator_qp(p, with_state_box):
    """the problem as a QP -- the dynamics are linear -- solved by the C oracle's dense PDIPM (tests/test_gpu_big.py,
    tests/test_gpu_ric.py): z = (x_t, u_t)_t, A z = b the dynamics and x_0 = x0, G z <= h the boxes"""
    T, B, dt = INTEGRATOR["T"], INTEGRATOR["B"], p["dt"]
    n, m, nt = 2, 1, 3
    nz = T * nt
    Ad, Bd = np.array([[1.0, dt], [0.0, 1.0]]), np.array([[dt * dt], [dt]])
    A = np.zeros((T * n, nz))
    for t in range(T - 1):
        A[t * n:(t + 1) * n, t * nt:t * nt + n] = -Ad
        A[t * n:(t + 1) * n, t * nt + n:(t + 1) * nt] = -Bd
        A[t * n:(t + 1) * n, (t + 1) * nt:(t + 1) * nt + n] = np.eye(n)
    A[(T - 1) * n:, :n] = np.eye(n)
    b = np.zeros((B, T * n))
    b[:, (T - 1) * n:] = p["x0"]
    rows, h = [], []
    for t in range(T):
        for sgn in (1.0, -1.0):
            g = np.zeros((m, nz))
            g[:, t * nt + n:(t + 1) * nt] = sgn * np.eye(m)
            rows.append(g)
            h.append(np.broadcast_to(p["hi"] if sgn > 0 else -p["lo"], (B, m)))
    if with_state_box:
        for t in range(T):
            for sgn in (1.0, -1.0):
                g = np.zeros((n, nz))
                g[:, t * nt:t * nt + n] = sgn * np.eye(n)
                rows.append(g)
                h.append(np.broadcast_to((p["xh"] if sgn > 0 else -p["xl"])[:, 0], (B, n)))
    G = np.concatenate(rows, 0)
    Q = np.stack([np.diag(p["Qd"][i].reshape(-1)) for i in range(B)])
    tile = lambda a: np.ascontiguousarray(np.broadcast_to(a, (B,) + a.shape))
    # guard: the reference's own get_step guard (batch_LU.py:204-210) -- without it a zero step direction on a row that
    # sits exactly on its bound is 0 / 0 and the iteration ends in NaN
    o = oracle.qp_forward(Q, p["c"].reshape(B, -1), tile(G), np.concatenate(h, 1), tile(A), b, maxIter=40, guard=True)
    assert (o["best_resid"] < 1e-9).all(), o["best_resid"]
    return o["zhat"].reshape(B, T, nt)


_INTEGRATOR = {}


def integrator_case():
    if not _INTEGRATOR:
        p = integrator_problem()
        _INTEGRATOR.update(p=p, z_box=integrator_qp(p, True), z_free=integrator_qp(p, False))
    return _INTEGRATOR["p"], _INTEGRATOR["z_box"], _INTEGRATOR["z_free"]


def check_integrator_inputs(p, z_box, z_free):
    """without the state box the optimum violates it by the stated margin; with it >= 1 knot sits on the velocity bound
    on every sample and none beyond it"""
    v_free, v_box = z_free[:, :, 1], z_box[:, :, 1]
    assert ((v_free.max(1) - p["vmax"]) >= INTEGRATOR["margin"]).all(), v_free.max(1) - p["vmax"]
    assert ((np.abs(v_box - p["vmax"][:, None]) <= 1e-6).sum(1) >= 1).all(), v_box
    assert (v_box <= p["vmax"][:, None] + 1e-6).all()


def test_integrator_velocity_box_against_the_qp_optimum():
    """al_iter = 6 on the integrator with a velocity box that binds: e_x = max |xu_AL - z_QP| with the state box against
    e_u, the same quantity of the control-box-only solve of the same problem against its own QP optimum.  Required:
    e_x <= 10 e_u (one rho decade for the extra active set)."""
    T, B = INTEGRATOR["T"], INTEGRATOR["B"]
    p, z_box, z_free = integrator_case()
    check_integrator_inputs(p, z_box, z_free)
    box = run_mpc("integrator", T, B, p, p["xl"], p["xh"], calls=1, al_iter=INTEGRATOR["al_iter"])[0]
    free = run_mpc("integrator", T, B, p, None, None, calls=1, al_iter=INTEGRATOR["al_iter"])[0]
    assert not box[0]["fail"] and not free[0]["fail"]
    assert any("al_banded_newton_kernel<dqp::BoxBounds<dqp::dyn::Integrator>" in k for k in box[1]), box[1]
    assert not any("BoxBounds<" in k for k in free[1])
    xu_box = np.concatenate((box[0]["x"], box[0]["u"]), 2).astype(np.float64)
    xu_free = np.concatenate((free[0]["x"], free[0]["u"]), 2).astype(np.float64)
    e_x, e_u = float(np.abs(xu_box - z_box).max()), float(np.abs(xu_free - z_free).max())
    viol = float((xu_free[:, :, 1].max(1) - p["vmax"]).min())
    print("integrator: e_x = %.3e (state box), e_u = %.3e (control box only), violation without the box >= %.3f" % (e_x, e_u, viol))
    assert viol >= INTEGRATOR["margin"]
    assert e_x <= 10.0 * e_u, (e_x, e_u)


# ------------------------------------------------------------------ 6
@pytest.mark.parametrize("robot,T,B", MPC_CASES)
def test_backward_vs_general_path(robot, T, B, monkeypatch):
    """Gradients of sum(x) + 2 sum(u) wrt C's diagonal and c under an active state box: the one-call device solve against
    the general torch path (ONE_CALL_SOLVE = False, FUSED_NEWTON_AL = False) on the same inputs; rtol 1e-4, atol 1e-6
    pendulum / 1e-5 others (test_gpu_al.py:253-254, :295-296)."""
    from diff_qp_mpc_amd import AL_mpc
    p, o1, _ = mpc_case(robot, T, B)
    n, m = SIZES[robot]
    assert (o1["lam"][:, T * n + 2 * T * m:] > 0).any()
    dev_out = run_mpc(robot, T, B, p, p["xl"], p["xh"], grads=True, calls=1)[0]
    monkeypatch.setattr(AL_mpc, "ONE_CALL_SOLVE", False)
    monkeypatch.setattr(AL_mpc, "FUSED_NEWTON_AL", False)
    gen_out = run_mpc(robot, T, B, p, p["xl"], p["xh"], grads=True, calls=1)[0]
    assert any("al_banded_newton_kernel<dqp::BoxBounds<" in k for k in dev_out[1])
    assert not any("al_banded" in k or "BoxBounds<" in k for k in gen_out[1]), gen_out[1]
    atol = 1e-6 if robot == "pendulum_euler" else 1e-5
    for k in ("dC", "dc"):
        print(robot, k, "max |device - general| = %.3e" % float(np.abs(dev_out[0][k] - gen_out[0][k]).max()))
    assert np.abs(dev_out[0]["dc"]).max() > 1e-3
    for k in ("dC", "dc"):
        np.testing.assert_allclose(dev_out[0][k], gen_out[0][k], rtol=1e-4, atol=atol, err_msg=k)


@pytest.mark.parametrize("robot,T,B", [("cartpole1l", 6, 3)])
def test_per_iteration_path_equals_the_one_call_path(robot, T, B, monkeypatch):
    """ONE_CALL_SOLVE = False: NewtonALDevice -> dqp_al_newton_solve_xbounds + dqp_al_outer_update_xbounds, the kernels of
    the one-call path launched per AL iteration -- the same bytes."""
    from diff_qp_mpc_amd import AL_mpc
    p, _, _ = mpc_case(robot, T, B)
    one = run_mpc(robot, T, B, p, p["xl"], p["xh"], grads=True, calls=1)[0]
    monkeypatch.setattr(AL_mpc, "ONE_CALL_SOLVE", False)
    per = run_mpc(robot, T, B, p, p["xl"], p["xh"], grads=True, calls=1)[0]
    assert sum("al_banded_newton_kernel<dqp::BoxBounds<" in k for k in per[1]) == 8 and not per[0]["fail"]
    assert not any("al_start" in k for k in per[1])
    for k in ("x", "u", "lam", "rho", "dC", "dc"):
        assert per[0][k].tobytes() == one[0][k].tobytes(), k


# ------------------------------------------------------------------ 7
def test_cholesky_failure_takes_the_lu_path_with_state_rows():
    """CFG5_cartpole2l_T5_b4 with one sample's control cost made strongly negative, as
    test_gpu_al.py::test_al_mpc_cholesky_failure_takes_the_lu_path forces it, plus a state box: the device path raises its
    flag, the call is redone on the general path with the state rows present, and agrees with the extended oracle's
    chol_fail branch on the healthy samples (x, u rtol 1e-4 / atol 1e-4, as there)."""
    from diff_qp_mpc_amd import AL_mpc, al_utils
    from diff_qp_mpc_amd.dynamics import DeviceDynamics
    g = dict(np.load(os.path.join(GOLDEN, "CFG5_cartpole2l_T5_b4.npz"), allow_pickle=False))
    B, T = g["in_Qd"].shape[:2]
    dyn = DeviceDynamics("cartpole2l", dt=float(g["dt"]))
    n, m = dyn.n_state, dyn.n_ctrl
    Qd = g["in_Qd"].copy()
    Qd[1, :, n:] = -5.0e3                                  # sample 1: negative control cost -> indefinite Hessian
    w = 0.5 * np.abs(g["in_x_init"]).max((0, 1)) + 0.05     # a box the trajectories leave
    xl, xh = -w, w
    step = host_step("cartpole2l", float(g["dt"]))
    lam0, rho0 = np.zeros((B, xo.ncon_x(n, m, T))), np.ones((B, 1))
    with xo.extended(xl, xh):
        o = aso.al_solve(g["in_x_init"], g["in_u_init"], g["in_x0"], Qd, g["in_c"], g["in_u_lower"], g["in_u_upper"], step,
                         lam0, rho0)
    assert o["chol_fail"]
    ok = np.array([0, 2, 3])
    assert (o["lam"][ok][:, T * n + 2 * T * m:] > 0).any()
    x0 = dev(g["in_x0"])
    ctrl = AL_mpc.MPC(n, m, T, u_lower=dev(g["in_u_lower"]), u_upper=dev(g["in_u_upper"]), n_batch=B, verbose=0,
                      solver_type="dense", dtype=torch.float64, eps=1e-5, exit_unconverged=False, backprop=False,
                      x_lower=dev(xl), x_upper=dev(xh))
    ctrl.reinitialize(x0, torch.ones(B, T, 1, device="cuda"))
    ctrl.x_init, ctrl.u_init = dev(g["in_x_init"]), dev(g["in_u_init"])
    from diff_qp_mpc_amd import _lib
    with _lib.trace(2048) as tr:
        x, u = ctrl(x0, al_utils.QuadCost(torch.diag_embed(dev(Qd)), dev(g["in_c"])), dyn, dyn.jac)
    names = [k for k, _ in tr.records]
    assert any(bool(f.any()) for f in ctrl.fail_log)                       # the device path flagged the failure ...
    assert any("al_banded_newton_kernel<dqp::BoxBounds<" in k for k in names)
    assert any("al_newton_kernel" in k for k in names)                     # ... and the general path redid the solve
    assert ctrl.lamda_prev.shape == (B, xo.ncon_x(n, m, T))
    assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(u).all())
    np.testing.assert_allclose(x.cpu().numpy()[ok], o["x"][ok], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(u.cpu().numpy()[ok], o["u"][ok], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(ctrl.lamda_prev.cpu().numpy()[ok], o["lam"][ok], rtol=1e-4, atol=1e-4)


# ------------------------------------------------------------------ 8
def test_graphed_mpc_with_a_state_box_replays_bitwise():
    """AL_mpc.GraphedMPC captures the cold call at pendulum_euler T = 5 with a (B, T, n) state box (the one-call path is
    enqueue-only with state bounds too); one replay equals the eager call bit for bit."""
    from diff_qp_mpc_amd import AL_mpc, al_utils
    from diff_qp_mpc_amd.dynamics import DeviceDynamics
    robot, T, B = "pendulum_euler", 5, 6
    n, m = SIZES[robot]
    p = mpc_problem(robot, T, B)
    assert p["xl"].shape == (B, T, n)
    dyn = DeviceDynamics(robot, dt=p["dt"])
    lo, hi, xl, xh = dev(p["lo"]), dev(p["hi"]), dev(p["xl"]), dev(p["xh"])
    x0, x_ref, u_ref = dev(p["x0"]), dev(p["x_init"]), dev(p["u_init"])

    def make():
        return AL_mpc.MPC(n, m, T, u_lower=lo, u_upper=hi, n_batch=B, verbose=0, solver_type="dense", dtype=torch.float64,
                          eps=1e-5, exit_unconverged=False, backprop=False, x_lower=xl, x_upper=xh)

    def inputs():
        return torch.diag_embed(dev(p["Qd"])).requires_grad_(), dev(p["c"], grad=True)

    C, c = inputs()
    ctrl = make()
    ctrl.reinitialize(x0, torch.ones(B, T, 1, device="cuda"))
    ctrl.x_init, ctrl.u_init = x_ref, u_ref
    xe, ue = ctrl(x0, al_utils.QuadCost(C, c), dyn, dyn.jac)
    gCe, gce = torch.autograd.grad(xe.double().sum() + 2.0 * ue.double().sum(), (C, c))
    assert bool((ctrl.lamda_prev[:, T * n + 2 * T * m:] > 0).any())           # a state row is active in the captured problem
    C, c = inputs()
    ctrl = make()
    ctrl.mask = torch.ones(B, T, 1, device="cuda")
    g = AL_mpc.GraphedMPC(ctrl, (x0, C, c), dyn, x_init=x_ref, u_init=u_ref)
    x, u = g(x0, C, c)
    gC, gc = torch.autograd.grad(x.double().sum() + 2.0 * u.double().sum(), (C, c))
    for a, b in zip((x, u, gC, gc), (xe.detach(), ue.detach(), gCe, gce)):
        assert torch.equal(a, b)
    assert not g.failed()
