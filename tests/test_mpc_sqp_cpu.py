"""The host side of the one-call SQP rounds (include/dqp.h: dqp_mpc_linearize, dqp_mpc_sqp_*; qp_wrapper.MPC._sqp_on_device):
what is supported, the workspace formula of the header, the argument checks in front of any launch, and the predicate that
sends solve_nonlin there.  Needs only the built library: no test here touches a GPU."""
import ctypes

import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from diff_qp_mpc_amd import _lib
    return _lib.load()


def _dims(B, n, m, T, name, has_bounds=1, host=0):
    from diff_qp_mpc_amd import _lib
    dyn_id = _lib.DQP_DYN[name] if isinstance(name, str) else name
    return _lib.dqp_mpc_dims(B, n, m, T, has_bounds, dyn_id, host)


def _opts(batch=True, dt=0.05):
    from diff_qp_mpc_amd import _lib
    o = _lib.dqp_opts(1e-12, 1e-10, 20, 3, _lib.DQP_FLAG_BATCH_TERMINATION if batch else 0, 0)
    o.dyn_dt = dt
    return o


@pytest.mark.parametrize("n,m,T,name,kw,want,valid_model", [
    (3, 1, 10, "pendulum_dx", {}, 1, True),
    (4, 1, 5, "cartpole1l", {}, 1, True),
    (4, 1, 12, "cartpole1l", {}, 1, True),
    (12, 4, 6, "rexquadrotor", {}, 1, True),
    (2, 1, 5, "integrator", {}, 1, True),
    (3, 1, 10, 0, {}, 0, False),
    (3, 1, 10, 99, {}, 0, False),
    (3, 1, 10, "pendulum_dx", dict(has_bounds=0), 0, True),
    (3, 1, 10, "pendulum_dx", dict(host=4), 0, True),
    (4, 1, 10, "pendulum_dx", {}, 0, False),        # the model is (3, 1)
    (3, 2, 10, "pendulum_dx", {}, 0, False),
])
def test_supported_table(lib, n, m, T, name, kw, want, valid_model):
    d = _dims(6, n, m, T, name, **kw)
    assert lib.dqp_mpc_sqp_supported(ctypes.byref(d)) == want
    if valid_model:
        assert lib.dqp_mpc_sqp_supported(ctypes.byref(d)) == lib.dqp_mpc_qp_supported(ctypes.byref(d))
    if not want:
        assert lib.dqp_mpc_sqp_workspace_bytes(ctypes.byref(d), ctypes.byref(_opts())) == 0
    assert lib.dqp_mpc_sqp_supported(None) == 0


@pytest.mark.parametrize("batch", [True, False])
@pytest.mark.parametrize("B,n,m,T,name", [(6, 3, 1, 10, "pendulum_dx"), (5, 4, 1, 5, "cartpole1l"),
                                          (130, 4, 1, 12, "cartpole1l"), (3, 12, 4, 6, "rexquadrotor")])
def test_workspace_is_the_formula_of_the_header(lib, B, n, m, T, name, batch):
    d, o = _dims(B, n, m, T, name), _opts(batch)
    nt = n + m
    ev = lambda v: v + (v & 1)
    own = (ev((T - 1) * B * n * nt) + ev((T - 1) * B * n)           # F, f
           + ev(B * T * nt) + 4 * B * T * m + ev(B * T * n)         # tau, lam, slack, nu
           + 2 * ev(B)                                              # info, best_resid
           + 2 * ev(T * B * m) + ev(T * B * n)                      # du, u_new, x_new
           + 2 * ev(B) + ev((B + 63) // 64))                        # alpha, cost_new, the partial sums
    qp_ws = lib.dqp_mpc_qp_workspace_bytes(ctypes.byref(d))
    term = lib.dqp_mpc_qp_termination_bytes(ctypes.byref(d), ctypes.byref(o))
    assert qp_ws > 0 and (term > 0) == batch
    want = 8 * own + 16 * ((qp_ws + 15) // 16) + 16 * ((term + 15) // 16)
    assert lib.dqp_mpc_sqp_workspace_bytes(ctypes.byref(d), ctypes.byref(o)) == want
    assert lib.dqp_mpc_sqp_workspace_bytes(ctypes.byref(d), None) == 0
    d0 = _dims(0, n, m, T, name)
    assert lib.dqp_mpc_sqp_workspace_bytes(ctypes.byref(d0), ctypes.byref(o)) == 0


P = 64      # a non-null pointer that no call here dereferences: every call below returns in front of its launches


def _rounds(lib, d, o, ptrs=None, bounds="ok", decay=0.2, max_ls=10, begin=0, end=1):
    from diff_qp_mpc_amd import _lib
    names = ("C", "c", "x0", "x", "u", "keep_x", "keep_u", "keep_cost", "state", "workspace")
    p = dict.fromkeys(names, P)
    p.update(ptrs or {})
    b = None if bounds is None else ctypes.byref(_lib.dqp_al_bounds(*(bounds if bounds != "ok" else (P, P, 0, 0))))
    return lib.dqp_mpc_sqp_rounds(None if d is None else ctypes.byref(d), None if o is None else ctypes.byref(o),
                                  p["C"], p["c"], p["x0"], b, decay, max_ls, 1e-4, 1e-7, begin, end, p["x"], p["u"],
                                  p["keep_x"], p["keep_u"], p["keep_cost"], p["state"], p["workspace"], None)


def test_rounds_argument_checks_need_no_gpu(lib):
    OK, BAD, LARGE = 0, -1, -2
    d, o = _dims(6, 3, 1, 10, "pendulum_dx"), _opts()
    assert _rounds(lib, None, o) == BAD
    assert _rounds(lib, d, None) == BAD
    assert _rounds(lib, d, o, bounds=None) == BAD
    assert _rounds(lib, d, o, bounds=(P, P, 2, 0)) == BAD                   # not a layout of dqp_mpc_bounds
    assert _rounds(lib, d, o, bounds=(None, P, 0, 0)) == BAD
    assert _rounds(lib, d, o, bounds=(P, None, 0, 0)) == BAD
    for name in ("C", "c", "x0", "x", "u", "keep_x", "keep_u", "keep_cost", "state", "workspace"):
        assert _rounds(lib, d, o, {name: None}) == BAD, name
    assert _rounds(lib, d, o, begin=-1, end=1) == BAD
    assert _rounds(lib, d, o, begin=2, end=1) == BAD
    assert _rounds(lib, d, o, max_ls=0) == BAD
    assert _rounds(lib, d, _opts(dt=0.0)) == BAD
    # the model: unknown, none, of other sizes; no bounds; a host pair
    assert _rounds(lib, _dims(6, 3, 1, 10, 99), o) == BAD
    assert _rounds(lib, _dims(6, 3, 1, 10, 0), o) == BAD
    assert _rounds(lib, _dims(6, 4, 1, 10, "pendulum_dx"), o) == BAD
    assert _rounds(lib, _dims(6, 3, 1, 10, "pendulum_dx", has_bounds=0), o) == BAD
    assert _rounds(lib, _dims(6, 3, 1, 10, "pendulum_dx", host=4), o) == BAD
    assert _rounds(lib, _dims(6, 3, 1, 300000, "pendulum_dx"), o) == LARGE   # beyond the stage-wise kernels' horizon
    # an empty batch: nothing to do, whatever the arrays
    d0 = _dims(0, 3, 1, 10, "pendulum_dx")
    assert _rounds(lib, d0, o, dict.fromkeys(("C", "c", "x0", "x", "u", "keep_x", "keep_u", "keep_cost", "state", "workspace"))) == OK
    assert _rounds(lib, d0, o, bounds=(None, None, 0, 0)) == OK
    assert _rounds(lib, d0, o, bounds=(P, P, 2, 0)) == BAD                  # the layout is checked in front of the return


def test_linearize_argument_checks_need_no_gpu(lib):
    OK, BAD = 0, -1
    d = _dims(6, 3, 1, 10, "pendulum_dx")
    call = lambda dd, x=P, u=P, F=P, f=P: lib.dqp_mpc_linearize(None if dd is None else ctypes.byref(dd), 0.05, x, u, F, f, None)
    assert call(None) == BAD
    for k in ("x", "u", "F", "f"):
        assert call(d, **{k: None}) == BAD, k
    assert call(_dims(6, 3, 1, 10, 0)) == BAD
    assert call(_dims(6, 3, 1, 10, 99)) == BAD
    assert call(_dims(6, 4, 1, 10, "pendulum_dx")) == BAD
    assert call(_dims(6, 3, 1, 1, "pendulum_dx")) == BAD                    # T < 2: no knot to linearise at
    assert call(_dims(-1, 3, 1, 10, "pendulum_dx")) == BAD
    assert call(_dims(0, 3, 1, 10, "pendulum_dx"), None, None, None, None) == OK
    assert call(_dims(0, 3, 1, 10, "pendulum_dx", has_bounds=0), None, None, None, None) == OK     # reads no bounds


def test_version_stays(lib):
    assert lib.dqp_version() == 303


# ---------------------------------------------------------------------------------------------- MPC._sqp_on_device
class _Module:
    """a caller's dynamics module"""


def _mpc(n, m, T, B=4, **kw):
    from diff_qp_mpc_amd import qp_wrapper as qw
    mpc = qw.MPC(n, m, T, u_lower=-1.0, u_upper=1.0, n_batch=B, **kw)
    cost = qw.QuadCost(torch.zeros(T, B, n + m, n + m), torch.zeros(T, B, n + m))
    return mpc, cost


@pytest.mark.parametrize("case,want", [
    ("device model", True), ("flag off", False), ("LinDx", False), ("module", False), ("dense route", False),
    ("goal constraint", False), ("finite differences", False), ("wrapped jac", False), ("other true model", False),
    ("unbatched cost", False),
])
def test_sqp_on_device_table(lib, monkeypatch, case, want):
    from diff_qp_mpc_amd import qp_wrapper as qw
    from diff_qp_mpc_amd.dynamics import DeviceDynamics
    monkeypatch.setattr(qw, "ONE_CALL_SQP", case != "flag off")
    dyn = DeviceDynamics("pendulum_dx")
    n, kw = 3, {}
    if case == "dense route":
        n = 7                                   # (7, 1, T 10) has no kernels of its own
    if case == "goal constraint":
        kw = dict(add_goal_constraint=True)
    if case == "finite differences":
        kw = dict(grad_method=qw.GradMethods.FINITE_DIFF)
    mpc, cost = _mpc(n, 1, 10, **kw)
    dx, dx_jac = dyn, dyn.jac
    if case == "LinDx":
        dx, dx_jac = qw.LinDx(None, None), None
    if case == "module":
        dx, dx_jac = _Module(), dyn.jac
    if case == "wrapped jac":
        dx_jac = lambda x, u: dyn.jac(x, u)
    if case == "unbatched cost":
        cost = qw.QuadCost(cost.C[:, 0], cost.c[:, 0])
    mpc.dx_true = DeviceDynamics("pendulum_dx") if case == "other true model" else dx
    assert mpc._sqp_on_device(dx, dx_jac, cost) is want
    if want:        # tensors that are not on a GPU keep the Python loop (which then refuses them)
        assert mpc._sqp_on_device(dx, dx_jac, cost, torch.zeros(4, 3)) is False


def test_the_flag_is_off_and_checks_every_round_by_default():
    from diff_qp_mpc_amd import qp_wrapper as qw
    assert qw.ONE_CALL_SQP is False and qw.SQP_CHECK_EVERY == 1
