"""dqp_al_mpc_solve_fused (csrc/dqp_al_fused.hip): AL_mpc.MPC.al_solve for a registered device model as ONE kernel
launch -- through the C ABI and through the AL_mpc.PERSISTENT_SOLVE switch.

 1. the reference's goldens with the switch on (cold call with gradients, warm-started second call), at the tolerances
    tests/test_gpu_al.py uses for the same fixtures
 2. against the multi-launch dqp_al_mpc_solve on the same inputs: the same arithmetic up to summation order
 3. an indefinite Newton system: the same failure flags, and AL_mpc.MPC then takes the LU path
 4. support and argument checks
 5. hipGraph capture, and ONE library launch for the forward solve
"""
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NEWTON_STEPS = 4
ROBOTS = {"pendulum1l": 1, "cartpole1l": 2, "cartpole2l": 3, "pendulum_euler": 4, "pendulum_dx": 5, "rexquadrotor": 6}


def load(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False))


def dev(a, grad=False):
    t = torch.tensor(np.asarray(a), dtype=torch.float64, device="cuda")
    return t.requires_grad_() if grad else t


@pytest.fixture
def switch_on(monkeypatch):
    from diff_qp_mpc_amd import AL_mpc
    monkeypatch.setattr(AL_mpc, "PERSISTENT_SOLVE", True)
    monkeypatch.setattr(AL_mpc, "PERSISTENT_SOLVE_MAX_BATCH", 1 << 20)
    return AL_mpc


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def solve(entry, dyn, T, al_iter, x_init, u_init, x0, Qd, q, lo, hi, lam, rho, prev=None, newton_steps=NEWTON_STEPS):
    """one call of dqp_al_mpc_solve / dqp_al_mpc_solve_fused -> dict of its outputs (and the workspace)"""
    from diff_qp_mpc_amd import _lib
    lib = _lib.load()
    B, n, m = x0.shape[0], dyn.n_state, dyn.n_ctrl
    nt, ncon = n + m, T * n + 2 * T * m
    dims = _lib.dqp_al_mpc_dims(B, n, m, T)
    kw = dict(dtype=torch.float64, device="cuda")
    o = dict(xu=torch.full((B, T, nt), np.nan, **kw), hist_cost=torch.full((al_iter + 1, B), np.nan, **kw),
             hist_lam=torch.full((al_iter + 1, B, ncon), np.nan, **kw), hist_rho=torch.full((al_iter + 1, B), np.nan, **kw),
             res_norm=torch.full((B,), np.nan, **kw),
             factor=torch.zeros(int(lib.dqp_al_banded_factor_bytes(ctypes.byref(dims), dyn.id)) // 8, **kw),
             status=torch.full((B,), np.nan, **kw), fail=torch.full((al_iter,), 7, dtype=torch.int32, device="cuda"),
             ws=torch.zeros(int(lib.dqp_al_mpc_solve_bytes(ctypes.byref(dims))) // 8 + 1, **kw))
    pc, pl, pr = prev if prev is not None else (None, None, None)
    keep = [t.contiguous() for t in (x_init, u_init, x0, Qd, q, lo, hi, lam, rho)]
    rc = getattr(lib, entry)(ctypes.byref(dims), dyn.id, dyn.dt, al_iter, newton_steps, *[_ptr(t) for t in keep],
                             _ptr(pc), _ptr(pl), _ptr(pr), 0 if prev is None else pc.shape[0], _ptr(o["xu"]),
                             _ptr(o["hist_cost"]), _ptr(o["hist_lam"]), _ptr(o["hist_rho"]), _ptr(o["res_norm"]),
                             _ptr(o["factor"]), _ptr(o["status"]), _ptr(o["fail"]), _ptr(o["ws"]),
                             ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, (entry, rc)
    torch.cuda.synchronize()
    o["dims"] = dims
    return o


def problem_np(robot, n, m, T, B, seed):
    """A tracking problem that two AL iterations of four Newton steps leave far from converged (a start well off the
    reference, control bounds that bind): every line search then has a clear winner among its candidates."""
    r = np.random.default_rng(seed)
    x0 = r.uniform(-1.0, 1.0, (B, n))
    if robot == "pendulum_dx":                      # state (cos th, sin th, thdot)
        th = r.uniform(-1.0, 1.0, B)
        x0 = np.stack([np.cos(th), np.sin(th), r.uniform(-1.0, 1.0, B)], 1)
    x_ref = x0[:, None, :] * np.linspace(1.0, 0.0, T)[None, :, None]
    Qd = np.concatenate([r.uniform(0.5, 2.0, (B, T, n)), r.uniform(1e-3, 1e-2, (B, T, m))], 2)
    ref = np.concatenate([x_ref, np.zeros((B, T, m))], 2)
    q = -Qd * ref + 0.05 * r.standard_normal((B, T, n + m))
    x_init = x_ref + 0.05 * r.standard_normal((B, T, n))
    u_init = 0.5 * r.standard_normal((B, T, m))
    lo, hi = np.full(m, -1.5), np.full(m, 1.5)
    lam = np.zeros((B, T * n + 2 * T * m))
    rho = np.ones(B)
    return [x_init, u_init, x0, Qd, q, lo, hi, lam, rho]


def problem(robot, T, B, seed):
    from diff_qp_mpc_amd.dynamics import DeviceDynamics
    dyn = DeviceDynamics(robot)
    return dyn, [dev(a) for a in problem_np(robot, dyn.n_state, dyn.n_ctrl, T, B, seed)]


def last_merits_distinct(dyn, multi, T, B):
    """The 20 candidate merits of the multi-launch path's LAST line search (its workspace: the update (B, nz), then the
    merits (20, B) where the selection ran as its own launch, which it does at these batch sizes): no two of a sample
    within 1e-12 relative.  Where they are, the update is about zero and the argmin / the acceptance is decided by the
    summation order, which the two paths do not share."""
    nz = T * (dyn.n_state + dyn.n_ctrl)
    merit = multi["ws"][B * nz:B * nz + 20 * B].reshape(20, B).cpu().numpy()
    if not np.isfinite(merit).all():
        return False
    m = np.sort(merit, axis=0)
    return bool((np.diff(m, axis=0) > 1e-12 * np.abs(m[1:])).all())


def inputs(robot, T, B, al_iter, n_prev, seed):
    dyn, ins = problem(robot, T, B, seed)
    prev = None
    if n_prev:
        # a previous call's history (n_prev = 3 rows); then the next control step of a closed loop: a new measurement x0
        # and the previous solution, disturbed, as the start -- so that this call, too, is far from converged
        first = solve("dqp_al_mpc_solve", dyn, T, n_prev - 1, *ins)
        prev = (first["hist_cost"], first["hist_lam"], first["hist_rho"])
        n = dyn.n_state
        r = np.random.default_rng(seed + 1)
        ins[2] = ins[2] + dev(0.3 * r.standard_normal(tuple(ins[2].shape)))
        if robot == "pendulum_dx":
            ins[2][:, :2] /= ins[2][:, :2].norm(dim=1, keepdim=True)
        ins[0] = first["xu"][:, :, :n].contiguous() + dev(0.05 * r.standard_normal((B, T, n)))
        ins[1] = first["xu"][:, :, n:].contiguous() + dev(0.2 * r.standard_normal((B, T, dyn.n_ctrl)))
        ins[7], ins[8] = first["hist_lam"][-1].contiguous(), first["hist_rho"][-1].contiguous()
    return dyn, ins, prev


def both(robot, T, B, al_iter, n_prev, seed, newton_steps=NEWTON_STEPS):
    """-> (dyn, multi-launch outputs, fused outputs) on the first of the seeds seed, seed + 1000, ... at which the
    multi-launch path itself has no near-tie among its last candidates (the choice looks at that path only)"""
    for k in range(16):
        dyn, ins, prev = inputs(robot, T, B, al_iter, n_prev, seed + 1000 * k)
        multi = solve("dqp_al_mpc_solve", dyn, T, al_iter, *ins, prev=prev, newton_steps=newton_steps)
        if last_merits_distinct(dyn, multi, T, B):
            return dyn, multi, solve("dqp_al_mpc_solve_fused", dyn, T, al_iter, *ins, prev=prev, newton_steps=newton_steps)
    raise AssertionError("no seed without a near-tie in the multi-launch line search")


def banded_solve(dyn, o, rhs):
    from diff_qp_mpc_amd import _lib
    out = torch.empty_like(rhs)
    rc = _lib.load().dqp_al_banded_solve(ctypes.byref(o["dims"]), dyn.id, _ptr(o["factor"]), _ptr(rhs), _ptr(out),
                                         ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    return out.cpu().numpy()


def compare(dyn, multi, fused, T, B):
    """The two paths run the same arithmetic up to summation order: iterates, costs and multipliers to rtol 1e-8 / atol
    1e-8 (two orders above the project's "same iterates to 1e-10" for banded against dense), penalties, status and
    failure flags exact, the kept factor through dqp_al_banded_solve of a random right-hand side (rtol 1e-8, atol 1e-10)."""
    for k in ("xu", "hist_cost", "hist_lam", "res_norm"):
        np.testing.assert_allclose(fused[k].cpu().numpy(), multi[k].cpu().numpy(), rtol=1e-8, atol=1e-8, err_msg=k)
    for k in ("hist_rho", "status", "fail"):
        assert torch.equal(fused[k], multi[k]), k
    rhs = dev(np.random.default_rng(11).standard_normal((B, T, dyn.n_state + dyn.n_ctrl)))
    np.testing.assert_allclose(banded_solve(dyn, fused, rhs), banded_solve(dyn, multi, rhs), rtol=1e-8, atol=1e-10)


# the smallest shapes at each edge: T = 2 (the minimum), cartpole-2 at T = 5 (the LDS-factor regime of the multi-launch
# kernel), T = 17 and 32 (the knot loops run past one 8- and 16-lane group; 32 is the top of the range).  Four Newton
# steps per AL iteration as AL_mpc.MPC runs them -- except at T = 2, a nearly quadratic problem in four unknowns that
# the second or third step solves to rounding (oracle/al_solve_oracle.py on these inputs: all 20 candidate merits of the
# later steps within 1e-14): there one Newton step per AL iteration, so that every line search has a winner
@pytest.mark.parametrize("n_prev", [0, 3])
@pytest.mark.parametrize("al_iter", [1, 2])
@pytest.mark.parametrize("B", [1, 3, 9])
@pytest.mark.parametrize("robot,T,newton_steps", [("pendulum1l", 2, 1), ("cartpole2l", 5, 4), ("cartpole1l", 17, 4), ("cartpole1l", 32, 4)])
def test_fused_solve_matches_multi_launch(robot, T, newton_steps, B, al_iter, n_prev):
    dyn, multi, fused = both(robot, T, B, al_iter, n_prev, seed=100 * T + B, newton_steps=newton_steps)
    assert not bool(multi["fail"].any())
    compare(dyn, multi, fused, T, B)


def test_fused_solve_matches_multi_launch_pendulum_dx():
    dyn, multi, fused = both("pendulum_dx", 10, 3, 2, 0, seed=5)
    compare(dyn, multi, fused, 10, 3)


def _mpc(AL_mpc, dyn, g, B, T, C, c, x_init=True):
    ctrl = AL_mpc.MPC(dyn.n_state, dyn.n_ctrl, T, u_lower=dev(g["in_u_lower"]), u_upper=dev(g["in_u_upper"]), n_batch=B,
                      verbose=0, solver_type="dense", dtype=torch.float64, eps=1e-5, exit_unconverged=False, backprop=False)
    ctrl.reinitialize(dev(g["in_x0"]), torch.ones(B, T, 1, device="cuda"))
    if x_init:
        ctrl.x_init = dev(g["in_x_init"])
    ctrl.u_init = dev(g["in_u_init"])
    return ctrl


def _fused_launches(records):
    return [k for k, _ in records if "al_solve_fused_kernel" in k]


@pytest.mark.parametrize("name,robot,atol", [("AL_pendulum_T5_b8", "pendulum_euler", 1e-5), ("AL_pendulum_T10_b6", "pendulum_euler", 1e-5),
                                             ("CFG3_cartpole1l_T20_b4", "cartpole1l", 1e-4), ("CFG5_cartpole2l_T5_b4", "cartpole2l", 1e-4)])
def test_switch_on_vs_reference(name, robot, atol, switch_on):
    """The reference's AL_mpc.MPC goldens with PERSISTENT_SOLVE on: cold call with gradients, then the warm-started
    call, at the tolerances of tests/test_gpu_al.py for the same fixtures (x, u rtol 1e-4 with atol 1e-5 pendulum / 1e-4
    cartpoles; multipliers rtol 1e-5; rho exact; dC, dc rtol 1e-4) -- the start, the warm start, both AL iterations, the
    outer update and the kept factor (through backward)."""
    from diff_qp_mpc_amd import _lib, al_utils
    from diff_qp_mpc_amd.dynamics import DeviceDynamics
    AL_mpc = switch_on
    g = load(name)
    B, T = g["in_Qd"].shape[:2]
    pend = robot == "pendulum_euler"
    dyn = DeviceDynamics(robot, dt=0.05 if pend else float(g["dt"]))
    lam_atol, grad_atol = ((1e-7, 1e-6), 1e-6) if pend else ((1e-5, 1e-5), 1e-5)
    C = torch.diag_embed(dev(g["in_Qd"])).requires_grad_()
    c = dev(g["in_c"], grad=True)
    ctrl = _mpc(AL_mpc, dyn, g, B, T, C, c, x_init=not pend)
    x0 = dev(g["in_x0"])
    with _lib.trace() as tr:
        x, u = ctrl(x0, al_utils.QuadCost(C, c), dyn, dyn.jac)
    assert len(_fused_launches(tr.records)) == 1 and not any("al_banded_newton_kernel" in k for k, _ in tr.records)
    assert x.dtype == torch.float32 and u.dtype == torch.float32
    np.testing.assert_allclose(x.detach().cpu().numpy(), g["x1"], rtol=1e-4, atol=atol)
    np.testing.assert_allclose(u.detach().cpu().numpy(), g["u1"], rtol=1e-4, atol=atol)
    np.testing.assert_allclose(ctrl.lamda_prev.cpu().numpy(), g["lam1"], rtol=1e-5, atol=lam_atol[0])
    np.testing.assert_allclose(ctrl.rho_prev.cpu().numpy(), g["rho1"], rtol=0, atol=0)
    (x.double().sum() + 2.0 * u.double().sum()).backward()
    np.testing.assert_allclose(C.grad.diagonal(dim1=-2, dim2=-1).cpu().numpy(), g["dC1"], rtol=1e-4, atol=grad_atol)
    np.testing.assert_allclose(c.grad.cpu().numpy(), g["dc1"], rtol=1e-4, atol=grad_atol)
    x2, u2 = ctrl(x0, al_utils.QuadCost(C.detach(), c.detach()), dyn, dyn.jac)
    np.testing.assert_allclose(x2.cpu().numpy(), g["x2"], rtol=1e-4, atol=atol)
    np.testing.assert_allclose(u2.cpu().numpy(), g["u2"], rtol=1e-4, atol=atol)
    np.testing.assert_allclose(ctrl.lamda_prev.cpu().numpy(), g["lam2"], rtol=1e-5, atol=lam_atol[1])
    np.testing.assert_allclose(ctrl.rho_prev.cpu().numpy(), g["rho2"], rtol=0, atol=0)


def test_switch_respects_the_batch_threshold(switch_on, monkeypatch):
    """B above PERSISTENT_SOLVE_MAX_BATCH, or the switch off: the multi-launch path serves"""
    from diff_qp_mpc_amd import _lib, al_utils
    from diff_qp_mpc_amd.dynamics import DeviceDynamics
    AL_mpc = switch_on
    g = load("CFG5_cartpole2l_T5_b4")
    B, T = g["in_Qd"].shape[:2]
    dyn = DeviceDynamics("cartpole2l", dt=float(g["dt"]))
    C, c = torch.diag_embed(dev(g["in_Qd"])), dev(g["in_c"])
    for max_batch, on, want in ((B - 1, True, 0), (B, True, 1), (B, False, 0)):
        monkeypatch.setattr(AL_mpc, "PERSISTENT_SOLVE_MAX_BATCH", max_batch)
        monkeypatch.setattr(AL_mpc, "PERSISTENT_SOLVE", on)
        ctrl = _mpc(AL_mpc, dyn, g, B, T, C, c)
        with _lib.trace() as tr:
            ctrl(dev(g["in_x0"]), al_utils.QuadCost(C, c), dyn, dyn.jac)
        assert len(_fused_launches(tr.records)) == want


def test_cholesky_failure_flags_and_lu_path(switch_on):
    """The input construction of test_al_mpc_cholesky_failure_takes_the_lu_path (one sample's control cost strongly
    negative: an indefinite Newton system, an ordinary flagged result): the fused call sets the same failure flags as the
    multi-launch call, and AL_mpc.MPC with the switch on then takes the LU path and matches oracle/al_solve_oracle.py
    as that test does (x, u rtol 1e-4 / atol 1e-4; gradients of the healthy samples rtol 1e-3 / atol 1e-5)."""
    from diff_qp_mpc_amd import al_utils
    from diff_qp_mpc_amd.dynamics import DeviceDynamics
    from oracle import al_solve_oracle as aso, dyn_host
    AL_mpc = switch_on
    name, robot = "CFG5_cartpole2l_T5_b4", "cartpole2l"
    g = load(name)
    B, T = g["in_Qd"].shape[:2]
    dyn = DeviceDynamics(robot, dt=float(g["dt"]))
    nx, nu = dyn.n_state, dyn.n_ctrl
    Qd = g["in_Qd"].copy()
    Qd[1, :, nx:] = -5.0e3
    lam0, rho0 = np.zeros((B, T * nx + 2 * T * nu)), np.ones((B, 1))
    ins = [dev(a) for a in (g["in_x_init"], g["in_u_init"], g["in_x0"], Qd, g["in_c"], g["in_u_lower"].reshape(-1),
                            g["in_u_upper"].reshape(-1), lam0, rho0.reshape(B))]
    multi = solve("dqp_al_mpc_solve", dyn, T, 2, *ins)
    fused = solve("dqp_al_mpc_solve_fused", dyn, T, 2, *ins)
    assert bool(multi["fail"].any())
    assert torch.equal(fused["fail"], multi["fail"])
    step = dyn_host.stepper(robot, float(g["dt"]))
    if step is None:
        pytest.skip("hipcc not available for the host build of the dynamics")
    o = aso.al_solve(g["in_x_init"], g["in_u_init"], g["in_x0"], Qd, g["in_c"], g["in_u_lower"], g["in_u_upper"], step,
                     lam0, rho0)
    assert o["chol_fail"]
    C = torch.diag_embed(dev(Qd)).requires_grad_()
    c = dev(g["in_c"], grad=True)
    ctrl = _mpc(AL_mpc, dyn, g, B, T, C, c)
    x, u = ctrl(dev(g["in_x0"]), al_utils.QuadCost(C, c), dyn, dyn.jac)
    assert bool(ctrl.fail_log[-1].any())
    ok = np.array([0, 2, 3])
    np.testing.assert_allclose(x.detach().cpu().numpy()[ok], o["x"][ok], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(u.detach().cpu().numpy()[ok], o["u"][ok], rtol=1e-4, atol=1e-4)
    assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(u).all())
    (x.double().sum() + 2.0 * u.double().sum()).backward()
    gxu = np.concatenate((np.ones((B, T, nx)), 2.0 * np.ones((B, T, nu))), 2)
    dQ, dq = aso.backward(o["L"], o["xu"], gxu, chol_fail=True)
    np.testing.assert_allclose(C.grad.diagonal(dim1=-2, dim2=-1).cpu().numpy()[ok], dQ[ok], rtol=1e-3, atol=1e-5)
    np.testing.assert_allclose(c.grad.cpu().numpy()[ok], dq[ok], rtol=1e-3, atol=1e-5)


def test_support_and_argument_checks():
    from diff_qp_mpc_amd import _lib
    lib = _lib.load()
    sizes = {"pendulum1l": (2, 1), "cartpole1l": (4, 1), "cartpole2l": (6, 1), "pendulum_euler": (2, 1), "pendulum_dx": (3, 1),
             "rexquadrotor": (12, 4)}

    def supported(robot, T, B=4):
        d = _lib.dqp_al_mpc_dims(B, *sizes[robot], T)
        return lib.dqp_al_mpc_solve_fused_supported(ctypes.byref(d), ROBOTS[robot])

    for robot in sizes:
        for T in (2, 32):
            assert supported(robot, T) == (0 if robot == "rexquadrotor" else 1)
        assert supported(robot, 33) == 0 and supported(robot, 1) == 0

    def call(robot, T, B, al_iter=2):
        n, m = sizes[robot]
        Bb = max(B, 1)
        kw = dict(dtype=torch.float64, device="cuda")
        ncon = max(T, 1) * (n + 2 * m)
        buf = lambda *s: torch.full(s, 3.0, **kw)
        outs = [buf(Bb, max(T, 1), n + m), buf(al_iter + 1, Bb), buf(al_iter + 1, Bb, ncon), buf(al_iter + 1, Bb), buf(Bb),
                buf(Bb * max(T, 1) * (n + m) * (2 * n + m + 1)), buf(Bb)]
        fail = torch.full((al_iter,), 7, dtype=torch.int32, device="cuda")
        ws = buf(Bb * (max(T, 1) * (n + m) + 32) + 8)
        ins = [buf(Bb, max(T, 1), n), buf(Bb, max(T, 1), m), buf(Bb, n), buf(Bb, max(T, 1), n + m), buf(Bb, max(T, 1), n + m),
               buf(m), buf(m), buf(Bb, ncon), buf(Bb)]
        d = _lib.dqp_al_mpc_dims(B, n, m, T)
        rc = lib.dqp_al_mpc_solve_fused(ctypes.byref(d), ROBOTS[robot], 0.05, al_iter, NEWTON_STEPS, *[_ptr(t) for t in ins],
                                        None, None, None, 0, *[_ptr(t) for t in outs], _ptr(fail), _ptr(ws), None)
        torch.cuda.synchronize()
        return rc, outs, fail

    assert call("rexquadrotor", 6, 4)[0] == -2                     # DQP_ERR_TOO_LARGE
    assert call("cartpole1l", 33, 4)[0] == -2
    assert call("cartpole1l", 1, 4)[0] == -1                       # DQP_ERR_BAD_ARG
    assert call("cartpole1l", 5, 4, al_iter=257)[0] == -1
    assert call("cartpole1l", 5, -1)[0] == -1
    rc, outs, fail = call("cartpole1l", 5, 0)                      # nbatch = 0: DQP_OK, nothing touched
    assert rc == 0
    assert all(bool((t == 3.0).all()) for t in outs) and bool((fail == 7).all())


def test_graphed_mpc_replay_bitwise_equal_to_eager_fused(switch_on):
    """With the switch on, AL_mpc.GraphedMPC (cartpole-2, T = 5, B = 8) replays bit for bit what the eager fused call
    computes -- x, u and the gradients -- on the captured batch and on a second one; and the forward solve of an eager call
    is ONE library launch."""
    from diff_qp_mpc_amd import _lib, al_utils
    from diff_qp_mpc_amd.dynamics import DeviceDynamics
    AL_mpc = switch_on
    robot, T, B = "cartpole2l", 5, 8
    dyn = DeviceDynamics(robot)
    nx, nu = dyn.n_state, dyn.n_ctrl
    lo, hi = dev(np.full(nu, -250.0)), dev(np.full(nu, 250.0))
    Qd = dev(np.concatenate([np.ones(nx), 1e-3 * np.ones(nu)])).repeat(B, T, 1)

    def batch(seed):
        r = np.random.default_rng(seed)
        x0 = dev(r.uniform(-0.5, 0.5, (B, nx)))
        x_ref = x0[:, None, :] * torch.linspace(1.0, 0.0, T, dtype=torch.float64, device="cuda")[None, :, None]
        u_ref = ((lo + hi) / 2).repeat(B, T, 1)
        C = torch.diag_embed(Qd).requires_grad_()
        c = (-(Qd * torch.cat([x_ref, u_ref], -1))).clone().requires_grad_()
        return x0, x_ref, u_ref, C, c

    def make():
        return AL_mpc.MPC(nx, nu, T, u_lower=lo, u_upper=hi, n_batch=B, verbose=0, solver_type="dense", dtype=torch.float64,
                          eps=1e-5, exit_unconverged=False, backprop=False)

    def eager(x0, x_ref, u_ref, C, c, trace=False):
        ctrl = make()
        ctrl.reinitialize(x0, torch.ones(B, T, 1, device="cuda"))
        ctrl.x_init, ctrl.u_init = x_ref, u_ref
        if trace:
            with _lib.trace() as tr:
                x, u = ctrl(x0, al_utils.QuadCost(C, c), dyn, dyn.jac)
            assert len(tr.records) == 1 and "al_solve_fused_kernel" in tr.records[0][0], tr.records
        else:
            x, u = ctrl(x0, al_utils.QuadCost(C, c), dyn, dyn.jac)
        gC, gc = torch.autograd.grad(x.double().sum() + 2.0 * u.double().sum(), (C, c))
        return x.detach(), u.detach(), gC, gc

    x0, x_ref, u_ref, C, c = batch(0)
    eager(x0, x_ref, u_ref, C, c, trace=True)
    ctrl = make()
    ctrl.mask = torch.ones(B, T, 1, device="cuda")
    g = AL_mpc.GraphedMPC(ctrl, (x0, C, c), dyn, x_init=x_ref, u_init=u_ref)
    for seed in (0, 1):
        x0b, x_refb, u_refb, Cb, cb = batch(seed)
        g.x_init.copy_(x_refb); g.u_init.copy_(u_refb)
        x, u = g(x0b, Cb, cb)
        gC, gc = torch.autograd.grad(x.double().sum() + 2.0 * u.double().sum(), (Cb, cb))
        wb = eager(x0b, x_refb, u_refb, Cb, cb)
        for a, b in zip((x, u, gC, gc), wb):
            assert torch.equal(a, b)
    assert not g.failed()
