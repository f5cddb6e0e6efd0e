"""State bounds on the single-launch AL_mpc solve: dqp_al_mpc_solve_fused_xbounds (csrc/dqp_al_fused.hip, the
al_solve_fused_kernel<BoxBounds<Model>> instantiations) through the C ABI and through AL_mpc.PERSISTENT_SOLVE.

 1. against the launch train dqp_al_mpc_solve_xbounds on the same inputs: the same arithmetic up to summation order
 2. AL_mpc.MPC with the switch on against the extended oracle (tests/al_xbounds_oracle.py), gradients against the general
    torch path; the quadrotor stays on the launch train
 3. an inactive box against dqp_al_mpc_solve_fused_bounds            6. GraphedMPC replay
 4. an indefinite Newton system: the same flags, then the LU path   7. guard bands around every array
 5. argument checks

Shapes of 1: pendulum1l T 2 (the minimum, one Newton step per AL iteration as in tests/test_gpu_al_fused.py), cartpole2l
T 5, cartpole1l T 17 (the knot loops run past one 8-lane group), cartpole2l T 32 (the largest LDS carve: 60 416 B).
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import al_xbounds_oracle as xo
import guardband as gb
import test_gpu_al_fused as fz
import test_gpu_al_xbounds as xb

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NEWTON_STEPS = 4
dev, _ptr = fz.dev, fz._ptr
switch_on = fz.switch_on


def np_(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------ the C ABI
def solve(entry, dyn, T, al_iter, ins, box=None, prev=None, newton_steps=NEWTON_STEPS, trace=None):
    """one call of a dqp_al_mpc_solve[_fused]_bounds / _xbounds entry -> dict of its outputs (and the workspace).
    ins: [x_init, u_init, x0, Qd, q, lo, hi, lam, rho] device tensors; box: (x_lower, x_upper) or None."""
    from diff_qp_mpc_amd import _lib, al_utils
    lib = _lib.load()
    x_init, u_init, x0, Qd, q, lo, hi, lam, rho = [t.contiguous() for t in ins]
    B, n, m = x0.shape[0], dyn.n_state, dyn.n_ctrl
    nt, ncon = n + m, T * n + 2 * T * m + (2 * T * n if box is not None else 0)
    assert lam.shape == (B, ncon) and entry.endswith("_xbounds" if box is not None else "_bounds")
    dims = _lib.dqp_al_mpc_dims(B, n, m, T)
    kw = dict(dtype=torch.float64, device="cuda")
    o = dict(xu=torch.full((B, T, nt), np.nan, **kw), hist_cost=torch.full((al_iter + 1, B), np.nan, **kw),
             hist_lam=torch.full((al_iter + 1, B, ncon), np.nan, **kw), hist_rho=torch.full((al_iter + 1, B), np.nan, **kw),
             res_norm=torch.full((B,), np.nan, **kw),
             factor=torch.zeros(int(lib.dqp_al_banded_factor_bytes(ctypes.byref(dims), dyn.id)) // 8, **kw),
             status=torch.full((B,), np.nan, **kw), fail=torch.full((al_iter,), 7, dtype=torch.int32, device="cuda"),
             ws=torch.zeros(int(lib.dqp_al_mpc_solve_xbounds_bytes(ctypes.byref(dims))) // 8 + 1, **kw))
    bd = al_utils.bounds_layout(lo, hi, B, T, m)
    boxes = (bd.ref(),) if box is None else (bd.ref(), al_utils.bounds_layout(box[0], box[1], B, T, n).ref())
    pc, pl, pr = prev if prev is not None else (None, None, None)
    with _lib.trace(1024) as tr:
        rc = getattr(lib, entry)(ctypes.byref(dims), dyn.id, dyn.dt, al_iter, newton_steps, _ptr(x_init), _ptr(u_init), _ptr(x0),
                                 _ptr(Qd), _ptr(q), *boxes, _ptr(lam), _ptr(rho), _ptr(pc), _ptr(pl), _ptr(pr),
                                 0 if prev is None else pc.shape[0], _ptr(o["xu"]), _ptr(o["hist_cost"]), _ptr(o["hist_lam"]),
                                 _ptr(o["hist_rho"]), _ptr(o["res_norm"]), _ptr(o["factor"]), _ptr(o["status"]), _ptr(o["fail"]),
                                 _ptr(o["ws"]), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
    assert rc == 0, (entry, rc)
    o["dims"] = dims
    o["names"] = [k for k, _ in tr.records]
    return o


# the layout of the state box and of the control box of a case of test 1: every state-box layout in at least one case,
# the control box a vector without a previous call and (B, T, m) with one
def layouts(B, al_iter, n_prev):
    if B == 1:
        return ("n" if n_prev == 0 else "Tn"), ("vector" if n_prev == 0 else "BTm")
    return ("B1n" if al_iter == 1 else "BTn"), ("vector" if n_prev == 0 else "BTm")


def boxed_problem(robot, T, B, seed, state_layout, ctrl_layout):
    """tests/test_gpu_al_fused.py::problem_np (a tracking problem far from converged after two AL iterations) with a state
    box and the multipliers of its rows.  The box is tight around the reference line (per-sample layouts) or around the
    origin (shared layouts) -- half-widths 0.05 above and 0.15 below, times 1 + 0.1 j over the states, so that states of
    size 1 leave it and the penalty of rho = 1 .. 100 does not bring them back -- on every sample but the last of B = 3,
    whose box (per-sample layouts only) is 1e3 wide: its state multipliers stay 0."""
    from diff_qp_mpc_amd.dynamics import DeviceDynamics
    dyn = DeviceDynamics(robot)
    n, m = dyn.n_state, dyn.n_ctrl
    x_init, u_init, x0, Qd, q, lo, hi, lam, rho = fz.problem_np(robot, n, m, T, B, seed)
    x_ref = x0[:, None, :] * np.linspace(1.0, 0.0, T)[None, :, None]
    w = (1.0 + 0.1 * np.arange(n))[None, None, :] * np.ones((B, T, 1))
    if B == 3:
        w = w * np.array([1.0, 4.0, 1e3 / 0.05])[:, None, None]
    fade = np.linspace(1.0, 0.5, T)[None, :, None]
    if state_layout == "n":
        xl, xh = -0.15 * w[0, 0], 0.05 * w[0, 0]
    elif state_layout == "Tn":
        xl, xh = (-0.15 * w * fade)[0], (0.05 * w * fade)[0]
    elif state_layout == "B1n":
        xl, xh = -0.15 * w[:, :1], 0.05 * w[:, :1]
    else:
        xl, xh = x_ref - 0.15 * w * fade, x_ref + 0.05 * w * fade
    if ctrl_layout == "BTm":
        s = np.linspace(1.0, 0.6, B * T).reshape(B, T, 1) * (1.0 + 0.1 * np.arange(m))
        lo, hi = -1.5 * s, 1.2 * s
    lam = np.zeros((B, xo.ncon_x(n, m, T)))
    ins = [dev(a) for a in (x_init, u_init, x0, Qd, q, lo, hi, lam, rho)]
    return dyn, ins, (dev(np.ascontiguousarray(xl)), dev(np.ascontiguousarray(xh)))


def boxed_inputs(robot, T, B, n_prev, seed, state_layout, ctrl_layout):
    """tests/test_gpu_al_fused.py::inputs with the state box: with n_prev = 3 a previous launch-train call's history and
    that file's disturbed start (a new x0, the previous solution disturbed: x_init[:, 0] != x0)"""
    dyn, ins, box = boxed_problem(robot, T, B, seed, state_layout, ctrl_layout)
    prev = None
    if n_prev:
        first = solve("dqp_al_mpc_solve_xbounds", dyn, T, n_prev - 1, ins, box)
        prev = (first["hist_cost"], first["hist_lam"], first["hist_rho"])
        n = dyn.n_state
        r = np.random.default_rng(seed + 1)
        ins[2] = ins[2] + dev(0.3 * r.standard_normal(tuple(ins[2].shape)))
        ins[0] = first["xu"][:, :, :n].contiguous() + dev(0.05 * r.standard_normal((B, T, n)))
        ins[1] = first["xu"][:, :, n:].contiguous() + dev(0.2 * r.standard_normal((B, T, dyn.n_ctrl)))
        ins[7], ins[8] = first["hist_lam"][-1].contiguous(), first["hist_rho"][-1].contiguous()
        assert not bool(torch.isclose(ins[0][:, 0], ins[2]).all())
    return dyn, ins, box, prev


def state_rows_as_required(dyn, multi, T, B):
    """on the launch train's output alone: at B = 3 a sample that ends with a positive state multiplier and one whose
    state multipliers are all zero; at B = 1 a positive state multiplier"""
    lx = np_(multi["hist_lam"][-1])[:, T * dyn.n_state + 2 * T * dyn.n_ctrl:]
    pos, zero = (lx > 0).any(1), (lx == 0).all(1)
    return bool(pos.any()) and (B == 1 or bool(zero.any()))


def both(robot, T, B, al_iter, n_prev, seed, newton_steps):
    """-> (dyn, launch-train outputs, single-launch outputs) on the first of the seeds seed, seed + 1000, ... at which
    the launch train itself has no near-tie among its last candidates and ends with the state rows the case needs (the
    choice looks at the launch train only); none among 16 seeds is a wrong input construction"""
    sl, cl = layouts(B, al_iter, n_prev)
    for k in range(16):
        dyn, ins, box, prev = boxed_inputs(robot, T, B, n_prev, seed + 1000 * k, sl, cl)
        multi = solve("dqp_al_mpc_solve_xbounds", dyn, T, al_iter, ins, box, prev, newton_steps)
        if fz.last_merits_distinct(dyn, multi, T, B) and state_rows_as_required(dyn, multi, T, B):
            return dyn, multi, solve("dqp_al_mpc_solve_fused_xbounds", dyn, T, al_iter, ins, box, prev, newton_steps)
    raise AssertionError("no seed without a near-tie in the launch train's line search and with the required state rows")


def report(what, multi, fused):
    print(what, " ".join("max |%s: fused - train| = %.3e" % (k, float((fused[k] - multi[k]).abs().max()))
                         for k in ("xu", "hist_cost", "hist_lam", "res_norm")))


# ------------------------------------------------------------------ 1
@pytest.mark.parametrize("n_prev", [0, 3])
@pytest.mark.parametrize("al_iter", [1, 2])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("robot,T,newton_steps", [("pendulum1l", 2, 1), ("cartpole2l", 5, 4), ("cartpole1l", 17, 4), ("cartpole2l", 32, 4)])
def test_single_launch_matches_the_launch_train(robot, T, newton_steps, B, al_iter, n_prev):
    """tests/test_gpu_al_fused.py::compare, its tolerances: iterates, costs, multipliers, res_norm rtol 1e-8 / atol 1e-8,
    hist_rho, status and fail exact, the kept factor through dqp_al_banded_solve of a random right-hand side rtol 1e-8 /
    atol 1e-10 -- two paths that differ in summation order only."""
    dyn, multi, fused = both(robot, T, B, al_iter, n_prev, seed=100 * T + B, newton_steps=newton_steps)
    assert not bool(multi["fail"].any())
    assert len(fused["names"]) == 1 and "al_solve_fused_kernel<dqp::BoxBounds<" in fused["names"][0], fused["names"]
    assert not any("al_solve_fused_kernel" in k for k in multi["names"])
    assert sum("al_banded_newton_kernel<dqp::BoxBounds<" in k for k in multi["names"]) == al_iter * newton_steps
    report("%s T %d B %d al_iter %d n_prev %d:" % (robot, T, B, al_iter, n_prev), multi, fused)
    fz.compare(dyn, multi, fused, T, B)


# ------------------------------------------------------------------ 2
FUSED_MPC_CASES = [("pendulum_euler", 5, 6), ("cartpole2l", 5, 3), ("cartpole1l", 6, 3)]


@pytest.mark.parametrize("robot,T,B", FUSED_MPC_CASES)
def test_al_mpc_switch_on_vs_extended_oracle(robot, T, B, switch_on):
    """tests/test_gpu_al_xbounds.py::test_al_mpc_cold_and_warm_vs_extended_oracle with PERSISTENT_SOLVE on: its problems,
    its input conditions and its tolerances (mpc_tol); each call is exactly one al_solve_fused_kernel<BoxBounds<>> launch."""
    p, o1, o2 = xb.mpc_case(robot, T, B)
    xb.check_mpc_inputs(robot, T, B, p, o1)
    n, m = xb.SIZES[robot]
    tol = xb.mpc_tol(robot)
    got = xb.run_mpc(robot, T, B, p, p["xl"], p["xh"], grads=True)
    for g, names in got:
        assert not g["fail"]
        fused = [k for k in names if "al_solve_fused_kernel" in k]
        assert len(fused) == 1 and "al_solve_fused_kernel<dqp::BoxBounds<" in fused[0], names
        assert not any("al_banded_newton_kernel" in k or "al_outer_kernel" in k or "al_start" in k for k in names), names
    for (g, _), o, lam_tol, call in zip(got, (o1, o2), tol["lam"], ("cold", "warm")):
        assert g["lam"].shape == (B, xo.ncon_x(n, m, T))
        for k in ("x", "u", "lam"):
            print(robot, call, k, "max |gpu - oracle| = %.3e" % float(np.abs(g[k] - o[k]).max()))
        for k in ("x", "u"):
            np.testing.assert_allclose(g[k], o[k], rtol=tol["xu"][0], atol=tol["xu"][1], err_msg=call + " " + k)
        np.testing.assert_allclose(g["lam"], o["lam"], rtol=lam_tol[0], atol=lam_tol[1], err_msg=call)
        np.testing.assert_array_equal(g["rho"], o["rho"], err_msg=call)


@pytest.mark.parametrize("robot,T,B", FUSED_MPC_CASES)
def test_backward_switch_on_vs_general_path(robot, T, B, switch_on, monkeypatch):
    """tests/test_gpu_al_xbounds.py::test_backward_vs_general_path with the switch on: dC, dc of sum(x) + 2 sum(u) through
    the factor the single launch keeps, against the general torch path; rtol 1e-4, atol 1e-6 pendulum / 1e-5 others."""
    AL_mpc = switch_on
    p, o1, _ = xb.mpc_case(robot, T, B)
    n, m = xb.SIZES[robot]
    assert (o1["lam"][:, T * n + 2 * T * m:] > 0).any()
    dev_out = xb.run_mpc(robot, T, B, p, p["xl"], p["xh"], grads=True, calls=1)[0]
    monkeypatch.setattr(AL_mpc, "ONE_CALL_SOLVE", False)
    monkeypatch.setattr(AL_mpc, "FUSED_NEWTON_AL", False)
    gen_out = xb.run_mpc(robot, T, B, p, p["xl"], p["xh"], grads=True, calls=1)[0]
    assert sum("al_solve_fused_kernel<dqp::BoxBounds<" in k for k in dev_out[1]) == 1
    assert not any("al_banded" in k or "BoxBounds<" in k for k in gen_out[1]), gen_out[1]
    atol = 1e-6 if robot == "pendulum_euler" else 1e-5
    for k in ("dC", "dc"):
        print(robot, k, "max |single launch - general| = %.3e" % float(np.abs(dev_out[0][k] - gen_out[0][k]).max()))
    assert np.abs(dev_out[0]["dc"]).max() > 1e-3
    for k in ("dC", "dc"):
        np.testing.assert_allclose(dev_out[0][k], gen_out[0][k], rtol=1e-4, atol=atol, err_msg=k)


def test_quadrotor_with_the_switch_on_stays_on_the_launch_train(switch_on, monkeypatch):
    """n_state + n_ctrl = 16 has no single-launch kernel: with the switch on the call is the launch train's, bit for bit"""
    AL_mpc = switch_on
    robot, T, B = "rexquadrotor", 4, 3
    p = xb.mpc_problem(robot, T, B)
    on = xb.run_mpc(robot, T, B, p, p["xl"], p["xh"], calls=1)[0]
    monkeypatch.setattr(AL_mpc, "PERSISTENT_SOLVE", False)
    off = xb.run_mpc(robot, T, B, p, p["xl"], p["xh"], calls=1)[0]
    assert on[1] == off[1] and not any("al_solve_fused_kernel" in k for k in on[1])
    assert sum("al_banded_newton_kernel<dqp::BoxBounds<" in k for k in on[1]) == 8 and not on[0]["fail"]
    for k in ("x", "u", "lam", "rho"):
        assert on[0][k].tobytes() == off[0][k].tobytes(), k


def test_switch_off_and_no_box_launch_what_they_launched(switch_on, monkeypatch):
    """with the switch off a state box runs the launch train; with it on and no state box the StridedBounds<> single launch"""
    AL_mpc = switch_on
    robot, T, B = "cartpole2l", 5, 3
    p = xb.mpc_problem(robot, T, B)
    free = xb.run_mpc(robot, T, B, p, None, None, calls=1)[0]
    assert len(free[1]) == 1 and "al_solve_fused_kernel<dqp::StridedBounds<" in free[1][0], free[1]
    monkeypatch.setattr(AL_mpc, "PERSISTENT_SOLVE", False)
    off = xb.run_mpc(robot, T, B, p, p["xl"], p["xh"], calls=1)[0]
    assert not any("al_solve_fused_kernel" in k for k in off[1])
    assert sum("al_banded_newton_kernel<dqp::BoxBounds<" in k for k in off[1]) == 8


# ------------------------------------------------------------------ 3
@pytest.mark.parametrize("robot,T,B,shape", [("cartpole2l", 5, 3, "n"), ("cartpole1l", 17, 3, "BTn"), ("pendulum1l", 2, 1, "BTn")])
def test_inactive_box_is_the_bounds_call(robot, T, B, shape):
    """Both state bounds at -+1e30 and zero state multipliers against dqp_al_mpc_solve_fused_bounds on the same inputs: the
    old rows and the iterates within test 1's tolerances, the state multipliers exactly 0; the call without a box launches
    no BoxBounds<> kernel.  (Whether the two are bit-identical is printed, not required.)"""
    dyn, ins, _ = boxed_problem(robot, T, B, 7 * T + B, "BTn", "BTm")
    n, m = dyn.n_state, dyn.n_ctrl
    ncu = T * n + 2 * T * m
    free_ins = list(ins)
    free_ins[7] = ins[7][:, :ncu].contiguous()
    ref = solve("dqp_al_mpc_solve_fused_bounds", dyn, T, 2, free_ins)
    s = (n,) if shape == "n" else (B, T, n)
    got = solve("dqp_al_mpc_solve_fused_xbounds", dyn, T, 2, ins, (dev(np.full(s, -1e30)), dev(np.full(s, 1e30))))
    assert len(ref["names"]) == 1 and "al_solve_fused_kernel<dqp::StridedBounds<" in ref["names"][0], ref["names"]
    assert len(got["names"]) == 1 and "al_solve_fused_kernel<dqp::BoxBounds<" in got["names"][0], got["names"]
    assert not bool(ref["fail"].any()) and bool(torch.isfinite(ref["xu"]).all())
    assert bool((got["hist_lam"][:, :, ncu:] == 0.0).all())
    cut = dict(got, hist_lam=got["hist_lam"][:, :, :ncu].contiguous())
    same = all(torch.equal(cut[k], ref[k]) for k in ("xu", "hist_cost", "hist_lam", "hist_rho", "res_norm", "status", "fail", "factor"))
    print("%s T %d B %d %s: inactive box bit-identical to the call without: %s" % (robot, T, B, shape, same))
    fz.compare(dyn, ref, cut, T, B)


# ------------------------------------------------------------------ 4
def test_cholesky_failure_flags_and_lu_path(switch_on):
    """The construction of tests/test_gpu_al_fused.py::test_cholesky_failure_flags_and_lu_path (one sample's control cost
    -5e3) with a state box the trajectories leave: the single launch sets the flags the launch train sets, and AL_mpc.MPC
    with the switch on then takes the LU path with the state rows and returns finite x, u."""
    from diff_qp_mpc_amd import _lib, al_utils
    from diff_qp_mpc_amd.dynamics import DeviceDynamics
    AL_mpc = switch_on
    g = fz.load("CFG5_cartpole2l_T5_b4")
    B, T = g["in_Qd"].shape[:2]
    dyn = DeviceDynamics("cartpole2l", dt=float(g["dt"]))
    n, m = dyn.n_state, dyn.n_ctrl
    Qd = g["in_Qd"].copy()
    Qd[1, :, n:] = -5.0e3
    w = 0.5 * np.abs(g["in_x_init"]).max((0, 1)) + 0.05
    box = (dev(-w), dev(w))
    ins = [dev(a) for a in (g["in_x_init"], g["in_u_init"], g["in_x0"], Qd, g["in_c"], g["in_u_lower"].reshape(-1),
                            g["in_u_upper"].reshape(-1), np.zeros((B, xo.ncon_x(n, m, T))), np.ones(B))]
    multi = solve("dqp_al_mpc_solve_xbounds", dyn, T, 2, ins, box)
    fused = solve("dqp_al_mpc_solve_fused_xbounds", dyn, T, 2, ins, box)
    assert bool(multi["fail"].any())
    assert torch.equal(fused["fail"], multi["fail"])
    ctrl = AL_mpc.MPC(n, m, T, u_lower=dev(g["in_u_lower"]), u_upper=dev(g["in_u_upper"]), n_batch=B, verbose=0,
                      solver_type="dense", dtype=torch.float64, eps=1e-5, exit_unconverged=False, backprop=False,
                      x_lower=box[0], x_upper=box[1])
    x0 = dev(g["in_x0"])
    ctrl.reinitialize(x0, torch.ones(B, T, 1, device="cuda"))
    ctrl.x_init, ctrl.u_init = dev(g["in_x_init"]), dev(g["in_u_init"])
    with _lib.trace(2048) as tr:
        x, u = ctrl(x0, al_utils.QuadCost(torch.diag_embed(dev(Qd)), dev(g["in_c"])), dyn, dyn.jac)
    names = [k for k, _ in tr.records]
    assert bool(ctrl.fail_log[-1].any())
    assert sum("al_solve_fused_kernel<dqp::BoxBounds<" in k for k in names) == 1
    assert any("al_newton_kernel" in k for k in names)                     # the general path redid the solve
    assert ctrl.lamda_prev.shape == (B, xo.ncon_x(n, m, T))
    assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(u).all())


# ------------------------------------------------------------------ 5
def test_argument_checks():
    from diff_qp_mpc_amd import _lib
    lib = _lib.load()
    sizes = {"cartpole1l": (4, 1), "rexquadrotor": (12, 4)}

    def call(robot, T, B, al_iter=2, xbox="ok"):
        n, m = sizes[robot]
        Bb, Tt = max(B, 1), max(T, 1)
        kw = dict(dtype=torch.float64, device="cuda")
        ncon = Tt * (n + 2 * m + 2 * n)
        buf = lambda *s: torch.full(s, 3.0, **kw)
        outs = [buf(Bb, Tt, n + m), buf(al_iter + 1, Bb), buf(al_iter + 1, Bb, ncon), buf(al_iter + 1, Bb), buf(Bb),
                buf(Bb * Tt * (n + m) * (2 * n + m + 1)), buf(Bb)]
        fail = torch.full((al_iter,), 7, dtype=torch.int32, device="cuda")
        d = _lib.dqp_al_mpc_dims(B, n, m, T)
        ws = buf(int(lib.dqp_al_mpc_solve_fused_bytes_xbounds(ctypes.byref(_lib.dqp_al_mpc_dims(Bb, n, m, max(T, 2))))) // 8 + 8)
        ins = [buf(Bb, Tt, n), buf(Bb, Tt, m), buf(Bb, n), buf(Bb, Tt, n + m), buf(Bb, Tt, n + m)]
        lo, hi, xl, xh = buf(m) - 5.0, buf(m), buf(Bb, Tt, n) - 5.0, buf(Bb, Tt, n)
        bd = _lib.dqp_al_bounds(lo.data_ptr(), hi.data_ptr(), 0, 0)
        xbd = {"ok": _lib.dqp_al_bounds(xl.data_ptr(), xh.data_ptr(), Tt * n, n),
               "stride": _lib.dqp_al_bounds(xl.data_ptr(), xh.data_ptr(), Tt * n, n + 1), "null": None}[xbox]
        rc = lib.dqp_al_mpc_solve_fused_xbounds(ctypes.byref(d), _lib.DQP_DYN[robot], 0.05, al_iter, NEWTON_STEPS,
                                                *[_ptr(t) for t in ins], ctypes.byref(bd),
                                                ctypes.byref(xbd) if xbd is not None else None, _ptr(buf(Bb, ncon)), _ptr(buf(Bb)),
                                                None, None, None, 0, *[_ptr(t) for t in outs], _ptr(fail), _ptr(ws), None)
        torch.cuda.synchronize()
        return rc, outs, fail

    rc, outs, fail = call("cartpole1l", 5, 0)                      # nbatch = 0: DQP_OK, nothing touched
    assert rc == 0
    assert all(bool((t == 3.0).all()) for t in outs) and bool((fail == 7).all())
    assert call("cartpole1l", 5, 4, xbox="null")[0] == -1          # DQP_ERR_BAD_ARG
    assert call("cartpole1l", 5, 4, xbox="stride")[0] == -1
    assert call("cartpole1l", 5, 4, al_iter=257)[0] == -1
    assert call("cartpole1l", 5, -1)[0] == -1
    for bad in (("rexquadrotor", 6, 4), ("cartpole1l", 33, 4)):    # DQP_ERR_TOO_LARGE, nothing touched
        rc, outs, fail = call(*bad)
        assert rc == -2
        assert all(bool((t == 3.0).all()) for t in outs) and bool((fail == 7).all())


# ------------------------------------------------------------------ 6
def test_graphed_mpc_replay_bitwise_equal_to_eager_single_launch(switch_on):
    """tests/test_gpu_al_fused.py::test_graphed_mpc_replay_bitwise_equal_to_eager_fused with a (B, T, n) state box that the
    reference line leaves: the replay equals the eager single-launch call bit for bit -- x, u and the gradients -- on the
    captured batch and on a second one, and the forward solve of an eager call is ONE library launch."""
    from diff_qp_mpc_amd import _lib, al_utils
    from diff_qp_mpc_amd.dynamics import DeviceDynamics
    AL_mpc = switch_on
    robot, T, B = "cartpole2l", 5, 8
    dyn = DeviceDynamics(robot)
    nx, nu = dyn.n_state, dyn.n_ctrl
    lo, hi = dev(np.full(nu, -250.0)), dev(np.full(nu, 250.0))
    s = np.linspace(1.0, 0.5, B * T).reshape(B, T, 1) * (1.0 + 0.1 * np.arange(nx))
    xl, xh = dev(-0.3 * s), dev(0.1 * s)
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
                          eps=1e-5, exit_unconverged=False, backprop=False, x_lower=xl, x_upper=xh)

    def eager(x0, x_ref, u_ref, C, c, trace=False):
        ctrl = make()
        ctrl.reinitialize(x0, torch.ones(B, T, 1, device="cuda"))
        ctrl.x_init, ctrl.u_init = x_ref, u_ref
        if trace:
            with _lib.trace() as tr:
                x, u = ctrl(x0, al_utils.QuadCost(C, c), dyn, dyn.jac)
            assert len(tr.records) == 1 and "al_solve_fused_kernel<dqp::BoxBounds<" in tr.records[0][0], tr.records
        else:
            x, u = ctrl(x0, al_utils.QuadCost(C, c), dyn, dyn.jac)
        assert bool((ctrl.lamda_prev[:, T * nx + 2 * T * nu:] > 0).any())       # a state row is active
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


# ------------------------------------------------------------------ 7
def test_guard_bands_cold_then_warm():
    """dqp_al_mpc_solve_fused_xbounds at cartpole-2, T 5, B 3 with a (B, T, n) state box and a (B, T, m) control box, cold and
    then warm from the cold call's history, every array between guards (tests/guardband.py::run_guarded): every guard
    intact, the outputs bit-identical over the "nan" / "nan" / "zero" runs; and, as
    tests/test_gpu_guardband.py::test_al_mpc_solve_through_the_c_abi, against the extended oracle's two calls at mpc_tol."""
    from diff_qp_mpc_amd import _lib, al_utils
    from diff_qp_mpc_amd.dynamics import DeviceDynamics
    lib = _lib.load()
    robot, T, B = "cartpole2l", 5, 3
    p, o1, o2 = xb.mpc_case(robot, T, B)
    assert p["xl"].shape == (B, T, 6) and p["lo"].shape == (B, T, 1)
    dyn = DeviceDynamics(robot, dt=p["dt"])
    n, m = dyn.n_state, dyn.n_ctrl
    nt, ncon = n + m, xo.ncon_x(n, m, T)
    dims = _lib.dqp_al_mpc_dims(B, n, m, T)
    wsb = int(lib.dqp_al_mpc_solve_fused_bytes_xbounds(ctypes.byref(dims)))
    fb = int(lib.dqp_al_banded_factor_bytes(ctypes.byref(dims), dyn.id))
    assert wsb > 0 and fb > 0
    K = 3
    launches = []

    def fn(t):
        x_init, u_init, x0, Qd, q, lo_d, hi_d, lam_in, rho_in, xl_d, xh_d = t
        kw = dict(dtype=torch.float64, device="cuda")
        bd, xbd = al_utils.bounds_layout(lo_d, hi_d, B, T, m), al_utils.bounds_layout(xl_d, xh_d, B, T, n)
        res = {}
        prev, n_prev = (None, None, None), 0
        for call in ("1", "2"):
            xu, hc, hl, hr = torch.empty(B, T, nt, **kw), torch.empty(K, B, **kw), torch.empty(K, B, ncon, **kw), torch.empty(K, B, **kw)
            resn, status, L, ws = torch.empty(B, **kw), torch.empty(B, **kw), torch.empty(fb // 8, **kw), torch.empty(wsb // 8, **kw)
            fail = torch.empty(2, dtype=torch.int32, device="cuda")
            with _lib.trace(64) as tr:
                _lib.call("dqp_al_mpc_solve_fused_xbounds", x0.device, dims, dyn.id, dyn.dt, 2, 4, x_init, u_init, x0, Qd, q,
                          bd.ref(), xbd.ref(), lam_in, rho_in, *prev, n_prev, xu, hc, hl, hr, resn, L, status, fail, ws)
            launches.append([k for k, _ in tr.records])
            res.update({"xu" + call: xu, "hc" + call: hc, "hl" + call: hl, "hr" + call: hr, "resn" + call: resn,
                        "status" + call: status, "fail" + call: fail})
            # the warm call: the float32 rounding of this solution as the start, this call's history, its last entry in
            x_init, u_init = torch.empty(B, T, n, **kw), torch.empty(B, T, m, **kw)
            x_init.copy_(xu[:, :, :n].float())
            u_init.copy_(xu[:, :, n:].float())
            prev, n_prev = (hc, hl, hr), K
            lam_in, rho_in = torch.empty(B, ncon, **kw), torch.empty(B, **kw)
            lam_in.copy_(hl[-1])
            rho_in.copy_(hr[-1])
        return res

    def make(put):
        t = [put(p[k], k) for k in ("x_init", "u_init", "x0", "Qd", "c", "lo", "hi")]
        return t + [put(np.zeros((B, ncon)), "lam_in"), put(np.ones(B), "rho_in"), put(p["xl"], "x_lower"), put(p["xh"], "x_upper")]

    out, sizes = gb.run_guarded(fn, make)
    assert all(len(k) == 1 and "al_solve_fused_kernel<dqp::BoxBounds<" in k[0] for k in launches), launches
    tol = xb.mpc_tol(robot)
    for call, o, lam_tol in (("1", o1, tol["lam"][0]), ("2", o2, tol["lam"][1])):
        assert not np_(out["fail" + call]).any()
        got = np_(out["xu" + call].float())
        print("guarded call", call, "max |xu - oracle| = %.3e, max |lam - oracle| = %.3e"
              % (float(np.abs(got - o["xu"]).max()), float(np.abs(np_(out["hl" + call][-1]) - o["lam"]).max())))
        np.testing.assert_allclose(got, o["xu"], rtol=tol["xu"][0], atol=tol["xu"][1], err_msg="xu" + call)
        np.testing.assert_allclose(np_(out["hl" + call][-1]), o["lam"], rtol=lam_tol[0], atol=lam_tol[1], err_msg="lam" + call)
        np.testing.assert_array_equal(np_(out["hr" + call][-1]), o["rho"].reshape(-1), err_msg="rho" + call)
    assert bool((out["hl2"][-1][:, T * n + 2 * T * m:] > 0).any())
    assert wsb in sizes and fb in sizes, (wsb, fb, sizes)
