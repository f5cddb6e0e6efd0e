#!/usr/bin/env python3
"""Timings of the wide block-tridiagonal NewtonAL route, HIP events after warm-up:
  (a) one AL_mpc.MPC forward + backward with a caller's module (tests/test_gpu_al_given.CallerToy) at (13, 4), T 30,
      B 1024 -- on the wide kernels, and with the banded route switched off (--general: the dense Jacobian / Hessian /
      LU path such a call took before the wide kernels existed; that path's code is unchanged);
  (b) the Newton and solve kernel times of the library's trace at (13, 4), (12, 4), (24, 8) and (14, 7), T 30, B 8192.
usage: python tools/bench_al_wide.py [--skip-general]"""
import argparse, ctypes, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
from diff_qp_mpc_amd import AL_mpc, _lib, al_utils
from test_gpu_al_given import CallerToy, dev, problem

ap = argparse.ArgumentParser()
ap.add_argument("--skip-general", action="store_true")
ap.add_argument("--batch", type=int, default=1024)
args = ap.parse_args()


def mpc_ms(n, m, T, B, warm, reps):
    rng = np.random.default_rng(1)
    mod = CallerToy(n, m)
    x0 = rng.standard_normal((B, n))
    u_init = 0.2 * rng.standard_normal((B, T, m))
    x_init = np.empty((B, T, n)); x_init[:, 0] = x0
    for t in range(T - 1):
        x_init[:, t + 1] = mod.step_np(x_init[:, t], u_init[:, t])[0]
    Qd, c = dev(rng.random((B, T, n + m)) + 0.1), dev(rng.standard_normal((B, T, n + m)))
    times = []
    for k in range(warm + reps):
        ctrl = AL_mpc.MPC(n, m, T, u_lower=dev(np.full(m, -0.5)), u_upper=dev(np.full(m, 0.5)), n_batch=B, verbose=0,
                          solver_type="dense", dtype=torch.float64, eps=1e-5, exit_unconverged=False, backprop=False)
        ctrl.reinitialize(dev(x0), torch.ones(B, T, 1, device="cuda"))
        ctrl.x_init, ctrl.u_init = dev(x_init), dev(u_init)
        C, cc = torch.diag_embed(Qd).requires_grad_(), c.clone().requires_grad_()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        x, u = ctrl(dev(x0), al_utils.QuadCost(C, cc), mod, mod.jac)
        (x.double().sum() + 2.0 * u.double().sum()).backward()
        e1.record(); torch.cuda.synchronize()
        if k >= warm:
            times.append(e0.elapsed_time(e1))
    return float(np.median(times)), x.detach()


ms_w, xw = mpc_ms(13, 4, 30, args.batch, 2, 5)
print("(a) AL_mpc.MPC fwd+bwd (13,4) T 30 B %d, wide kernels: %.2f ms" % (args.batch, ms_w), flush=True)
if not args.skip_general:
    keep = al_utils.banded_jac_supported
    al_utils.banded_jac_supported = lambda *a: False
    ms_g, xg = mpc_ms(13, 4, 30, args.batch, 1, 3)
    al_utils.banded_jac_supported = keep
    print("(a) the same call on the general (dense LU) path: %.2f ms  -> %.1fx; max |x - x| %.2e" % (
        ms_g, ms_g / ms_w, float((xw - xg).abs().max())), flush=True)

lib = _lib.load()
P = lambda x: ctypes.c_void_p(x.data_ptr())
for n, m in [(13, 4), (12, 4), (24, 8), (14, 7)]:
    B, T, nt = 8192, 30, n + m
    p = problem(n, m, T, B=B, seed=9)
    t = {k: dev(v).contiguous() for k, v in p.items()}
    dims = _lib.dqp_al_mpc_dims(B, n, m, T)
    fac = torch.empty(int(lib.dqp_al_banded_jac_factor_bytes(ctypes.byref(dims))) // 8, dtype=torch.float64, device="cuda")
    upd, out = torch.empty(B, T, nt, dtype=torch.float64, device="cuda"), torch.empty(B, T, nt, dtype=torch.float64, device="cuda")
    info = torch.empty(B, dtype=torch.int32, device="cuda")
    rho = t["rho"].reshape(B).contiguous()
    acc = {}
    for k in range(7):
        with _lib.trace(16) as tr:
            assert lib.dqp_al_banded_newton_step_jac(ctypes.byref(dims), P(t["xu"]), P(t["x0"]), P(t["Qd"]), P(t["q"]), P(t["lam"]),
                                                     P(rho), P(t["lo"]), P(t["hi"]), P(t["xn"]), P(t["Jx"]), P(t["Ju"]), P(upd),
                                                     P(fac), P(info), None) == 0
            assert lib.dqp_al_banded_solve(ctypes.byref(dims), 0, P(fac), P(t["rhs"]), P(out), None) == 0
            torch.cuda.synchronize()
        if k >= 2:
            for name, ms in tr.records:
                acc.setdefault("newton" if "newton" in name else "solve", []).append(ms)
    assert int(info.abs().max()) == 0
    print("(b) (%d,%d) T 30 B 8192: newton %.3f ms  solve %.3f ms" % (n, m, np.median(acc["newton"]), np.median(acc["solve"])), flush=True)
