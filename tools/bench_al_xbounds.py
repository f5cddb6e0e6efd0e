#!/usr/bin/env python3
"""The price of state bounds on the device AL_mpc paths: forward + backward of one cold AL_mpc.MPC
call at config 3's and config 4's shapes (cartpole-1 T 20; quadrotor T 30, B 8192) in three variants, alternating inside
one process, median and quartiles of the per-call times after warm-up, and the library's launch trace per variant:

  (a) no state box                       -- the launch list and the time of the parent commit
  (b) a state box that never binds       -- (b) - (a) is the price: two more loads per knot, a handful of flops on the x lanes
  (c) a box that binds on about a third of the knots -- reported only: an active set changes the iterate path

usage: tools/bench_al_xbounds.py [--reps N] [--batch B]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from diff_qp_mpc_amd import AL_mpc, al_utils, _lib
from diff_qp_mpc_amd.dynamics import DeviceDynamics


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def case(robot, T, B, mid, warmup, reps):
    dyn = DeviceDynamics(robot)
    n, m = dyn.n_state, dyn.n_ctrl
    gen = torch.Generator().manual_seed(0)
    x0 = (torch.rand(B, n, generator=gen, dtype=torch.float64) - 0.5).cuda()
    Qd = torch.ones(B, T, n + m, dtype=torch.float64).cuda(); Qd[..., n:] = 1e-3
    x_ref = x0[:, None, :] * torch.linspace(1.0, 0.0, T, dtype=torch.float64, device="cuda")[None, :, None]
    u_ref = torch.full((B, T, m), mid, dtype=torch.float64, device="cuda")
    C = torch.diag_embed(Qd).requires_grad_()
    c = (-(Qd * torch.cat((x_ref, u_ref), 2))).requires_grad_()
    lim = torch.full((m,), 6.0, dtype=torch.float64).cuda()
    # (c): the box follows the reference line, tight above it on every third knot
    w = torch.full((B, T, n), 5.0, dtype=torch.float64, device="cuda")
    hi = x_ref + w
    hi[:, 1::3] = x_ref[:, 1::3] + 0.01
    boxes = [("(a) no state box", None), ("(b) box that never binds", (torch.full((n,), -1e3, dtype=torch.float64).cuda(),
                                                                          torch.full((n,), 1e3, dtype=torch.float64).cuda())),
             ("(c) box binding on a third of the knots", ((x_ref - w).contiguous(), hi.contiguous()))]
    ctrls = [AL_mpc.MPC(n, m, T, u_lower=mid - lim, u_upper=mid + lim, n_batch=B, verbose=0, solver_type="dense",
                        dtype=torch.float64, eps=1e-5, exit_unconverged=False, backprop=False,
                        **({} if bx is None else dict(x_lower=bx[0], x_upper=bx[1]))) for _, bx in boxes]

    def call(ctrl):
        ctrl.reinitialize(x0, torch.ones(B, T, 1, device="cuda"))
        ctrl.x_init, ctrl.u_init = x_ref, u_ref
        torch.cuda.synchronize(); t0 = time.perf_counter()
        x, u = ctrl(x0, al_utils.QuadCost(C, c), dyn, dyn.jac)
        (x.double().sum() + 2.0 * u.double().sum()).backward()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, x.detach()

    times, xs = [[] for _ in boxes], [None] * len(boxes)
    for r in range(warmup + reps):
        for i in range(len(boxes)):             # alternate the variants inside one run
            t, xs[i] = call(ctrls[i])
            if r >= warmup:
                times[i].append(t * 1e3)
    for i, ((name, _), ts) in enumerate(zip(boxes, times)):
        q1, med, q3 = np.percentile(ts, [25, 50, 75])
        print("%s B=%d T=%d  %-42s median %.3f ms  quartiles [%.3f, %.3f]  (%d calls, forward + backward)" % (
            robot, B, T, name, med, q1, q3, len(ts)))
        with _lib.trace(4096) as tr:
            call(ctrls[i])
        for k, (cnt, ms) in sorted(tr.by_kernel().items(), key=lambda kv: -kv[1][0] * kv[1][1]):
            print("      %3d x %8.4f ms  %s" % (cnt, ms, k[:150]))
        assert not any(bool(f.any()) for f in ctrls[i].fail_log)
    print("   (a) == (b) iterates: max |x| difference %.2e; active state multipliers in (c): %d of %d" % (
        float((xs[0] - xs[1]).abs().max()), int((ctrls[2].lamda_prev[:, T * n + 2 * T * m:] > 0).sum()), 2 * B * T * n))


if __name__ == "__main__":
    reps, batch = arg("--reps", 20), arg("--batch", 8192)
    case("cartpole1l", 20, batch, 0.0, 3, reps)
    case("rexquadrotor", 30, batch, 14.5, 3, reps)
