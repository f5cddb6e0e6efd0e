#!/usr/bin/env python3
"""The price of state bounds for a CALLER's dynamics module: forward + backward of one cold AL_mpc.MPC
call with a toy module that is no registered model, variants alternating inside one process, median and quartiles of
the per-call times after warm-up, and the library's launch trace per variant:

  (a) no state box
  (b) a state box that never binds (-+1e3), on the block-tridiagonal step (dqp_al_banded_newton_step_jac_xbounds)
  (c) a box that binds on a third of the knots -- reported only: an active set changes the iterate path
  (p) the same as (b) with AL_mpc.BANDED_USER_DYNAMICS = False: the general torch route with its dense Jacobian and
      (B, nz, nz) Hessian, which is where a state box sent such a caller before.  The comparator, not the code under test.

Shapes: the nz 60 and nz 120 shapes of tools/bench_al_user.py, (12, 4) T 30 and (13, 4) T 30, at a batch size the dense
route still fits in memory (--batch-dense, default 4096 at n + m = 3 and 64 at the two large ones), and (a), (b), (c)
alone at --batch (default 8192).

usage: tools/bench_al_user_xbounds.py [--reps N] [--batch B] [--batch-dense B] [--only K | --from K]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from diff_qp_mpc_amd import AL_mpc, al_utils, _lib
from diff_qp_mpc_amd.dynamics import recognise


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


class Toy(torch.nn.Module):
    """x+ = x + dt (A x + 0.3 sin(x) + B u) with analytic Jacobians"""

    def __init__(self, n, m, dt=0.05):
        super().__init__()
        g = torch.Generator().manual_seed(100 * n + m)
        self.dt = dt
        self.A = (0.3 * torch.randn(n, n, generator=g, dtype=torch.float64)).cuda()
        self.Bm = torch.randn(n, m, generator=g, dtype=torch.float64).cuda()

    def forward(self, x, u):
        return x + self.dt * (x @ self.A.T + 0.3 * torch.sin(x) + u @ self.Bm.T)

    def jac(self, x, u):
        eye = torch.eye(x.shape[1], dtype=x.dtype, device=x.device)
        R = eye + self.dt * (self.A + 0.3 * torch.diag_embed(torch.cos(x)))
        return self.forward(x, u), (R, (self.dt * self.Bm).expand(x.shape[0], -1, -1))


def case(n, m, T, B, with_parent, warmup, reps):
    mod = Toy(n, m)
    assert recognise(mod, n, m, dt=mod.dt, device="cuda") is None
    gen = torch.Generator().manual_seed(0)
    x0 = (torch.rand(B, n, generator=gen, dtype=torch.float64) - 0.5).cuda()
    Qd = torch.ones(B, T, n + m, dtype=torch.float64).cuda(); Qd[..., n:] = 1e-2
    x_ref = x0[:, None, :] * torch.linspace(1.0, 0.0, T, dtype=torch.float64, device="cuda")[None, :, None]
    u_ref = torch.zeros(B, T, m, dtype=torch.float64, device="cuda")
    C = torch.diag_embed(Qd).requires_grad_()
    c = (-(Qd * torch.cat((x_ref, u_ref), 2))).requires_grad_()
    lim = torch.full((m,), 2.0, dtype=torch.float64).cuda()
    # (c): the box follows the reference line, tight above it on every third knot
    w = torch.full((B, T, n), 5.0, dtype=torch.float64, device="cuda")
    hi = x_ref + w
    hi[:, 1::3] = x_ref[:, 1::3] + 0.01
    wide = (torch.full((n,), -1e3, dtype=torch.float64).cuda(), torch.full((n,), 1e3, dtype=torch.float64).cuda())
    variants = [("(a) no state box", None, True), ("(b) box that never binds", wide, True),
                ("(c) box binding on a third of the knots", ((x_ref - w).contiguous(), hi.contiguous()), True)]
    if with_parent:
        variants.append(("(p) as (b), general torch route", wide, False))
    ctrls = [AL_mpc.MPC(n, m, T, u_lower=-lim, u_upper=lim, n_batch=B, verbose=0, solver_type="dense",
                        dtype=torch.float64, eps=1e-5, exit_unconverged=False, backprop=False,
                        **({} if bx is None else dict(x_lower=bx[0], x_upper=bx[1]))) for _, bx, _ in variants]

    def call(i):
        ctrl = ctrls[i]
        AL_mpc.BANDED_USER_DYNAMICS = variants[i][2]
        ctrl.reinitialize(x0, torch.ones(B, T, 1, device="cuda"))
        ctrl.x_init, ctrl.u_init = x_ref, u_ref
        torch.cuda.synchronize(); t0 = time.perf_counter()
        x, u = ctrl(x0, al_utils.QuadCost(C, c), mod, mod.jac)
        (x.double().sum() + 2.0 * u.double().sum()).backward()
        torch.cuda.synchronize()
        AL_mpc.BANDED_USER_DYNAMICS = True
        return time.perf_counter() - t0, x.detach()

    if with_parent:         # the dense route may not run at all at a large nz (its batched LU allocates per problem)
        try:
            call(len(variants) - 1)
        except RuntimeError as e:
            print("(%d, %d) B=%d T=%d nz=%d  %s does not run: %s" % (n, m, B, T, T * (n + m), variants[-1][0],
                                                                     str(e).splitlines()[0][:160]), flush=True)
            AL_mpc.BANDED_USER_DYNAMICS = True
            variants.pop(); ctrls.pop()
            with_parent = False
    times, xs = [[] for _ in variants], [None] * len(variants)
    for r in range(warmup + reps):
        for i in range(len(variants)):             # alternate the variants inside one run
            t, xs[i] = call(i)
            if r >= warmup:
                times[i].append(t * 1e3)
    for i, ((name, _, _), ts) in enumerate(zip(variants, times)):
        q1, med, q3 = np.percentile(ts, [25, 50, 75])
        print("(%d, %d) B=%d T=%d nz=%d  %-42s median %.3f ms  quartiles [%.3f, %.3f]  (%d calls, forward + backward)" % (
            n, m, B, T, T * (n + m), name, med, q1, q3, len(ts)), flush=True)
        torch.cuda.reset_peak_memory_stats()
        with _lib.trace(4096) as tr:
            call(i)
        print("      peak device memory of one call: %.1f MiB" % (torch.cuda.max_memory_allocated() / 2 ** 20))
        for k, (cnt, ms) in sorted(tr.by_kernel().items(), key=lambda kv: -kv[1][0] * kv[1][1]):
            print("      %3d x %8.4f ms  %s" % (cnt, ms, k[:150]))
        assert not any(bool(f.any()) for f in ctrls[i].fail_log)
    print("   (a) == (b) iterates: max |x| difference %.2e; active state multipliers in (c): %d of %d" % (
        float((xs[0] - xs[1]).abs().max()), int((ctrls[2].lamda_prev[:, T * n + 2 * T * m:] > 0).sum()), 2 * B * T * n))
    if with_parent:
        print("   (b) vs (p) iterates: max |x| difference %.2e" % float((xs[1] - xs[3]).abs().max()), flush=True)


if __name__ == "__main__":
    reps, batch, only, first = arg("--reps", 15), arg("--batch", 8192), arg("--only", -1), arg("--from", 0)
    shapes = [(2, 1, 20, 4096), (2, 1, 40, 4096), (12, 4, 30, 64), (13, 4, 30, 64)]
    for k, (n, m, T, Bd) in enumerate(shapes):
        if only not in (-1, k) or k < first:
            continue
        case(n, m, T, arg("--batch-dense", Bd), True, 3, reps)
        case(n, m, T, batch, False, 3, reps)
