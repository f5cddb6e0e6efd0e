#!/usr/bin/env python3
"""AL_mpc.MPC with a caller-supplied dynamics MODULE (torch nn.Module with its own Jacobian function, what the reference's
envs are): the dense Newton step (dqp_al_assemble + dqp_al_newton_step: Hessian by fp64 MFMA, cyclic LDL^T in registers;
nz <= 128) against the block-tridiagonal step on the module's Jacobians (dqp_al_banded_newton_step_jac) at the same
sizes -- one call = 2 AL iterations x 4 Newton steps + backward, pendulum of deqmpc/envs.py.

--integrator: the reference's `--env integrator --bsz 256 --T 5` (deqmpc/run.sh:3), forward + backward of one cold
AL_mpc.MPC call three ways, alternating, median and quartiles of the per-call times after warm-up:
  (a) a plain torch module of the integrator's formula on the caller-dynamics path (recognition is not involved: the
      module goes to AL_mpc.MPC as it is) -- what the library did for this env before the model was registered
  (b) DeviceDynamics("integrator") on the one-call solve (dqp_al_mpc_solve)
  (c) the same on the persistent solve (dqp_al_mpc_solve_fused; PERSISTENT_SOLVE_MAX_BATCH raised for the run)

--bounds {vector,per_sample,per_knot,full}: the cost of per-sample / per-knot control bounds (dqp_al_bounds) against the
n_ctrl-vector on the same commit.  The SAME limits expanded to the layout -- (B, 1, m), (T, m) or (B, T, m) -- so both
calls compute the same iterates and only the kernels' bound addressing differs; forward + backward of one cold
AL_mpc.MPC call, vector and layout alternating, median and quartiles after warm-up, on the registered pendulum
(one-call solve, and the persistent solve at B = 128) and on the caller's module (dqp_al_banded_newton_step_jac)."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import torch
from diff_qp_mpc_amd import AL_mpc, al_utils
from test_gpu_al import Pendulum, PendulumJac


class IntegratorModule(torch.nn.Module):
    """deqmpc/envs.py:182-233 restated: x+ and (df/dx, df/du) of the semi-implicit Euler step"""
    dt = 0.1

    def forward(self, x, u):
        vel = x[..., 1:] + u * self.dt
        return torch.cat((x[..., :1] + vel * self.dt, vel), dim=-1)

    def jac(self, x, u):
        dt = self.dt
        fx = x.new_tensor([[1.0, dt], [0.0, 1.0]]).expand(x.shape[0], 2, 2)
        fu = x.new_tensor([[dt * dt], [dt]]).expand(x.shape[0], 2, 1)
        return self.forward(x, u), (fx, fu)


def integrator_case(B=256, T=5, warmup=5, reps=40):
    import numpy as np
    from diff_qp_mpc_amd.dynamics import DeviceDynamics
    nx, nu = 2, 1
    gen = torch.Generator().manual_seed(0)
    x0 = ((torch.rand(B, nx, generator=gen, dtype=torch.float64) * 4 - 2) * (torch.arange(B) % 2 * 0.99 + 0.01)[:, None]).cuda()
    Qd = torch.tensor([10.0, 1.0, 0.01], dtype=torch.float64).repeat(B, T, 1).cuda()
    C = torch.diag_embed(Qd).requires_grad_()
    c = torch.zeros(B, T, nx + nu, dtype=torch.float64).cuda().requires_grad_()
    lim = torch.full((nu,), 2.0, dtype=torch.float64).cuda()
    mod, dev_dyn = IntegratorModule(), DeviceDynamics("integrator")
    ways = [("(a) caller's torch module", mod, mod.jac, False), ("(b) registered, one-call solve", dev_dyn, dev_dyn.jac, False),
            ("(c) registered, persistent solve", dev_dyn, dev_dyn.jac, True)]
    ctrls = [AL_mpc.MPC(nx, nu, T, u_lower=-lim, u_upper=lim, n_batch=B, verbose=0, solver_type="dense", dtype=torch.float64,
                        eps=1e-5, exit_unconverged=False, backprop=False) for _ in ways]

    def call(i):
        _, dyn, jac, persistent = ways[i]
        AL_mpc.PERSISTENT_SOLVE, AL_mpc.PERSISTENT_SOLVE_MAX_BATCH = persistent, (B if persistent else 0)
        ctrls[i].reinitialize(x0, torch.ones(B, T, 1, device="cuda"))
        torch.cuda.synchronize(); t0 = time.perf_counter()
        x, u = ctrls[i](x0, al_utils.QuadCost(C, c), dyn, jac)
        (x.double().sum() + 2.0 * u.double().sum()).backward()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, x.detach()

    times, xs = [[] for _ in ways], [None] * len(ways)
    for r in range(warmup + reps):
        for i in range(len(ways)):          # alternate the three ways inside one run
            t, xs[i] = call(i)
            if r >= warmup:
                times[i].append(t * 1e3)
    AL_mpc.PERSISTENT_SOLVE, AL_mpc.PERSISTENT_SOLVE_MAX_BATCH = False, 0
    for (name, *_), ts in zip(ways, times):
        q1, med, q3 = np.percentile(ts, [25, 50, 75])
        print("integrator B=%d T=%d  %-34s median %.3f ms  quartiles [%.3f, %.3f]  (%d calls, forward + backward)" % (
            B, T, name, med, q1, q3, len(ts)))
    print("   max |x| difference to (a): (b) %.2e  (c) %.2e" % (float((xs[1] - xs[0]).abs().max()), float((xs[2] - xs[0]).abs().max())))


def bounds_case(layout, warmup=5, reps=30):
    import numpy as np
    from diff_qp_mpc_amd.dynamics import DeviceDynamics
    nx, nu = 2, 1
    shapes = {"vector": lambda B, T: (nu,), "per_sample": lambda B, T: (B, 1, nu), "per_knot": lambda B, T: (T, nu),
              "full": lambda B, T: (B, T, nu)}
    dev_dyn = DeviceDynamics("pendulum_euler")
    cases = [("registered, one-call solve", 4096, 20, dev_dyn, dev_dyn.jac, False),
             ("registered, persistent solve", 128, 20, dev_dyn, dev_dyn.jac, True),
             ("caller's module, banded step", 4096, 20, Pendulum(), PendulumJac(), False)]
    for name, B, T, dyn, jac, persistent in cases:
        gen = torch.Generator().manual_seed(0)
        x0 = (torch.rand(B, nx, generator=gen, dtype=torch.float64) * 2 - 1).cuda()
        Qd = torch.ones(B, T, nx + nu, dtype=torch.float64).cuda(); Qd[..., nx:] = 1e-2
        C = torch.diag_embed(Qd).requires_grad_()
        c = torch.zeros(B, T, nx + nu, dtype=torch.float64).cuda().requires_grad_()
        ctrls = []
        for lay in ("vector", layout):
            lim = torch.full(shapes[lay](B, T), 2.0, dtype=torch.float64).cuda()
            ctrls.append(AL_mpc.MPC(nx, nu, T, u_lower=-lim, u_upper=lim, n_batch=B, verbose=0, solver_type="dense",
                                    dtype=torch.float64, eps=1e-5, exit_unconverged=False, backprop=False))
        AL_mpc.PERSISTENT_SOLVE, AL_mpc.PERSISTENT_SOLVE_MAX_BATCH = persistent, (B if persistent else 0)

        def call(ctrl):
            ctrl.reinitialize(x0, torch.ones(B, T, 1, device="cuda"))
            torch.cuda.synchronize(); t0 = time.perf_counter()
            x, u = ctrl(x0, al_utils.QuadCost(C, c), dyn, jac)
            (x.double().sum() + 2.0 * u.double().sum()).backward()
            torch.cuda.synchronize()
            return time.perf_counter() - t0, x.detach()

        times, xs = [[], []], [None, None]
        for r in range(warmup + reps):
            for i in (0, 1):                    # alternate the two layouts inside one run
                t, xs[i] = call(ctrls[i])
                if r >= warmup:
                    times[i].append(t * 1e3)
        AL_mpc.PERSISTENT_SOLVE, AL_mpc.PERSISTENT_SOLVE_MAX_BATCH = False, 0
        for lay, ts in zip(("vector", layout), times):
            q1, med, q3 = np.percentile(ts, [25, 50, 75])
            print("bounds B=%d T=%d  %-30s %-10s median %.3f ms  quartiles [%.3f, %.3f]  (%d calls, forward + backward)" % (
                B, T, name, lay, med, q1, q3, len(ts)))
        print("   identical iterates: %s" % bool(torch.equal(xs[0], xs[1])))


if "--bounds" in sys.argv:
    layout = sys.argv[sys.argv.index("--bounds") + 1]
    if layout not in ("vector", "per_sample", "per_knot", "full"):
        sys.exit("--bounds {vector,per_sample,per_knot,full}")
    bounds_case(layout)
    sys.exit(0)

if "--integrator" in sys.argv:
    integrator_case()
    sys.exit(0)

nx, nu = 2, 1
for B, T in ((4096, 20), (4096, 40), (128, 20)):
    gen = torch.Generator().manual_seed(0)
    x0 = (torch.rand(B, nx, generator=gen, dtype=torch.float64) * 2 - 1).cuda()
    Qd = torch.ones(B, T, nx + nu, dtype=torch.float64).cuda(); Qd[..., nx:] = 1e-2
    C = torch.diag_embed(Qd).requires_grad_()
    c = torch.zeros(B, T, nx + nu, dtype=torch.float64).cuda().requires_grad_()
    lim = torch.full((nu,), 2.0, dtype=torch.float64).cuda()
    dyn, dyn_jac = Pendulum(), PendulumJac()
    out = {}
    for name, thr in (("dense Newton step", 128), ("block-tridiagonal on the module's Jacobians", 0)):
        AL_mpc.BANDED_USER_DYNAMICS_FROM_NZ = thr
        ctrl = AL_mpc.MPC(nx, nu, T, u_lower=-lim, u_upper=lim, n_batch=B, verbose=0, solver_type="dense",
                          dtype=torch.float64, eps=1e-5, exit_unconverged=False, backprop=False)
        def step():
            ctrl.reinitialize(x0, torch.ones(B, T, 1, device="cuda"))
            x, u = ctrl(x0, al_utils.QuadCost(C, c), dyn, dyn_jac)
            (x.double().sum() + 2.0 * u.double().sum()).backward()
            return x, u
        for _ in range(2): x, u = step()
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(5): step()
        torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / 5
        out[name] = (dt, x.detach().clone())
        print("B=%d T=%d nz=%d  %-46s %.2f ms per call" % (B, T, T * (nx + nu), name, dt * 1e3))
    a, b = [v[1] for v in out.values()]
    print("   max |x| difference between the two paths: %.2e" % float((a - b).abs().max()))
