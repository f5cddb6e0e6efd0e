#!/usr/bin/env python3
"""Golden vectors for AL_mpc.MPC on the double integrator (the reference's `--env integrator`, deqmpc/run.sh:3),
produced by importing the reference (build container only; see make_golden.py for the ipdb stand-in).

Reference entry points exercised:
  deqmpc/envs.py:182-233,246-289  IntegratorDynamics / IntegratorDynamics_jac (semi-implicit Euler), IntegratorEnv
  qpth/AL_mpc.py:116-321          MPC.__init__/forward/al_solve, reinitialize (:432-438)
  qpth/al_utils.py:363-500        NewtonAL forward/backward

B = 6, T = 5 (run.sh's horizon), al_iter = 2, control bounds +-max_acc = +-2, diagonal cost Qlqr = (10, 1), Rlqr = 0.01
towards the origin.  x0 is drawn (seeded) from env.reset()'s ranges, [-2, 2] x [-max_vel, max_vel]; the last three
samples are then scaled by 0.01, which keeps them inside the ranges and their controls off the bounds: with 10 on the
position against 0.01 on the control every unscaled sample saturates, and with every bound active or every bound
inactive the clamp rows of the merit would be exercised on one side only.  The script asserts that at least two samples
have an active bound and at least two have none, in both calls.

Stored: the inputs, then for the cold call (reinitialize + forward) and the warm call from the stored state: x, u, the
cost_lam_hist rows (oldest first), lamda_prev, rho_prev; for the cold call the gradients wrt C's diagonal and c of the
loss sum(x) + 2 sum(u).

The file is INTEGRATOR_AL_b6.npz, not AL_integrator_b6.npz: tests/test_gpu_al.py and tests/test_oracle_golden.py take
every AL_*.npz for a pendulum fixture of make_golden_al.py.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("DQP_REFERENCE", "/root/reference")
m = types.ModuleType("ipdb")
def _st(*a, **k):
    raise RuntimeError("ipdb.set_trace() reached inside the reference")
m.set_trace = _st
sys.modules["ipdb"] = m
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(REF, "deqmpc"))
torch.set_default_dtype(torch.float64)

from qpth import AL_mpc, al_utils  # noqa: E402
import envs  # noqa: E402  (deqmpc/envs.py)

ACTIVE_TOL, INACTIVE_MARGIN = 1e-3, 0.1


def activity(u, lo, hi):
    """-> (samples with a control within ACTIVE_TOL of a bound or beyond it, samples whose controls all stay
    INACTIVE_MARGIN inside the bounds)"""
    gap = np.minimum(hi - u, u - lo).min(axis=(1, 2))
    return gap <= ACTIVE_TOL, gap >= INACTIVE_MARGIN


def run_case(name, B, T, seed):
    env = envs.IntegratorEnv()
    nx, nu = env.nx, env.nu
    assert (nx, nu, env.dt, env.max_acc) == (2, 1, 0.1, 2)
    dyn, dyn_jac = env.dynamics, env.dynamics_derivatives
    u_upper = torch.tensor(env.action_space.high, dtype=torch.float64)
    u_lower = torch.tensor(env.action_space.low, dtype=torch.float64)
    rng = np.random.default_rng(seed)
    low = np.concatenate((np.full(env.nq, -2.0), np.full(env.nq, -env.max_vel)))       # envs.py:285
    x0 = rng.uniform(low=low, high=-low, size=(B, nx))
    x0[B // 2:] *= 0.01
    x0 = torch.tensor(x0)
    Qd = torch.cat([env.Qlqr.double(), env.Rlqr.double()]).repeat(B, T, 1)
    C = torch.diag_embed(Qd).requires_grad_()
    c = torch.zeros(B, T, nx + nu).requires_grad_()                                     # towards the origin
    u_init = torch.tensor(0.1 * rng.standard_normal((B, T, nu)))

    ctrl = AL_mpc.MPC(nx, nu, T, u_lower=u_lower, u_upper=u_upper, n_batch=B, verbose=0, u_init=u_init, al_iter=2,
                      solver_type="dense", dtype=torch.float64, eps=1e-5, exit_unconverged=False, backprop=False)
    ctrl.reinitialize(x0, torch.ones(B, T, 1))
    ctrl.u_init = u_init
    out = {}

    def state(tag):
        h = ctrl.cost_lam_hist
        out.update({"hist_cost" + tag: torch.stack([t.reshape(B) for t in h[0]]).detach().numpy(),
                    "hist_lam" + tag: torch.stack(list(h[1])).detach().numpy(),
                    "hist_rho" + tag: torch.stack([t.reshape(B) for t in h[2]]).detach().numpy(),
                    "lam" + tag: ctrl.lamda_prev.detach().numpy(), "rho" + tag: ctrl.rho_prev.detach().numpy()})

    x, u = ctrl(x0, al_utils.QuadCost(C, c), dyn, dyn_jac)
    (x.double().sum() + 2.0 * u.double().sum()).backward()
    out.update(x1=x.detach().numpy(), u1=u.detach().numpy(),
               dC1=C.grad.diagonal(dim1=-2, dim2=-1).numpy().copy(), dc1=c.grad.numpy().copy())
    state("1")
    # second call: warm start from the history and the previous x_init / u_init
    x2, u2 = ctrl(x0, al_utils.QuadCost(C.detach().clone(), c.detach().clone()), dyn, dyn_jac)
    out.update(x2=x2.detach().numpy(), u2=u2.detach().numpy())
    state("2")

    lo, hi = u_lower.numpy(), u_upper.numpy()
    for tag in ("u1", "u2"):
        act, inact = activity(out[tag].astype(np.float64), lo, hi)
        assert act.sum() >= 2 and inact.sum() >= 2, (tag, act, inact)
    ins = dict(x0=x0.numpy(), Qd=Qd.numpy(), c=c.detach().numpy(), u_lower=lo, u_upper=hi, u_init=u_init.numpy())
    arrs = {"in_" + k: v for k, v in ins.items()}
    arrs.update(out, dt=np.float64(env.dt))
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **arrs)
    assert not np.load(path, allow_pickle=False)["in_x0"].dtype.hasobject
    print("wrote %s %.1f KB  active %s  u1[:, 0]=%s rho1=%s" % (
        name, os.path.getsize(path) / 1024, activity(out["u1"].astype(np.float64), lo, hi)[0],
        out["u1"][:, 0].ravel(), ctrl.rho_prev.detach().numpy()[0]))


if __name__ == "__main__":
    run_case("INTEGRATOR_AL_b6", B=6, T=5, seed=0)
