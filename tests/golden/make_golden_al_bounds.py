#!/usr/bin/env python3
"""Golden vectors for AL_mpc.MPC with PER-SAMPLE, PER-KNOT control bounds, produced by importing the reference (build
container only; see make_golden.py for the ipdb stand-in).

Reference entry points exercised:
  deqmpc/envs.py:5-82             PendulumDynamics / PendulumDynamics_jac (semi-implicit Euler), PendulumEnv
  qpth/AL_mpc.py:116-321          MPC.__init__/forward/al_solve, reinitialize (:432-438)
  qpth/al_utils.py:266-271        dyn_res_ineq: u - u_upper, u_lower - u by broadcasting against u (B, T, n_ctrl)
  qpth/al_utils.py:363-500        NewtonAL forward/backward

B = 6, T = 5, al_iter = 2, the pendulum fixtures' cost (make_golden_al.py).  The bounds are (B, T, n_ctrl) arrays:
+-limit[b] * fade[t] with the env's limit scaled per sample and faded linearly to 20 % along the horizon, so that a
control that saturates early is released later (or the other way round).  The script asserts that at least two samples
have a bound active at some knots and inactive at others and at least one sample has no active bound, in both calls.

The reference takes bounds that vary along the horizon, but not bounds that vary over a batch: its line search folds the
20 candidates into the batch axis (al_utils.py:503-527) and dyn_res_ineq (:266-271) then subtracts (B, T, n_ctrl) bounds
from a (20 B, T, n_ctrl) control -- a shape error for B > 1.  Every problem of an AL_mpc.MPC call is solved on its own
(residuals, merit, line search, multipliers and penalty are per sample; only a failed Cholesky factorisation switches the
whole batch, and none fails here), so the script runs the reference ONCE PER SAMPLE at n_batch = 1 with that sample's
(1, T, n_ctrl) bounds, which broadcast, and stacks the results: the golden is what the reference computes for each of the
B problems.

Stored: the fields of make_golden_integrator.py -- the inputs, then for the cold call (reinitialize + forward) and the
warm call from the stored state: x, u, the cost_lam_hist rows (oldest first), lamda_prev, rho_prev; for the cold call the
gradients wrt C's diagonal and c of the loss sum(x) + 2 sum(u).

The file is BOUNDS_AL_pendulum_T5_b6.npz, not AL_*.npz: tests/test_gpu_al.py and tests/test_oracle_golden.py take every
AL_*.npz for a vector-bound fixture of make_golden_al.py.
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

ACTIVE_TOL, INACTIVE_MARGIN = 1e-3, 0.02


def activity(u, lo, hi):
    """per (sample, knot): a control within ACTIVE_TOL of its bound or beyond it / all controls INACTIVE_MARGIN inside.
    -> (samples with both kinds of knot, samples whose knots are all of the second kind)"""
    gap = np.minimum(hi - u, u - lo).min(axis=2)
    act, inact = gap <= ACTIVE_TOL, gap >= INACTIVE_MARGIN
    return act.any(1) & inact.any(1), inact.all(1)


def make_bounds(limit, B, T, nu):
    """+-limit * scale[b] * fade[t]: per-sample scales between 15 % and 100 %, the horizon fading linearly to 20 %"""
    scale = np.linspace(0.15, 1.0, B)[:, None, None]
    fade = np.linspace(1.0, 0.2, T)[None, :, None]
    hi = np.asarray(limit, dtype=np.float64).reshape(1, 1, nu) * scale * fade
    return -hi, hi


def solve_batch(nx, nu, T, x0, Qd, c0, u_init, lo, hi, dyn, dyn_jac):
    """two AL_mpc.MPC calls of the reference on the batch it is given -> dict of numpy results"""
    B = x0.shape[0]
    u_lower, u_upper = torch.tensor(lo), torch.tensor(hi)
    C = torch.diag_embed(Qd).requires_grad_()
    c = c0.clone().requires_grad_()
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
    x2, u2 = ctrl(x0, al_utils.QuadCost(C.detach().clone(), c.detach().clone()), dyn, dyn_jac)
    out.update(x2=x2.detach().numpy(), u2=u2.detach().numpy())
    state("2")
    return out


# axis of the sample in each stored field
BATCH_AXIS = {"hist_cost": 1, "hist_lam": 1, "hist_rho": 1}


def run_case(name, B, T, seed):
    g = torch.Generator().manual_seed(seed)
    env = envs.PendulumEnv(stabilization=False)
    nx, nu = env.nx, env.nu
    dyn, dyn_jac = env.dynamics, env.dynamics_derivatives
    lo, hi = make_bounds(env.action_space.high, B, T, nu)
    x0 = torch.stack([3.0 * (torch.rand(B, generator=g) - 0.5), torch.rand(B, generator=g) - 0.5], 1)
    x0[-1] *= 0.01                  # one sample next to the target: its controls stay off every bound
    Qd = torch.cat([torch.tensor([10.0, 1.0]), torch.tensor([0.01])]).repeat(B, T, 1)
    c = torch.zeros(B, T, nx + nu)                      # towards the origin
    u_init = 0.01 * torch.randn(B, T, nu, generator=g)
    # the reference, one sample at a time (see the module docstring)
    per = [solve_batch(nx, nu, T, x0[b:b + 1], Qd[b:b + 1], c[b:b + 1], u_init[b:b + 1], lo[b:b + 1], hi[b:b + 1], dyn, dyn_jac)
           for b in range(B)]
    out = {k: np.concatenate([p[k] for p in per], axis=BATCH_AXIS.get(k.rstrip("12"), 0)) for k in per[0]}
    for tag in ("u1", "u2"):
        mixed, free = activity(out[tag].astype(np.float64), lo, hi)
        assert mixed.sum() >= 2 and free.sum() >= 1, (tag, mixed, free)
    ins = dict(x0=x0.numpy(), Qd=Qd.numpy(), c=c.numpy(), u_lower=lo, u_upper=hi, u_init=u_init.numpy())
    arrs = {"in_" + k: v for k, v in ins.items()}
    arrs.update(out, dt=np.float64(env.dt))
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **arrs)
    assert not np.load(path, allow_pickle=False)["in_x0"].dtype.hasobject
    print("wrote %s %.1f KB  mixed %s free %s\nu1=%s\nhi=%s" % (
        name, os.path.getsize(path) / 1024, *activity(out["u1"].astype(np.float64), lo, hi), out["u1"][..., 0], hi[..., 0]))


if __name__ == "__main__":
    run_case("BOUNDS_AL_pendulum_T5_b6", B=6, T=5, seed=0)
