#!/usr/bin/env python3
"""Golden vectors for AL_mpc.MPC with a caller's dynamics module at a WIDE knot (n_state 13, n_ctrl 4: n + m = 17),
produced by importing the reference (build container only; see make_golden.py for the ipdb stand-in).

Reference entry points exercised:
  qpth/AL_mpc.py:116-321      MPC.__init__/forward/al_solve, reinitialize (:432-438)
  qpth/al_utils.py:363-500    NewtonAL forward/backward (dense Jacobian, dense Hessian, Cholesky, line search)

The dynamics is the toy map of tests/test_gpu_al_given.py (CallerToy: x+ = x + dt (A x + 0.3 sin x + B u) with analytic
Jacobians), defined again here in plain torch so that this script needs nothing of the test suite; its matrices are
stored in the fixture and the test checks them against CallerToy's.

Stored: the inputs (x0, Q diagonal, c, bounds, x_init, u_init, A, Bm, dt), the outputs of two successive MPC.forward
calls (cold, then warm-started from the history), the solver state after each (lamda_prev, rho_prev) and the gradients
of the loss sum(x) + 2 sum(u) with respect to C's diagonal and c of both calls.  Arrays only.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("DQP_REFERENCE", "/root/reference")
m_ = types.ModuleType("ipdb")
def _st(*a, **k):
    raise RuntimeError("ipdb.set_trace() reached inside the reference")
m_.set_trace = _st
sys.modules["ipdb"] = m_
sys.path.insert(0, REF)
torch.set_default_dtype(torch.float64)

from qpth import AL_mpc, al_utils  # noqa: E402


class Toy(torch.nn.Module):
    def __init__(self, n, m, dt=0.05):
        super().__init__()
        g = torch.Generator().manual_seed(100 * n + m)
        self.dt = dt
        self.A = 0.3 * torch.randn(n, n, generator=g, dtype=torch.float64)
        self.Bm = torch.randn(n, m, generator=g, dtype=torch.float64)

    def forward(self, x, u):
        return x + self.dt * (x @ self.A.T + 0.3 * torch.sin(x) + u @ self.Bm.T)

    def jac(self, x, u):
        eye = torch.eye(x.shape[1], dtype=x.dtype)
        R = eye + self.dt * (self.A + 0.3 * torch.diag_embed(torch.cos(x)))
        return self.forward(x, u), (R, (self.dt * self.Bm).expand(x.shape[0], -1, -1))


def run_case(name, n, m, T, B, seed):
    rng = np.random.default_rng(seed)
    mod = Toy(n, m)
    nt = n + m
    x0 = torch.tensor(rng.standard_normal((B, n)))
    u_init = torch.tensor(0.2 * rng.standard_normal((B, T, m)))
    x_init = torch.empty(B, T, n)
    x_init[:, 0] = x0
    for t in range(T - 1):
        x_init[:, t + 1] = mod(x_init[:, t], u_init[:, t])
    Qd = torch.tensor(rng.random((B, T, nt)) + 0.1)
    c0 = torch.tensor(rng.standard_normal((B, T, nt)))
    u_lower, u_upper = torch.full((m,), -0.5), torch.full((m,), 0.5)

    ctrl = AL_mpc.MPC(n, m, T, u_lower=u_lower, u_upper=u_upper, n_batch=B, verbose=0, solver_type="dense",
                      dtype=torch.float64, eps=1e-5, exit_unconverged=False, backprop=False)
    ctrl.reinitialize(x0, torch.ones(B, T, 1))
    ctrl.x_init, ctrl.u_init = x_init.clone(), u_init.clone()
    out = {}
    for call in (1, 2):
        C = torch.diag_embed(Qd).requires_grad_()
        c = c0.clone().requires_grad_()
        x, u = ctrl(x0, al_utils.QuadCost(C, c), mod, mod.jac)
        (x.double().sum() + 2.0 * u.double().sum()).backward()
        out.update({"x%d" % call: x.detach().numpy(), "u%d" % call: u.detach().numpy(),
                    "lam%d" % call: ctrl.lamda_prev.detach().numpy().copy(),
                    "rho%d" % call: ctrl.rho_prev.detach().numpy().copy(),
                    "dC%d" % call: C.grad.diagonal(dim1=-2, dim2=-1).numpy().copy(), "dc%d" % call: c.grad.numpy().copy()})
    ins = dict(x0=x0.numpy(), Qd=Qd.numpy(), c=c0.numpy(), u_lower=u_lower.numpy(), u_upper=u_upper.numpy(),
               x_init=x_init.numpy(), u_init=u_init.numpy(), A=mod.A.numpy(), Bm=mod.Bm.numpy(), dt=np.float64(mod.dt))
    arrs = {"in_" + k: v for k, v in ins.items()}
    arrs.update(out)
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **arrs)
    print("wrote %s %.1f KB  x1[0,1,:2]=%s u1[0,0,:2]=%s rho1=%s rho2=%s" % (
        name, os.path.getsize(path) / 1024, out["x1"][0, 1, :2], out["u1"][0, 0, :2], out["rho1"].ravel(),
        out["rho2"].ravel()))


if __name__ == "__main__":
    run_case("ALW_n13_m4_T6_b3", n=13, m=4, T=6, B=3, seed=134)
