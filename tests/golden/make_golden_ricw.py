#!/usr/bin/env python3
"""Golden vectors for the wide stage-wise MPC QP kernels (16 < n_state + n_ctrl <= 32): the reference's
qp_wrapper.MPC at n_state 13, n_ctrl 4 (the quaternion-quadrotor shape BASELINE config 4 quotes).
Build container only (imports the reference).

  RICW_n13_m4_T6_b3     LinDx dynamics (family of make_golden_ric.py), single-QP and SQP (qp_iter 3):
                        x, u and the gradients wrt C, c, F, f, x0
  RICWNL_n13_m4_T5_b3   a caller's nonlinear torch module (WideToy below, not a registered model), single-QP:
                        x, u and the gradients wrt C, c

Usage:  python tests/golden/make_golden_ricw.py
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
sys.path.insert(0, HERE)
torch.set_default_dtype(torch.float64)
from qpth import qp_wrapper  # noqa: E402
from make_golden_ric import family  # noqa: E402


class WideToy(torch.nn.Module):
    """x+ = x + dt (A x + 0.3 sin(x) + B u): smooth, nonlinear, 13 states and 4 controls.  Restated verbatim in
    tests/test_gpu_ric_wide.py."""

    def __init__(self, n=13, m=4, dt=0.05):
        super().__init__()
        g = torch.Generator().manual_seed(1234)
        self.dt = dt
        self.A = 0.3 * torch.randn(n, n, generator=g, dtype=torch.float64)
        self.Bm = torch.randn(n, m, generator=g, dtype=torch.float64)

    def forward(self, x, u):
        A, Bm = self.A.to(x), self.Bm.to(x)
        return x + self.dt * (x @ A.T + 0.3 * torch.sin(x) + u @ Bm.T)

    def jac(self, x, u):
        A, Bm = self.A.to(x), self.Bm.to(x)
        eye = torch.eye(x.shape[1], dtype=x.dtype, device=x.device)
        R = eye + self.dt * (A + 0.3 * torch.diag_embed(torch.cos(x)))
        S = (self.dt * Bm).expand(x.shape[0], -1, -1)
        return None, (R, S)


def run_lindx(name, B, n, m, T, seed):
    md = family(seed, B, n, m, T)
    outs = {"in_" + k: v.numpy() for k, v in md.items()}
    for tag, kw in (("single", dict(single_qp_solve=True)), ("sqp", dict(qp_iter=3))):
        ins = {k: md[k].clone().requires_grad_() for k in ("C", "c", "F", "f", "x0")}
        mpc = qp_wrapper.MPC(n, m, T, u_lower=md["u_lower"], u_upper=md["u_upper"], n_batch=B, verbose=-1, **kw)
        x, u = mpc(ins["x0"], qp_wrapper.QuadCost(ins["C"], ins["c"]), qp_wrapper.LinDx(ins["F"], ins["f"]), None)
        (x.sum() + 2.0 * u.sum()).backward()
        outs["%s_x" % tag] = x.detach().numpy()
        outs["%s_u" % tag] = u.detach().numpy()
        for k, t in ins.items():
            outs["%s_d%s" % (tag, k)] = t.grad.numpy() if t.grad is not None else np.zeros(t.shape)
        print(name, tag, "|u| max %.3f" % float(u.abs().max()), "share on a bound %.2f" % float((u.abs() > 0.4999).double().mean()))
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **outs)


def run_module(name, B, n, m, T, seed):
    md = family(seed, B, n, m, T)
    dx = WideToy(n, m)
    outs = {"in_" + k: md[k].numpy() for k in ("C", "c", "x0", "u_lower", "u_upper")}
    C, c = md["C"].clone().requires_grad_(), md["c"].clone().requires_grad_()
    mpc = qp_wrapper.MPC(n, m, T, u_lower=md["u_lower"], u_upper=md["u_upper"], n_batch=B, verbose=-1,
                         single_qp_solve=True)
    x, u = mpc(md["x0"], qp_wrapper.QuadCost(C, c), dx, dx.jac)
    (x.sum() + 2.0 * u.sum()).backward()
    outs.update(single_x=x.detach().numpy(), single_u=u.detach().numpy(), single_dC=C.grad.numpy(),
                single_dc=c.grad.numpy())
    print(name, "|u| max %.3f" % float(u.abs().max()), "share on a bound %.2f" % float((u.abs() > 0.4999).double().mean()))
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **outs)


if __name__ == "__main__":
    run_lindx("RICW_n13_m4_T6_b3", 3, 13, 4, 6, seed=13)
    run_module("RICWNL_n13_m4_T5_b3", 3, 13, 4, 5, seed=14)
