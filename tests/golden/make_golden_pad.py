#!/usr/bin/env python3
"""Golden vectors for padded stage-wise MPC QPs (dqp_mpc_dims.n_state_host): the reference's qp_wrapper.MPC at
(n_state, n_ctrl) pairs without stage-wise kernels of their own.  Build container only (imports the reference).

  PADNL_n5_m3_T6_b3     a caller's nonlinear torch module (WideToy of make_golden_ricw.py at n 5, m 3; host 6),
                        single-QP and SQP (qp_iter 3): x, u and the gradients wrt C, c
  PADNL_n17_m3_T5_b3    the same module at n 17, m 3 (host 29, a wide host-only pair), single-QP
  PAD_n7_m1_T80_b2      LinDx at n 7, m 1, T 80 (nz 640: beyond the dense kernels; host 8), single-QP:
                        x, u and the gradients wrt C, c, F, f, x0

Usage:  python tests/golden/make_golden_pad.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_ricw import WideToy, qp_wrapper  # noqa: E402  (sets up the reference import)
from make_golden_ric import family  # noqa: E402


def run_module(name, B, n, m, T, seed, tags):
    md = family(seed, B, n, m, T)
    dx = WideToy(n, m)
    outs = {"in_" + k: md[k].numpy() for k in ("C", "c", "x0", "u_lower", "u_upper")}
    for tag, kw in tags:
        C, c = md["C"].clone().requires_grad_(), md["c"].clone().requires_grad_()
        mpc = qp_wrapper.MPC(n, m, T, u_lower=md["u_lower"], u_upper=md["u_upper"], n_batch=B, verbose=-1, **kw)
        x, u = mpc(md["x0"], qp_wrapper.QuadCost(C, c), dx, dx.jac)
        (x.sum() + 2.0 * u.sum()).backward()
        outs.update({tag + "_x": x.detach().numpy(), tag + "_u": u.detach().numpy(), tag + "_dC": C.grad.numpy(),
                     tag + "_dc": c.grad.numpy()})
        print(name, tag, "|u| max %.3f" % float(u.abs().max()), "share on a bound %.2f" % float((u.abs() > 0.4999).double().mean()))
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **outs)


def run_lindx(name, B, n, m, T, seed):
    md = family(seed, B, n, m, T)
    outs = {"in_" + k: v.numpy() for k, v in md.items()}
    ins = {k: md[k].clone().requires_grad_() for k in ("C", "c", "F", "f", "x0")}
    mpc = qp_wrapper.MPC(n, m, T, u_lower=md["u_lower"], u_upper=md["u_upper"], n_batch=B, verbose=-1,
                         single_qp_solve=True)
    x, u = mpc(ins["x0"], qp_wrapper.QuadCost(ins["C"], ins["c"]), qp_wrapper.LinDx(ins["F"], ins["f"]), None)
    (x.sum() + 2.0 * u.sum()).backward()
    outs.update(single_x=x.detach().numpy(), single_u=u.detach().numpy())
    for k, t in ins.items():
        outs["single_d%s" % k] = t.grad.numpy() if t.grad is not None else np.zeros(t.shape)
    print(name, "|u| max %.3f" % float(u.abs().max()), "share on a bound %.2f" % float((u.abs() > 0.4999).double().mean()))
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **outs)


if __name__ == "__main__":
    run_module("PADNL_n5_m3_T6_b3", 3, 5, 3, 6, seed=21,
               tags=(("single", dict(single_qp_solve=True)), ("sqp", dict(qp_iter=3))))
    run_module("PADNL_n17_m3_T5_b3", 3, 17, 3, 5, seed=22, tags=(("single", dict(single_qp_solve=True)),))
    run_lindx("PAD_n7_m1_T80_b2", 2, 7, 1, 80, seed=23)
