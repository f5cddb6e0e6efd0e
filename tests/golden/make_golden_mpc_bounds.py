#!/usr/bin/env python3
"""Golden vectors for per-sample, per-knot control bounds on qp_wrapper.MPC: the reference's qp_wrapper.MPC with LinDx
dynamics at n_state 3, n_ctrl 1, T 6, B 6, single_qp_solve=True, with bounds that differ for every (knot, sample, control).

The reference's class docstring promises bounds "shaped as [T, n_batch, n_ctrl]", but its compute_Gh_dense
(qp_wrapper.py:664-679) builds h from an (n_ctrl,) vector.  The box enters the solver only as h, so the instance's
compute_Gh_dense is wrapped here by a function of ours that keeps the reference's G and overwrites h with
[upper (T m, knot-major) ; -lower (T m)] per sample; everything else -- assembly of Q, p, A, b, the PDIPM, the line
search and the backward -- is the reference's.  Recorded: the inputs, x, u and the gradients wrt C, c, F, f, x0, as
make_golden_ric.py does.  Build container only (imports the reference).

Bounds: mid +- half with mid ~ U(-0.3, 0.3), half ~ U(0.05, 0.5) drawn per element from np.random.default_rng; the rest
of the problem as tests/test_gpu_ric.py::problem.  The script asserts the property the tests rely on: every sample has a
bound row that is active (gap <= 1e-6) and one that is not (gap >= 0.02).

Usage:  DQP_REFERENCE=<reference checkout> python tests/golden/make_golden_mpc_bounds.py
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ["DQP_REFERENCE"]        # a checkout of the reference project
m_ = types.ModuleType("ipdb")
def _st(*a, **k):
    raise RuntimeError("ipdb.set_trace() reached inside the reference")
m_.set_trace = _st
sys.modules["ipdb"] = m_
sys.path.insert(0, REF)
torch.set_default_dtype(torch.float64)
from qpth import qp_wrapper  # noqa: E402


def family(seed, B, n, m, T, active=0.4, spread=0.15):
    rng = np.random.default_rng(seed)
    nt = n + m
    L = rng.standard_normal((T, B, nt, nt)) * 0.3
    C = L @ L.transpose(0, 1, 3, 2) + np.eye(nt)
    c = rng.standard_normal((T, B, nt))
    F = np.concatenate([np.eye(n) + spread * rng.standard_normal((T - 1, B, n, n)),
                        0.5 * rng.standard_normal((T - 1, B, n, m))], axis=-1)
    f = 0.1 * rng.standard_normal((T - 1, B, n))
    x0 = rng.standard_normal((B, n))
    mid = rng.uniform(-0.3, 0.3, (T, B, m))
    half = rng.uniform(0.05, 0.5, (T, B, m))
    return dict(C=C, c=c, F=F, f=f, x0=x0, u_lower=mid - half, u_upper=mid + half)


def run(name, B, n, m, T, seed):
    md = {k: torch.tensor(v) for k, v in family(seed, B, n, m, T).items()}
    outs = {"in_" + k: v.numpy() for k, v in md.items()}
    ins = {k: md[k].clone().requires_grad_() for k in ("C", "c", "F", "f", "x0")}
    # the constructor's vector bounds only size G; h is replaced below
    mpc = qp_wrapper.MPC(n, m, T, u_lower=-torch.ones(m), u_upper=torch.ones(m), n_batch=B, verbose=-1, single_qp_solve=True)
    ref_Gh = mpc.compute_Gh_dense
    hi = md["u_upper"].permute(1, 0, 2).reshape(B, T * m)          # (B, T m), knot-major rows
    lo = md["u_lower"].permute(1, 0, 2).reshape(B, T * m)

    def Gh_with_bounds(x0):
        G, h = ref_Gh(x0)
        return G, torch.cat([hi, -lo], dim=1).to(h)
    mpc.compute_Gh_dense = Gh_with_bounds
    x, u = mpc(ins["x0"], qp_wrapper.QuadCost(ins["C"], ins["c"]), qp_wrapper.LinDx(ins["F"], ins["f"]), None)
    (x.sum() + 2.0 * u.sum()).backward()
    outs["single_x"] = x.detach().numpy()
    outs["single_u"] = u.detach().numpy()
    for k, t in ins.items():
        outs["single_d%s" % k] = t.grad.numpy() if t.grad is not None else np.zeros(t.shape)
    gap = np.minimum(outs["in_u_upper"] - outs["single_u"], outs["single_u"] - outs["in_u_lower"])     # (T, B, m)
    per_sample = gap.transpose(1, 0, 2).reshape(B, -1)
    print(name, "min gap per sample", per_sample.min(1), "max gap per sample", per_sample.max(1))
    assert (per_sample.min(1) <= 1e-6).all() and (per_sample.max(1) >= 0.02).all(), "golden without an active and an inactive row"
    assert (gap > -1e-9).all()
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **outs)


if __name__ == "__main__":
    run("MPCB_n3_m1_T6_b6", 6, 3, 1, 6, seed=5)      # a seed at which the assertion above holds for all six samples
