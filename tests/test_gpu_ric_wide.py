"""Wide stage-wise MPC QP kernels (the wide part of csrc/dqp_ric.hip: 16 < n_state + n_ctrl <= 32, one QP per 32-lane
half-wavefront) through the C ABI and qp_wrapper.MPC.

Checkers, as in test_gpu_ric.py: (1) assemble -> DenseQPFunction on the dense GPU kernels where the dense QP fits
(nz <= 512); (2) the CPU oracle on the QP assembled in numpy; (3) KKT properties at sizes no other path serves;
(4) the caller-stepped mode against the fused forward; (5) the reference's own qp_wrapper.MPC at n 13, m 4
(tests/golden/make_golden_ricw.py), LinDx and a caller's nonlinear module; (6) a 16-lane pair keeps its kernels.
Tolerances: zhat rtol 1e-6 / atol 1e-8, duals rtol 1e-5 / atol 1e-7, gradients rtol 1e-4 / atol 1e-6.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import oracle
from test_gpu_ric import assemble, dev, problem, run_fused
from test_gpu_round3 import _forward
from test_ric_wide_cpu import per_qp_doubles

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
ZT = dict(rtol=1e-6, atol=1e-8)
DT = dict(rtol=1e-5, atol=1e-7)
GT = dict(rtol=1e-4, atol=1e-6)


def _per_problem():
    from diff_qp_mpc_amd import qp as qpmod

    class Ctx:
        def __enter__(self):
            self.old, qpmod.TERMINATION = qpmod.TERMINATION, "per_problem"

        def __exit__(self, *a):
            qpmod.TERMINATION = self.old
    return Ctx()


@pytest.mark.parametrize("n,m,T,B", [(13, 4, 4, 3), (13, 4, 4, 37), (13, 4, 30, 1), (14, 7, 5, 37), (14, 7, 5, 1),
                                     (24, 8, 3, 3)])
def test_wide_equals_assemble_plus_dense_gpu(n, m, T, B):
    """Fused forward and backward (tau, dC, dc, dF, df, dx0) against assemble + DenseQPFunction on the dense GPU
    kernels (T 30 at (13, 4): nz 510, the blocked dense kernels), per-problem termination on both sides."""
    from diff_qp_mpc_amd import qp as qpmod, qp_wrapper, _lib
    data = problem(n, m, T, B, seed=n * 100 + T + B)
    with _per_problem():
        with _lib.trace(64) as tr:
            tau, grads, w = run_fused(n, m, T, data)
        names = [k for k, _ in tr.records]
        assert any("ric::forward_kernel" in k and "Cfg<%d, %d" % (n, m) in k for k in names), names
        assert any("ric::backward_kernel" in k and "Cfg<%d, %d" % (n, m) in k for k in names), names
        C, c, F, f, x0, lo, hi = data
        ins = [dev(a, grad=True) for a in (C, c, F, f, x0)]
        Q, p, G, h, A, b = qp_wrapper._AssembleDenseQP.apply(*ins, dev(lo), dev(hi), n, m, T)
        z = qpmod.DenseQPFunction(verbose=-1)(Q, p, G, h, A, b)
        (z.reshape(B, T, n + m) * dev(w)).sum().backward()
    np.testing.assert_allclose(tau.reshape(B, -1), z.detach().cpu().numpy(), **ZT)
    for a, t, k in zip(grads, ins, ("dC", "dc", "dF", "df", "dx0")):
        np.testing.assert_allclose(a, t.grad.cpu().numpy(), err_msg=k, **GT)


@pytest.mark.parametrize("n,m,T,B", [(13, 4, 6, 3), (24, 8, 4, 2), (14, 7, 5, 3)])
@pytest.mark.parametrize("batch_rule", [True, False])
def test_wide_vs_cpu_oracle(n, m, T, B, batch_rule):
    """Against the CPU oracle's DenseQPFunction restatement on the numpy-assembled QP: the batch-coupled rule (the
    default) exactly, the per-problem rule within the float tolerance of test_gpu_ric's batch-rule test."""
    data = problem(n, m, T, B, seed=7 * n + T)
    if batch_rule:
        tau, grads, w = run_fused(n, m, T, data)
    else:
        with _per_problem():
            tau, grads, w = run_fused(n, m, T, data)
    Q, p, G, h, A, b = assemble(*data)
    o = oracle.dense_forward(Q, p, G, h, A, b)
    np.testing.assert_allclose(tau.reshape(B, -1), o["zhat"], **(ZT if batch_rule else DT))
    og = oracle.dense_backward(o["K"], o["zhat"], o["lam"], o["nu"], w.reshape(B, -1))
    nt = n + m
    dC = np.stack([og["dQ"][:, t * nt:(t + 1) * nt, t * nt:(t + 1) * nt] for t in range(T)])
    dc = np.stack([og["dp"][:, t * nt:(t + 1) * nt] for t in range(T)])
    dF = np.stack([og["dA"][:, t * n:(t + 1) * n, t * nt:(t + 1) * nt] for t in range(T - 1)])
    df = np.stack([-og["db"][:, t * n:(t + 1) * n] for t in range(T - 1)])
    dx0 = og["db"][:, (T - 1) * n:]
    for a, want, k in zip(grads, (dC, dc, dF, df, dx0), ("dC", "dc", "dF", "df", "dx0")):
        np.testing.assert_allclose(a, want, err_msg=k, **GT)


@pytest.mark.parametrize("n,m,T,B,batch_rule", [(13, 4, 40, 1024, True), (24, 8, 30, 256, False)])
def test_wide_kkt_properties(n, m, T, B, batch_rule):
    """Sizes no other path serves (nz 680 / 960): stationarity, primal feasibility, complementarity and signs of
    the returned (tau, lam, nu, slack) on the original data."""
    from diff_qp_mpc_amd import _lib
    nt = n + m
    C, c, F, f, x0, lo, hi = problem(n, m, T, B, seed=3, spread=0.05)
    lib = _lib.load()
    dims = _lib.dqp_mpc_dims(B, n, m, T, 1, 0)
    assert lib.dqp_mpc_qp_supported(ctypes.byref(dims)) == 1
    opts = _lib.dqp_opts(1e-12, 1e-10, 20, 3, _lib.DQP_FLAG_BATCH_TERMINATION if batch_rule else 0, 0)
    t = [dev(a) for a in (C, c, F, f, x0, lo, hi)]
    kw = dict(dtype=torch.float64, device="cuda")
    tau = torch.empty(B, T, nt, **kw); lam = torch.empty(B, 2 * T * m, **kw); slack = torch.empty(B, 2 * T * m, **kw)
    nu = torch.empty(B, T * n, **kw); info = torch.empty(B, 2, dtype=torch.int32, device="cuda")
    ws = torch.empty(int(lib.dqp_mpc_qp_workspace_bytes(ctypes.byref(dims))) // 8, **kw)
    P = lambda x: ctypes.c_void_p(x.data_ptr())
    resid = torch.empty(B, **kw)
    tb = int(lib.dqp_mpc_qp_termination_bytes(ctypes.byref(dims), ctypes.byref(opts)))
    term = torch.empty(tb // 8 + 1, **kw) if tb else None
    rc = lib.dqp_mpc_qp_forward(ctypes.byref(dims), ctypes.byref(opts), *[P(x) for x in t], P(tau), P(lam), P(nu),
                                P(slack), P(info), P(resid), P(ws), P(term) if tb else None, None)
    assert rc == 0
    torch.cuda.synchronize()
    assert int(info[:, 0].abs().max()) == 0
    assert float(resid.max()) < 1e-8, "not converged: %s" % resid.topk(4).values.tolist()
    Ct, ct, Ft, ft, x0t = t[:5]
    tk = tau.transpose(0, 1)
    x, u = tk[..., :n], tk[..., n:]
    scale = float(tk.abs().max())
    dyn = (Ft @ tk[:-1].unsqueeze(-1)).squeeze(-1) + ft - x[1:]
    assert float(dyn.abs().max()) < 1e-8 * max(1.0, scale)
    assert float((x[0] - x0t).abs().max()) < 1e-9
    lu, ll = lam[:, :T * m].reshape(B, T, m).transpose(0, 1), lam[:, T * m:].reshape(B, T, m).transpose(0, 1)
    su, sl = slack[:, :T * m].reshape(B, T, m).transpose(0, 1), slack[:, T * m:].reshape(B, T, m).transpose(0, 1)
    assert float((u - dev(hi) + su).abs().max()) < 1e-8 and float((-u + dev(lo) + sl).abs().max()) < 1e-8
    assert float(lam.min()) > 0 and float(slack.min()) > 0
    assert float((lam * slack).max()) < 1e-8
    nuk = nu.reshape(B, T, n).transpose(0, 1)
    g = (Ct @ tk.unsqueeze(-1)).squeeze(-1) + ct
    g[..., n:] += lu - ll
    g[:-1] += (Ft.transpose(-1, -2) @ nuk[:-1].unsqueeze(-1)).squeeze(-1)
    g[1:, :, :n] -= nuk[:-1]
    g[0, :, :n] += nuk[-1]
    assert float(g.abs().max()) < 1e-7 * max(1.0, float(nu.abs().max()))


@pytest.mark.parametrize("n,m,T,B", [(13, 4, 6, 5), (24, 8, 4, 3)])
@pytest.mark.parametrize("batch_rule", [True, False])
def test_wide_stepped_forward_matches_fused(n, m, T, B, batch_rule):
    """dqp_mpc_qp_forward_stepped fed the linear residual of each iterate = the fused forward."""
    from diff_qp_mpc_amd import _lib
    lib = _lib.load()
    data = problem(n, m, T, B, seed=7 + n)
    flags = _lib.DQP_FLAG_STAGEWISE | (_lib.DQP_FLAG_BATCH_TERMINATION if batch_rule else 0)
    a = _forward(lib, _lib, n, m, T, data, flags)
    b = _forward(lib, _lib, n, m, T, data, flags, stepped=True)
    torch.cuda.synchronize()
    assert int(a["info"][:, 0].abs().max()) == 0 and int(b["info"][:, 0].abs().max()) == 0
    np.testing.assert_allclose(b["tau"].cpu().numpy(), a["tau"].cpu().numpy(), **ZT)
    for k in ("lam", "nu", "slack"):
        np.testing.assert_allclose(b[k].cpu().numpy(), a[k].cpu().numpy(), **DT)
    if batch_rule:
        assert int(b["info"][:, 1].min()) == int(a["info"][:, 1].min())


@pytest.mark.parametrize("tag,kw", [("single", dict(single_qp_solve=True)), ("sqp", dict(qp_iter=3))])
def test_mpc_lindx_vs_reference_n13_m4(tag, kw):
    """qp_wrapper.MPC with LinDx at n 13, m 4, T 6 (nz 102: no dense kernel of the fused path) against the
    reference's own qp_wrapper.MPC: x, u and the gradients wrt C, c, F, f, x0."""
    from diff_qp_mpc_amd.qp_wrapper import MPC, QuadCost, LinDx
    g = dict(np.load(os.path.join(GOLDEN, "RICW_n13_m4_T6_b3.npz"), allow_pickle=False))
    B, n, m, T = g["in_x0"].shape[0], 13, 4, 6
    C, c, F, f, x0 = [dev(g["in_" + k], grad=True) for k in ("C", "c", "F", "f", "x0")]
    mpc = MPC(n, m, T, u_lower=dev(g["in_u_lower"]), u_upper=dev(g["in_u_upper"]), n_batch=B, verbose=-1, **kw)
    x, u = mpc(x0, QuadCost(C, c), LinDx(F, f), None)
    np.testing.assert_allclose(x.detach().cpu().numpy(), g["%s_x" % tag], **ZT)
    np.testing.assert_allclose(u.detach().cpu().numpy(), g["%s_u" % tag], **ZT)
    (x.sum() + 2.0 * u.sum()).backward()
    for k, t in (("C", C), ("c", c), ("F", F), ("f", f), ("x0", x0)):
        got = t.grad.cpu().numpy() if t.grad is not None else np.zeros(t.shape)
        np.testing.assert_allclose(got, g["%s_d%s" % (tag, k)], err_msg="%s d%s" % (tag, k), **GT)


class WideToy(torch.nn.Module):
    """x+ = x + dt (A x + 0.3 sin(x) + B u) -- restated from tests/golden/make_golden_ricw.py"""

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


def test_mpc_caller_module_vs_reference_n13_m4():
    """A caller's nonlinear torch module at n 13, m 4 (n + m = 17): the residual closure is evaluated once per PDIPM
    iteration around the wide stage-wise kernels (dqp_mpc_qp_forward_stepped) instead of NotImplementedError.
    Against the reference's qp_wrapper.MPC on the same module: x, u rtol 1e-5 / atol 1e-7, dC, dc as gradients."""
    from diff_qp_mpc_amd import qp_wrapper, _lib
    g = dict(np.load(os.path.join(GOLDEN, "RICWNL_n13_m4_T5_b3.npz"), allow_pickle=False))
    B, n, m, T = g["in_x0"].shape[0], 13, 4, 5
    C, c = dev(g["in_C"], grad=True), dev(g["in_c"], grad=True)
    dx = WideToy(n, m)
    mpc = qp_wrapper.MPC(n, m, T, u_lower=dev(g["in_u_lower"]), u_upper=dev(g["in_u_upper"]), n_batch=B, verbose=-1,
                         single_qp_solve=True)
    with _lib.trace(4096) as tr:
        x, u = mpc(dev(g["in_x0"]), qp_wrapper.QuadCost(C, c), dx, dx.jac)
        torch.cuda.synchronize()
    # the caller-residual instantiation (RES_CALLER = 2) of the wide pair
    assert any("forward_kernel<dqp::ric::Cfg<13, 4, false>, 2>" in k for k, _ in tr.records), [k for k, _ in tr.records]
    np.testing.assert_allclose(x.detach().cpu().numpy(), g["single_x"], **DT)
    np.testing.assert_allclose(u.detach().cpu().numpy(), g["single_u"], **DT)
    (x.sum() + 2.0 * u.sum()).backward()
    np.testing.assert_allclose(C.grad.cpu().numpy(), g["single_dC"], err_msg="dC", **GT)
    np.testing.assert_allclose(c.grad.cpu().numpy(), g["single_dc"], err_msg="dc", **GT)


def test_sixteen_lane_pair_keeps_its_kernels():
    """(12, 4) at T 30: the 16-lane kernels, its workspace size unchanged, no wide kernel launched."""
    from diff_qp_mpc_amd import _lib
    n, m, T, B = 12, 4, 30, 6
    lib = _lib.load()
    dims = _lib.dqp_mpc_dims(B, n, m, T, 1, 0)
    assert lib.dqp_mpc_qp_workspace_bytes(ctypes.byref(dims)) == 8 * 8 * per_qp_doubles(n, m, T)     # B 6 -> 8
    data = problem(n, m, T, B, seed=2, spread=0.05)
    with _lib.trace(64) as tr:
        run_fused(n, m, T, data)
        torch.cuda.synchronize()
    names = [k for k, _ in tr.records]
    assert any("ric::forward_kernel" in k and "Cfg<12, 4" in k for k in names), names
    assert not any(any("Cfg<%d, %d" % p in k for p in ((13, 4), (14, 7), (24, 8))) for k in names), names
