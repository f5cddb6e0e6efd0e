"""Padded stage-wise MPC QPs (dqp_mpc_dims.n_state_host, csrc/dqp_ric_pad.hip, the host parts of csrc/dqp_ric.hip): a problem
(n, m) solved by the kernels of a compiled pair (n', m) with n' - n dummy states.

Checkers: (1) on compiled pairs, the padded solve against the native one (both termination rules, partial
wavefronts); (2) at pairs without kernels of their own, the CPU oracle on the numpy-assembled QP; (3) KKT properties
at sizes beyond the dense route; (4) the reference's own qp_wrapper.MPC (tests/golden/make_golden_pad.py), a caller's
nonlinear module and LinDx at T 80; (5) the padded stepped mode against the padded fused forward; (6) a shape the
dense route serves keeps it.  Tolerances of test_gpu_ric_wide.py.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import oracle
from test_gpu_ric import assemble, dev, problem
from test_gpu_ric_wide import DT, GT, ZT, WideToy, _per_problem

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def capi_solve(n, m, T, data, host, batch_rule, w, stepped=False):
    """Forward (fused, or stepped with the linear residual computed in torch) and backward through the C ABI at
    dqp_mpc_dims.n_state_host = host (0: the native kernels, DQP_FLAG_STAGEWISE).  Returns the outputs and gradients."""
    from diff_qp_mpc_amd import _lib
    lib = _lib.load()
    C, c, F, f, x0, lo, hi = [dev(a) for a in data]
    B, nt = x0.shape[0], n + m
    dims = _lib.dqp_mpc_dims(B, n, m, T, 1, 0, host)
    flags = _lib.DQP_FLAG_STAGEWISE | (_lib.DQP_FLAG_BATCH_TERMINATION if batch_rule else 0)
    opts = _lib.dqp_opts(1e-12, 1e-10, 20, 3, flags, 0)
    kw = dict(dtype=torch.float64, device="cuda")
    o = dict(tau=torch.empty(B, T, nt, **kw), lam=torch.empty(B, 2 * T * m, **kw), nu=torch.empty(B, T * n, **kw),
             slack=torch.empty(B, 2 * T * m, **kw), info=torch.empty(B, 2, dtype=torch.int32, device="cuda"),
             resid=torch.empty(B, **kw))
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ins = [_p(t) for t in (C, c, F, f, x0, lo, hi)]
    outs = [_p(o[k]) for k in ("tau", "lam", "nu", "slack", "info", "resid")]
    if stepped:
        ws = torch.empty(int(lib.dqp_mpc_qp_stepped_workspace_bytes(ctypes.byref(dims))) // 8, **kw)
        tb = int(lib.dqp_mpc_qp_stepped_termination_bytes(ctypes.byref(dims), ctypes.byref(opts)))
    else:
        ws = torch.empty(int(lib.dqp_mpc_qp_workspace_bytes(ctypes.byref(dims))) // 8, **kw)
        tb = int(lib.dqp_mpc_qp_termination_bytes(ctypes.byref(dims), ctypes.byref(opts)))
    assert ws.numel() > 0
    term = torch.empty(tb // 8 + 1, **kw)
    if not stepped:
        assert lib.dqp_mpc_qp_forward(ctypes.byref(dims), ctypes.byref(opts), *ins, *outs, _p(ws), _p(term), st) == 0
    else:
        call = lambda ry, a, b: lib.dqp_mpc_qp_forward_stepped(ctypes.byref(dims), ctypes.byref(opts), *ins, _p(ry), a, b,
                                                               *outs, _p(ws), _p(term), st)
        assert call(None, 0, 0) == 0
        for it in range(20):
            tau = o["tau"]
            pred = torch.matmul(F.transpose(0, 1), tau[:, :-1, :, None])[..., 0] + f.transpose(0, 1)
            ry = torch.cat(((pred - tau[:, 1:, :n]).reshape(B, -1), tau[:, 0, :n] - x0), 1).contiguous()
            assert call(ry, it, it + 1) == 0
    g = [torch.full(a.shape, float("nan"), **kw) for a in (C, c, F, f, x0)]
    bo = _lib.dqp_opts(0.0, 0.0, 0, 0, _lib.DQP_FLAG_DENSE_BACKWARD | _lib.DQP_FLAG_STAGEWISE, 0)
    rc = lib.dqp_mpc_qp_backward(ctypes.byref(dims), ctypes.byref(bo), _p(C), _p(F), _p(o["tau"]), _p(o["lam"]),
                                 _p(o["nu"]), _p(o["slack"]), _p(dev(w)), *[_p(t) for t in g], _p(None), _p(ws), st)
    assert rc == 0
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in o.items()}
    res.update({k: t.cpu().numpy() for k, t in zip(("dC", "dc", "dF", "df", "dx0"), g)})
    return res


def _weights(B, T, nt):
    return np.linspace(0.5, 1.5, B * T * nt).reshape(B, T, nt)


@pytest.mark.parametrize("n,m,host,T", [(3, 1, 4, 6), (3, 1, 8, 6), (3, 3, 6, 6), (12, 4, 28, 5), (13, 4, 28, 5)])
@pytest.mark.parametrize("B", [1, 5, 37])
@pytest.mark.parametrize("batch_rule", [True, False])
def test_padded_equals_native(n, m, host, T, B, batch_rule):
    """A compiled pair on a larger host ((12, 4) -> 28: 16-lane to wide; (13, 4) -> 28: wide to wide) against its own
    kernels: tau, lam, nu, slack, the five gradients and the status."""
    from diff_qp_mpc_amd import _lib
    data = problem(n, m, T, B, seed=31 * n + host + B)
    w = _weights(B, T, n + m)
    a = capi_solve(n, m, T, data, 0, batch_rule, w)
    with _lib.trace(256) as tr:
        b = capi_solve(n, m, T, data, host, batch_rule, w)
    names = [k for k, _ in tr.records]
    assert any("ric::forward_kernel" in k and "Cfg<%d, %d" % (host, m) in k for k in names), names
    assert any("ric::backward_kernel" in k and "Cfg<%d, %d" % (host, m) in k for k in names), names
    assert any("pad_copy_kernel" in k for k in names), names
    assert not any("Cfg<%d, %d," % (n, m) in k for k in names), names
    np.testing.assert_array_equal(b["info"][:, 0], a["info"][:, 0])
    if batch_rule:      # the batch's stop (which converged iterate counts as best may differ at round-off level)
        assert int(b["info"][:, 1].min()) == int(a["info"][:, 1].min())
    np.testing.assert_allclose(b["tau"], a["tau"], **ZT)
    for k in ("lam", "nu", "slack"):
        np.testing.assert_allclose(b[k], a[k], err_msg=k, **DT)
    for k in ("dC", "dc", "dF", "df", "dx0"):
        np.testing.assert_allclose(b[k], a[k], err_msg=k, **GT)


# every host-only pair serves at least one of these (host in the comment)
UNCOMPILED = [(7, 1, 5), (5, 3, 6), (9, 2, 5), (11, 1, 6), (5, 5, 4), (7, 6, 5), (3, 8, 4), (17, 3, 4), (20, 5, 4),
              (9, 8, 4),
              (13, 2, 5),     # 14
              (7, 3, 5),      # 13
              (2, 7, 5),      # 9
              (16, 1, 4),     # 31
              (16, 2, 4),     # 30
              (15, 4, 4),     # 28
              (11, 6, 4),     # 26
              (15, 7, 4)]     # 25


@pytest.mark.parametrize("n,m,T", UNCOMPILED)
@pytest.mark.parametrize("batch_rule", [True, False])
def test_uncompiled_pairs_vs_cpu_oracle(n, m, T, batch_rule):
    """qp_wrapper._MPCQP on the host the library names, against the CPU oracle's DenseQPFunction on the
    numpy-assembled QP: the batch rule within ZT, the per-problem rule within DT; gradients within GT."""
    from diff_qp_mpc_amd import qp_wrapper, _lib
    B = 3
    data = problem(n, m, T, B, seed=5 * n + 11 * m + T)
    assert not qp_wrapper._MPCQP.supported(B, n, m, T)
    host = qp_wrapper._MPCQP.host_n_state(B, n, m, T)
    assert host > n
    ins = [dev(a, grad=True) for a in data[:5]]
    w = torch.tensor(_weights(B, T, n + m), dtype=torch.float64, device="cuda")
    with _lib.trace(256) as tr:
        if batch_rule:
            tau = qp_wrapper._MPCQP.apply(*ins, dev(data[5]), dev(data[6]), n, m, T, None, host)
        else:
            with _per_problem():
                tau = qp_wrapper._MPCQP.apply(*ins, dev(data[5]), dev(data[6]), n, m, T, None, host)
        (tau * w).sum().backward()
        torch.cuda.synchronize()
    assert any("Cfg<%d, %d" % (host, m) in k for k, _ in tr.records)
    Q, p, G, h, A, b = assemble(*data)
    o = oracle.dense_forward(Q, p, G, h, A, b)
    np.testing.assert_allclose(tau.detach().cpu().numpy().reshape(B, -1), o["zhat"], **(ZT if batch_rule else DT))
    og = oracle.dense_backward(o["K"], o["zhat"], o["lam"], o["nu"], w.cpu().numpy().reshape(B, -1))
    nt = n + m
    dC = np.stack([og["dQ"][:, t * nt:(t + 1) * nt, t * nt:(t + 1) * nt] for t in range(T)])
    dc = np.stack([og["dp"][:, t * nt:(t + 1) * nt] for t in range(T)])
    dF = np.stack([og["dA"][:, t * n:(t + 1) * n, t * nt:(t + 1) * nt] for t in range(T - 1)])
    df = np.stack([-og["db"][:, t * n:(t + 1) * n] for t in range(T - 1)])
    dx0 = og["db"][:, (T - 1) * n:]
    for t, want, k in zip(ins, (dC, dc, dF, df, dx0), ("dC", "dc", "dF", "df", "dx0")):
        np.testing.assert_allclose(t.grad.cpu().numpy(), want, err_msg=k, **GT)


@pytest.mark.parametrize("n,m,T,B", [(7, 1, 80, 256), (5, 3, 70, 256)])
def test_beyond_dense_kkt_properties(n, m, T, B):
    """nz 640 / 560, more than the dense kernels take: stationarity, primal feasibility, complementarity and signs of
    the returned (tau, lam, nu, slack) on the original data."""
    from diff_qp_mpc_amd import _lib
    nt = n + m
    C, c, F, f, x0, lo, hi = problem(n, m, T, B, seed=3, spread=0.05)
    lib = _lib.load()
    host = lib.dqp_mpc_qp_host_n_state(ctypes.byref(_lib.dqp_mpc_dims(B, n, m, T, 1, 0)))
    dims = _lib.dqp_mpc_dims(B, n, m, T, 1, 0, host)
    assert host > n and lib.dqp_mpc_qp_supported(ctypes.byref(dims)) == 1
    opts = _lib.dqp_opts(1e-12, 1e-10, 20, 3, _lib.DQP_FLAG_BATCH_TERMINATION, 0)
    t = [dev(a) for a in (C, c, F, f, x0, lo, hi)]
    kw = dict(dtype=torch.float64, device="cuda")
    tau = torch.empty(B, T, nt, **kw); lam = torch.empty(B, 2 * T * m, **kw); slack = torch.empty(B, 2 * T * m, **kw)
    nu = torch.empty(B, T * n, **kw); info = torch.empty(B, 2, dtype=torch.int32, device="cuda")
    ws = torch.empty(int(lib.dqp_mpc_qp_workspace_bytes(ctypes.byref(dims))) // 8, **kw)
    resid = torch.empty(B, **kw)
    tb = int(lib.dqp_mpc_qp_termination_bytes(ctypes.byref(dims), ctypes.byref(opts)))
    term = torch.empty(tb // 8 + 1, **kw)
    rc = lib.dqp_mpc_qp_forward(ctypes.byref(dims), ctypes.byref(opts), *[_p(x) for x in t], _p(tau), _p(lam), _p(nu),
                                _p(slack), _p(info), _p(resid), _p(ws), _p(term), None)
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


@pytest.mark.parametrize("name,n,m,T,host,tags", [("PADNL_n5_m3_T6_b3", 5, 3, 6, 6, ("single", "sqp")),
                                                  ("PADNL_n17_m3_T5_b3", 17, 3, 5, 29, ("single",))])
def test_mpc_caller_module_vs_reference(name, n, m, T, host, tags):
    """A caller's nonlinear torch module at (5, 3) and (17, 3): no stage-wise kernels of their own, so qp_wrapper.MPC
    runs the stepped solve on the host pair instead of raising NotImplementedError.  Against the reference's
    qp_wrapper.MPC on the same module: x, u within DT; dC, dc within GT for the single QP.  (The SQP gradients with a
    caller's module differ from the reference's at native pairs as well, e.g. (6, 3): DESIGN §4.10.p.)"""
    from diff_qp_mpc_amd import qp_wrapper, _lib
    g = dict(np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False))
    B = g["in_x0"].shape[0]
    dx = WideToy(n, m)
    for tag in tags:
        C, c = dev(g["in_C"], grad=True), dev(g["in_c"], grad=True)
        kw = dict(single_qp_solve=True) if tag == "single" else dict(qp_iter=3)
        mpc = qp_wrapper.MPC(n, m, T, u_lower=dev(g["in_u_lower"]), u_upper=dev(g["in_u_upper"]), n_batch=B, verbose=-1,
                             **kw)
        with _lib.trace(8192) as tr:
            x, u = mpc(dev(g["in_x0"]), qp_wrapper.QuadCost(C, c), dx, dx.jac)
            torch.cuda.synchronize()
        assert any("forward_kernel<dqp::ric::Cfg<%d, %d, false>, 2>" % (host, m) in k for k, _ in tr.records)
        np.testing.assert_allclose(x.detach().cpu().numpy(), g[tag + "_x"], err_msg=tag, **DT)
        np.testing.assert_allclose(u.detach().cpu().numpy(), g[tag + "_u"], err_msg=tag, **DT)
        if tag != "single":
            continue
        (x.sum() + 2.0 * u.sum()).backward()
        np.testing.assert_allclose(C.grad.cpu().numpy(), g[tag + "_dC"], err_msg=tag + " dC", **GT)
        np.testing.assert_allclose(c.grad.cpu().numpy(), g[tag + "_dc"], err_msg=tag + " dc", **GT)


def test_mpc_lindx_vs_reference_beyond_dense():
    """LinDx at (7, 1), T 80 (nz 640: the dense kernels stop at 512) on host 8 against the reference's
    qp_wrapper.MPC: x, u and the gradients wrt C, c, F, f, x0."""
    from diff_qp_mpc_amd.qp_wrapper import MPC, QuadCost, LinDx
    from diff_qp_mpc_amd import _lib
    g = dict(np.load(os.path.join(GOLDEN, "PAD_n7_m1_T80_b2.npz"), allow_pickle=False))
    B, n, m, T = g["in_x0"].shape[0], 7, 1, 80
    C, c, F, f, x0 = [dev(g["in_" + k], grad=True) for k in ("C", "c", "F", "f", "x0")]
    mpc = MPC(n, m, T, u_lower=dev(g["in_u_lower"]), u_upper=dev(g["in_u_upper"]), n_batch=B, verbose=-1,
              single_qp_solve=True)
    with _lib.trace(4096) as tr:
        x, u = mpc(x0, QuadCost(C, c), LinDx(F, f), None)
        torch.cuda.synchronize()
    assert any("forward_kernel<dqp::ric::Cfg<8, 1, false>, 0>" in k for k, _ in tr.records)
    np.testing.assert_allclose(x.detach().cpu().numpy(), g["single_x"], **ZT)
    np.testing.assert_allclose(u.detach().cpu().numpy(), g["single_u"], **ZT)
    (x.sum() + 2.0 * u.sum()).backward()
    for k, t in (("C", C), ("c", c), ("F", F), ("f", f), ("x0", x0)):
        got = t.grad.cpu().numpy() if t.grad is not None else np.zeros(t.shape)
        np.testing.assert_allclose(got, g["single_d%s" % k], err_msg="d%s" % k, **GT)


@pytest.mark.parametrize("n,m,T,B", [(5, 3, 6, 5), (17, 3, 5, 3), (11, 1, 8, 6)])
@pytest.mark.parametrize("batch_rule", [True, False])
def test_padded_stepped_matches_padded_fused(n, m, T, B, batch_rule):
    """dqp_mpc_qp_forward_stepped on the host, fed the linear residual of each compact iterate, = the padded fused
    forward; the backward from either gives the same gradients."""
    from diff_qp_mpc_amd import _lib
    lib = _lib.load()
    host = lib.dqp_mpc_qp_host_n_state(ctypes.byref(_lib.dqp_mpc_dims(B, n, m, T, 1, 0)))
    data = problem(n, m, T, B, seed=17 + n)
    w = _weights(B, T, n + m)
    a = capi_solve(n, m, T, data, host, batch_rule, w)
    b = capi_solve(n, m, T, data, host, batch_rule, w, stepped=True)
    assert int(np.abs(a["info"][:, 0]).max()) == 0 and int(np.abs(b["info"][:, 0]).max()) == 0
    np.testing.assert_allclose(b["tau"], a["tau"], **ZT)
    for k in ("lam", "nu", "slack"):
        np.testing.assert_allclose(b[k], a[k], err_msg=k, **DT)
    for k in ("dC", "dc", "dF", "df", "dx0"):
        np.testing.assert_allclose(b[k], a[k], err_msg=k, **GT)
    if batch_rule:
        assert int(b["info"][:, 1].min()) == int(a["info"][:, 1].min())


def test_stepped_callback_sees_the_compact_iterate():
    """_MPCQPStepped at (5, 3) (host 6): every iterate handed to the residual callback is (B, T (n + m))."""
    from diff_qp_mpc_amd import qp_wrapper
    n, m, T, B = 5, 3, 6, 4
    C, c, F, f, x0, lo, hi = [dev(a) for a in problem(n, m, T, B, seed=9)]
    seen = []

    def residual(z):
        seen.append(tuple(z.shape))
        tau = z.reshape(B, T, n + m)
        pred = torch.matmul(F.transpose(0, 1), tau[:, :-1, :, None])[..., 0] + f.transpose(0, 1)
        return torch.cat(((pred - tau[:, 1:, :n]).reshape(B, -1), tau[:, 0, :n] - x0), 1)

    assert qp_wrapper._MPCQPStepped.host_n_state(B, n, m, T) == 6
    tau = qp_wrapper._MPCQPStepped.apply(C, c, F, f, x0, lo, hi, n, m, T, residual)
    assert tuple(tau.shape) == (B, T, n + m)
    assert len(seen) == 20 and set(seen) == {(B, T * (n + m))}
    fused = qp_wrapper._MPCQP.apply(C, c, F, f, x0, lo, hi, n, m, T, None, 6)
    np.testing.assert_allclose(tau.cpu().numpy(), fused.cpu().numpy(), **ZT)


def test_dense_route_unchanged_for_lindx_7_1():
    """LinDx (7, 1) at T 10 (nz 80) keeps assemble + the dense kernels: no stage-wise and no pack kernel."""
    from diff_qp_mpc_amd.qp_wrapper import MPC, QuadCost, LinDx
    from diff_qp_mpc_amd import _lib
    n, m, T, B = 7, 1, 10, 4
    C, c, F, f, x0, lo, hi = [dev(a) for a in problem(n, m, T, B, seed=4)]
    mpc = MPC(n, m, T, u_lower=lo, u_upper=hi, n_batch=B, verbose=-1, single_qp_solve=True)
    with _lib.trace(4096) as tr:
        mpc(x0, QuadCost(C, c), LinDx(F, f), None)
        torch.cuda.synchronize()
    names = [k for k, _ in tr.records]
    assert not any("ric::" in k or "pad_copy" in k for k in names), names
    assert any("mpc_assemble" in k or "assemble" in k for k in names), names
    assert any("qp_forward_kernel" in k or "big" in k for k in names), names
