#!/usr/bin/env python3
"""Timing of the stage-wise MPC QP kernels (csrc/dqp_ric_kernels.h) at the BASELINE config-4 shape:
n_state 12, n_ctrl 4, T 30 (nz 480, nineq 240, neq 360), B = 8192 (BATCH), HIP events around the
C-ABI calls dqp_mpc_qp_forward / dqp_mpc_qp_backward, both termination modes.
HOST=n': the problem padded onto the kernels of (n', m) (dqp_mpc_dims.n_state_host), with the per-kernel split of one
forward and backward (pack / solve / unpack).  DENSE=1: also assemble + DenseQPFunction on the same data (forward and
backward, per-problem termination), the route the dense kernels give where nz <= 512.
--bounds: only the comparison of the per-sample, per-knot bound layout with the vector one -- the same limits as an
(n_ctrl,) vector and as a (T, B, n_ctrl) tensor through qp_wrapper._MPCQP forward + backward (what qp_wrapper.MPC runs per
QP), 30 calls each, alternating; median and quartiles.  DYN=name: with that registered model's residual (config 2:
N=3 M=1 T=10 BATCH=1024 DYN=pendulum_dx)."""
import ctypes, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from diff_qp_mpc_amd import _lib
lib = _lib.load()
n, m, T = int(os.environ.get("N", 12)), int(os.environ.get("M", 4)), int(os.environ.get("T", 30))
B = int(os.environ.get("BATCH", 8192))
nt = n + m
gen = torch.Generator(device="cuda").manual_seed(0)
rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64, device="cuda")
L = 0.3 * rnd(T, B, nt, nt)
C = L @ L.transpose(2, 3) + torch.eye(nt, dtype=torch.float64, device="cuda")
del L
c = rnd(T, B, nt)
F = torch.cat([torch.eye(n, dtype=torch.float64, device="cuda") + 0.05 * rnd(T - 1, B, n, n), 0.5 * rnd(T - 1, B, n, m)], -1).contiguous()
f = 0.1 * rnd(T - 1, B, n)
x0 = rnd(B, n)
lo, hi = torch.full((m,), -0.4, dtype=torch.float64, device="cuda"), torch.full((m,), 0.4, dtype=torch.float64, device="cuda")
host = int(os.environ.get("HOST", 0))
dims = _lib.dqp_mpc_dims(B, n, m, T, 1, 0, host)
assert lib.dqp_mpc_qp_supported(ctypes.byref(dims)) == 1
kw = dict(dtype=torch.float64, device="cuda")
tau = torch.empty(B, T, nt, **kw); lam = torch.empty(B, 2 * T * m, **kw); slack = torch.empty(B, 2 * T * m, **kw)
nu = torch.empty(B, T * n, **kw); info = torch.empty(B, 2, dtype=torch.int32, device="cuda"); resid = torch.empty(B, **kw)
wsb = int(lib.dqp_mpc_qp_workspace_bytes(ctypes.byref(dims)))
ws = torch.empty(wsb // 8, **kw)
P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
g = torch.ones(B, T, nt, **kw)
dC, dc, dF, df, dx0 = torch.empty_like(C), torch.empty_like(c), torch.empty_like(F), torch.empty_like(f), torch.empty_like(x0)
if "--bounds" in sys.argv[1:]:
    from diff_qp_mpc_amd import qp_wrapper
    from diff_qp_mpc_amd.dynamics import DeviceDynamics
    dyn = DeviceDynamics(os.environ["DYN"]) if os.environ.get("DYN") else None
    ins = [t.detach().clone().requires_grad_() for t in (C, c, F, f, x0)]
    pairs = {"vector": (lo, hi), "(T, B, m)": (lo.expand(T, B, m).contiguous(), hi.expand(T, B, m).contiguous())}
    def call(k):
        z = qp_wrapper._MPCQP.apply(*ins, *pairs[k], n, m, T, dyn)
        z.backward(g)
    ms = {k: [] for k in pairs}
    for k in pairs:
        call(k); call(k)
    torch.cuda.synchronize()
    for _ in range(30):
        for k in pairs:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); call(k); b.record()
            torch.cuda.synchronize()
            ms[k].append(a.elapsed_time(b))
    print("B=%d n=%d m=%d T=%d dyn=%s: _MPCQP forward + backward, 30 calls each, alternating" % (B, n, m, T, os.environ.get("DYN")))
    for k, v in ms.items():
        q1, q2, q3 = np.percentile(v, [25, 50, 75])
        print("  bounds %-10s median %.3f ms   quartiles %.3f .. %.3f" % (k, q2, q1, q3))
    sys.exit(0)
print("B=%d n=%d m=%d T=%d  nz=%d  workspace %.0f MB  inputs %.0f MB" % (B, n, m, T, T * nt, wsb / 1e6, (C.numel() + F.numel()) * 8 / 1e6))


def timed(fn, reps=5):
    fn(); fn(); torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    ts = sorted(a.elapsed_time(b) for a, b in ev)
    return ts[len(ts) // 2]


for mode, flag in (("batch", _lib.DQP_FLAG_BATCH_TERMINATION), ("per_problem", 0)):
    opts = _lib.dqp_opts(1e-12, 1e-10, 20, 3, flag, 0)
    tb = int(lib.dqp_mpc_qp_termination_bytes(ctypes.byref(dims), ctypes.byref(opts)))
    term = torch.empty(max(tb // 8, 1), **kw)
    def fwd():
        rc = lib.dqp_mpc_qp_forward(ctypes.byref(dims), ctypes.byref(opts), P(C), P(c), P(F), P(f), P(x0), P(lo), P(hi),
                                    P(tau), P(lam), P(nu), P(slack), P(info), P(resid), P(ws), P(term) if tb else None, None)
        assert rc == 0, rc
    tf = timed(fwd)
    it = info[:, 1].float()
    print("termination %-12s forward %.2f ms (%.0f k QP/s)   iterations mean %.1f max %d   best residual max %.1e   status!=0: %d"
          % (mode, tf, B / tf, float(it.mean()), int(it.max()), float(resid.max()), int((info[:, 0] != 0).sum())))
bo = _lib.dqp_opts(0.0, 0.0, 0, 0, _lib.DQP_FLAG_DENSE_BACKWARD, 0)
def bwd():
    rc = lib.dqp_mpc_qp_backward(ctypes.byref(dims), ctypes.byref(bo), P(C), P(F), P(tau), P(lam), P(nu), P(slack), P(g),
                                 P(dC), P(dc), P(dF), P(df), P(dx0), None, P(ws), None)
    assert rc == 0, rc
tb_ = timed(bwd)
print("backward %.2f ms" % tb_)

if host:
    opts = _lib.dqp_opts(1e-12, 1e-10, 20, 3, 0, 0)
    with _lib.trace(64) as tr:
        assert lib.dqp_mpc_qp_forward(ctypes.byref(dims), ctypes.byref(opts), P(C), P(c), P(F), P(f), P(x0), P(lo), P(hi),
                                      P(tau), P(lam), P(nu), P(slack), P(info), P(resid), P(ws), None, None) == 0
        bwd()
        torch.cuda.synchronize()
    for k, (cnt, ms) in tr.by_kernel().items():
        print("  %-90s x%d  %.3f ms" % (k[:90], cnt, ms))
if os.environ.get("DENSE"):
    from diff_qp_mpc_amd import qp as qpmod, qp_wrapper
    qpmod.TERMINATION = "per_problem"
    ins = [t.detach().clone().requires_grad_() for t in (C, c, F, f, x0)]
    def dense():
        Q, p, G, h, A, b = qp_wrapper._AssembleDenseQP.apply(*ins, lo, hi, n, m, T)
        z = qpmod.DenseQPFunction(verbose=-1)(Q, p, G, h, A, b)
        z.sum().backward()
    def padded():
        z = qp_wrapper._MPCQP.apply(*ins, lo, hi, n, m, T, None, host)
        z.sum().backward()
    print("per problem, forward + backward through autograd: assemble + dense %.2f ms, padded stage-wise (host %d) %.2f ms"
          % (timed(dense), host, timed(padded)))
