"""Per-sample, per-knot control bounds on the device paths of qp_wrapper.MPC (dqp_mpc_bounds):
dqp_mpc_assemble_bounds, dqp_mpc_qp_forward_bounds, dqp_mpc_qp_forward_stepped_bounds and the Python layers above them.

Checkers: (1) the assembly against numpy, element for element; (2) a vector bound written out in every layout against
the old entry point, bit for bit, on every route; (3) bounds that differ per (sample, knot, control) against the CPU
oracle's DenseQPFunction restatement on the numpy-assembled QP (h per row), every sample, on the null-space, stage-wise
(LDS-resident, streamed, wide, padded) and stepped routes; (4) the registered-model residual of the stage-wise kernels
against the dense route; (5) the reference's own qp_wrapper.MPC (tests/golden/make_golden_mpc_bounds.py) and a captured
SQP run; (6) the error paths.  Tolerances of test_gpu_ric.py: solution rtol 1e-6 / atol 1e-8, duals rtol 1e-5 /
atol 1e-7, gradients rtol 1e-4 / atol 1e-6.  Bounds: mid +- half, mid ~ U(-0.3, 0.3), half ~ U(0.05, 0.5) per element of
the layout under test.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import oracle

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "MPCB_n3_m1_T6_b6.npz")
ZT = dict(rtol=1e-6, atol=1e-8)
DT = dict(rtol=1e-5, atol=1e-7)
GT = dict(rtol=1e-4, atol=1e-6)
LAYOUTS = ("time_major", "batch_major", "per_knot", "per_sample")
GRADS = ("dC", "dc", "dF", "df", "dx0")


def dev(a, grad=False):
    t = torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")
    return t.requires_grad_() if grad else t


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def problem(n, m, T, B, seed, spread=0.15):
    """tests/test_gpu_ric.py::problem without its bounds: (C, c, F, f, x0), time-major."""
    rng = np.random.default_rng(seed)
    nt = n + m
    L = rng.standard_normal((T, B, nt, nt)) * 0.3
    C = L @ L.transpose(0, 1, 3, 2) + np.eye(nt)
    c = rng.standard_normal((T, B, nt))
    F = np.concatenate([np.eye(n) + spread * rng.standard_normal((T - 1, B, n, n)),
                        0.5 * rng.standard_normal((T - 1, B, n, m))], axis=-1)
    f = 0.1 * rng.standard_normal((T - 1, B, n))
    x0 = rng.standard_normal((B, n))
    return C, c, F, f, x0


def bounds(layout, m, T, B, seed, vector=None):
    """-> (lower buffer, upper buffer, (stride_b, stride_t), lower (T, B, m), upper (T, B, m)): mid +- half drawn per
    element of the layout (or the given (lower, upper) vectors written out in it), the buffers as the kernels index
    them and the same bounds broadcast to (T, B, m) for the numpy assembly."""
    shape = {"vector": (m,), "per_knot": (T, m), "per_sample": (B, m), "time_major": (T, B, m), "batch_major": (B, T, m)}[layout]
    strides = {"vector": (0, 0), "per_knot": (0, m), "per_sample": (m, 0), "time_major": (m, B * m),
               "batch_major": (T * m, m)}[layout]
    if vector is None:
        rng = np.random.default_rng(seed)
        mid, half = rng.uniform(-0.3, 0.3, shape), rng.uniform(0.05, 0.5, shape)
        lo, hi = mid - half, mid + half
    else:
        lo, hi = np.broadcast_to(vector[0], shape).copy(), np.broadcast_to(vector[1], shape).copy()
    full = {"vector": lambda a: np.broadcast_to(a, (T, B, m)), "per_knot": lambda a: np.broadcast_to(a[:, None], (T, B, m)),
            "per_sample": lambda a: np.broadcast_to(a[None], (T, B, m)), "time_major": lambda a: a,
            "batch_major": lambda a: a.transpose(1, 0, 2)}[layout]
    return lo, hi, strides, np.ascontiguousarray(full(lo)), np.ascontiguousarray(full(hi))


def assemble(C, c, F, f, x0, lo, hi):
    """The dense QP of qp_wrapper.py:638-679 in numpy (reference orderings), h per (b, t, k): lo, hi are (T, B, m)."""
    T, B, nt, _ = C.shape
    n = x0.shape[1]
    m = nt - n
    nz, neq, nineq = T * nt, T * n, 2 * T * m
    Q = np.zeros((B, nz, nz)); p = np.zeros((B, nz)); A = np.zeros((B, neq, nz)); b = np.zeros((B, neq))
    G = np.zeros((B, nineq, nz)); h = np.zeros((B, nineq))
    for t in range(T):
        Q[:, t * nt:(t + 1) * nt, t * nt:(t + 1) * nt] = C[t]
        p[:, t * nt:(t + 1) * nt] = c[t]
        for a in range(m):
            G[:, t * m + a, t * nt + n + a] = 1.0; h[:, t * m + a] = hi[t, :, a]
            G[:, T * m + t * m + a, t * nt + n + a] = -1.0; h[:, T * m + t * m + a] = -lo[t, :, a]
    for t in range(T - 1):
        A[:, t * n:(t + 1) * n, t * nt:(t + 1) * nt] = F[t]
        A[:, t * n:(t + 1) * n, (t + 1) * nt:(t + 1) * nt + n] = -np.eye(n)
        b[:, t * n:(t + 1) * n] = -f[t]
    A[:, (T - 1) * n:, :n] = np.eye(n); b[:, (T - 1) * n:] = x0
    return Q, p, G, h, A, b


def weights(B, T, nt):
    return np.linspace(0.5, 1.5, B * T * nt).reshape(B, T, nt)


_ORACLE = {}


def oracle_solve(key, data, lo_full, hi_full, w):
    """oracle.dense_forward / dense_backward on the numpy-assembled QP, computed once per problem and shared."""
    if key not in _ORACLE:
        C, c, F, f, x0 = data
        T, B, nt = c.shape
        n = x0.shape[1]
        Q, p, G, h, A, b = assemble(C, c, F, f, x0, lo_full, hi_full)
        o = oracle.dense_forward(Q, p, G, h, A, b)
        og = oracle.dense_backward(o["K"], o["zhat"], o["lam"], o["nu"], w.reshape(B, -1))
        res = dict(tau=o["zhat"].reshape(B, T, nt), lam=o["lam"], nu=o["nu"], slack=o["slack"])
        res["dC"] = np.stack([og["dQ"][:, t * nt:(t + 1) * nt, t * nt:(t + 1) * nt] for t in range(T)])
        res["dc"] = np.stack([og["dp"][:, t * nt:(t + 1) * nt] for t in range(T)])
        res["dF"] = np.stack([og["dA"][:, t * n:(t + 1) * n, t * nt:(t + 1) * nt] for t in range(T - 1)])
        res["df"] = np.stack([-og["db"][:, t * n:(t + 1) * n] for t in range(T - 1)])
        res["dx0"] = og["db"][:, (T - 1) * n:]
        for v in res.values():
            v.setflags(write=False)
        _ORACLE[key] = res
    return _ORACLE[key]


# route -> (extra forward flags, stepped, padded)
def _flags():
    from diff_qp_mpc_amd import _lib
    return {"nullspace": (0, False, False),
            "stage_lds": (_lib.DQP_FLAG_STAGEWISE, False, False),
            "stage_global": (_lib.DQP_FLAG_STAGEWISE | _lib.DQP_FLAG_RIC_GLOBAL_WS, False, False),
            "wide": (_lib.DQP_FLAG_STAGEWISE, False, False),
            "padded": (_lib.DQP_FLAG_STAGEWISE, False, True),
            "stepped": (_lib.DQP_FLAG_STAGEWISE, True, False),
            "stepped_padded": (_lib.DQP_FLAG_STAGEWISE, True, True)}


ROUTES = [("nullspace", 3, 1, 5, 5), ("nullspace", 3, 3, 5, 6), ("nullspace", 3, 1, 10, 6),
          ("stage_lds", 3, 1, 10, 6), ("stage_global", 3, 1, 10, 6), ("stage_lds", 12, 4, 6, 5), ("stage_global", 12, 4, 6, 5),
          ("stage_lds", 3, 1, 14, 8), ("wide", 13, 4, 6, 3), ("padded", 5, 3, 6, 3), ("stepped", 3, 1, 5, 5),
          ("stepped_padded", 5, 3, 6, 3)]


def capi_solve(route, n, m, T, data, lo, hi, strides, w, old_entry=False):
    """Forward (fused, or stepped with the linear residual computed in torch between the calls) and backward through the
    C ABI with the bounds buffers lo / hi at (stride_b, stride_t); old_entry: the entry point that takes the (u_lower,
    u_upper) vectors.  Returns outputs, gradients and the names of the kernels launched."""
    from diff_qp_mpc_amd import _lib
    lib = _lib.load()
    flags, stepped, padded = _flags()[route]
    C, c, F, f, x0 = [dev(a) for a in data]
    lo_d, hi_d = dev(lo), dev(hi)
    B, nt = x0.shape[0], n + m
    host = 0
    if padded:
        host = int(lib.dqp_mpc_qp_host_n_state(ctypes.byref(_lib.dqp_mpc_dims(B, n, m, T, 1, 0))))
        assert host > n
    dims = _lib.dqp_mpc_dims(B, n, m, T, 1, 0, host)
    opts = _lib.dqp_opts(1e-12, 1e-10, 20, 3, flags | _lib.DQP_FLAG_BATCH_TERMINATION, 0)
    kw = dict(dtype=torch.float64, device="cuda")
    o = dict(tau=torch.empty(B, T, nt, **kw), lam=torch.empty(B, 2 * T * m, **kw), nu=torch.empty(B, T * n, **kw),
             slack=torch.empty(B, 2 * T * m, **kw), info=torch.empty(B, 2, dtype=torch.int32, device="cuda"),
             resid=torch.empty(B, **kw))
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ins = [_p(t) for t in (C, c, F, f, x0)]
    bd = _lib.dqp_al_bounds(lo_d.data_ptr(), hi_d.data_ptr(), *strides)
    bnd = [_p(lo_d), _p(hi_d)] if old_entry else [ctypes.byref(bd)]
    outs = [_p(o[k]) for k in ("tau", "lam", "nu", "slack", "info", "resid")]
    if stepped:
        ws = torch.empty(int(lib.dqp_mpc_qp_stepped_workspace_bytes(ctypes.byref(dims))) // 8, **kw)
        tb = int(lib.dqp_mpc_qp_stepped_termination_bytes(ctypes.byref(dims), ctypes.byref(opts)))
    else:
        ws = torch.empty(int(lib.dqp_mpc_qp_workspace_bytes(ctypes.byref(dims))) // 8, **kw)
        tb = int(lib.dqp_mpc_qp_termination_bytes(ctypes.byref(dims), ctypes.byref(opts)))
    assert ws.numel() > 0 and tb > 0
    term = torch.empty(tb // 8 + 1, **kw)
    with _lib.trace(512) as tr:
        if not stepped:
            fwd = lib.dqp_mpc_qp_forward if old_entry else lib.dqp_mpc_qp_forward_bounds
            assert fwd(ctypes.byref(dims), ctypes.byref(opts), *ins, *bnd, *outs, _p(ws), _p(term), st) == 0
        else:
            fwd = lib.dqp_mpc_qp_forward_stepped if old_entry else lib.dqp_mpc_qp_forward_stepped_bounds
            call = lambda ry, a, b: fwd(ctypes.byref(dims), ctypes.byref(opts), *ins, *bnd, _p(ry), a, b, *outs, _p(ws), _p(term), st)
            assert call(None, 0, 0) == 0
            for it in range(20):
                tau = o["tau"]
                pred = torch.matmul(F.transpose(0, 1), tau[:, :-1, :, None])[..., 0] + f.transpose(0, 1)
                ry = torch.cat(((pred - tau[:, 1:, :n]).reshape(B, -1), tau[:, 0, :n] - x0), 1).contiguous()
                assert call(ry, it, it + 1) == 0
        g = [torch.full(a.shape, float("nan"), **kw) for a in (C, c, F, f, x0)]
        bflags = _lib.DQP_FLAG_DENSE_BACKWARD | (flags & _lib.DQP_FLAG_STAGEWISE)
        bo = _lib.dqp_opts(0.0, 0.0, 0, 0, bflags, 0)
        rc = lib.dqp_mpc_qp_backward(ctypes.byref(dims), ctypes.byref(bo), _p(C), _p(F), _p(o["tau"]), _p(o["lam"]),
                                     _p(o["nu"]), _p(o["slack"]), _p(dev(w)), *[_p(t) for t in g], _p(None), _p(ws), st)
        assert rc == 0
        torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in o.items()}
    res.update({k: t.cpu().numpy() for k, t in zip(GRADS, g)})
    res["kernels"] = [k for k, _ in tr.records]
    return res


def _strided_kernels(names):
    return [k for k in names if "forward_kernel" in k and "StridedBounds" in k]


# ------------------------------------------------------------------ 1. assembly
@pytest.mark.parametrize("layout", LAYOUTS)
def test_assembly_builds_h_from_the_layout(layout):
    from diff_qp_mpc_amd import _lib
    lib = _lib.load()
    n, m, T, B = 3, 2, 4, 5
    data = problem(n, m, T, B, seed=41)
    lo, hi, strides, lo_f, hi_f = bounds(layout, m, T, B, seed=42)
    want = assemble(*data, lo_f, hi_f)
    nt = n + m
    nz, neq, nineq = T * nt, T * n, 2 * T * m
    kw = dict(dtype=torch.float64, device="cuda")
    dims = _lib.dqp_mpc_dims(B, n, m, T, 1, 0)
    ins = [dev(a) for a in data]
    got = {}
    for tag in ("twin", "vector"):
        outs = [torch.full(s, float("nan"), **kw) for s in ((B, nz, nz), (B, nz), (B, nineq, nz), (B, nineq), (B, neq, nz), (B, neq))]
        if tag == "twin":
            lo_d, hi_d = dev(lo), dev(hi)
            bd = _lib.dqp_al_bounds(lo_d.data_ptr(), hi_d.data_ptr(), *strides)
            rc = lib.dqp_mpc_assemble_bounds(ctypes.byref(dims), *[_p(t) for t in ins], ctypes.byref(bd), *[_p(t) for t in outs], None)
        else:
            lo_d, hi_d = dev(lo_f[0, 0]), dev(hi_f[0, 0])
            rc = lib.dqp_mpc_assemble(ctypes.byref(dims), *[_p(t) for t in ins], _p(lo_d), _p(hi_d), *[_p(t) for t in outs], None)
        assert rc == 0
        torch.cuda.synchronize()
        got[tag] = [t.cpu().numpy() for t in outs]
    np.testing.assert_array_equal(got["twin"][3], want[3])                # h, element for element
    assert not np.array_equal(got["twin"][3], got["vector"][3])
    for i, k in ((0, "Q"), (1, "p"), (2, "G"), (4, "A"), (5, "b")):
        np.testing.assert_array_equal(got["twin"][i], got["vector"][i], err_msg=k)
        np.testing.assert_array_equal(got["twin"][i], want[i], err_msg=k)


# ------------------------------------------------------------------ 2. same arithmetic
@pytest.mark.parametrize("route,n,m,T,B", ROUTES)
def test_vector_bound_in_every_layout_equals_the_old_entry_point(route, n, m, T, B):
    """A vector bound written out as (T, m), (B, m), (T, B, m) and (B, T, m): the same numbers reach the same
    arithmetic, so tau, lam, nu, slack and the five gradients equal the old entry point's bit for bit -- on the
    stage-wise routes from the strided instantiations, which the kernel names show."""
    data = problem(n, m, T, B, seed=7 * n + T + B)
    w = weights(B, T, n + m)
    vec = (-0.4 * np.ones(m) - 0.05 * np.arange(m), 0.4 * np.ones(m) + 0.03 * np.arange(m))
    old = capi_solve(route, n, m, T, data, vec[0], vec[1], (0, 0), w, old_entry=True)
    assert not _strided_kernels(old["kernels"])
    twin = capi_solve(route, n, m, T, data, vec[0], vec[1], (0, 0), w)
    assert twin["kernels"] == old["kernels"]                    # the twin at (0, 0) launches the old entry point's kernels
    for layout in LAYOUTS:
        lo, hi, strides, _, _ = bounds(layout, m, T, B, seed=0, vector=vec)
        got = capi_solve(route, n, m, T, data, lo, hi, strides, w)
        assert bool(_strided_kernels(got["kernels"])) == (route != "nullspace"), (layout, got["kernels"])
        for k in ("tau", "lam", "nu", "slack", "info") + GRADS:
            np.testing.assert_array_equal(got[k], old[k], err_msg="%s %s" % (layout, k))


# ------------------------------------------------------------------ 3. varying bounds against the oracle
VARYING = [(r, n, m, T, B, "time_major") for r, n, m, T, B in ROUTES] + \
          [("stage_lds", 3, 1, 10, 6, layout) for layout in ("per_knot", "per_sample", "batch_major")]


def _check(got, want, B):
    np.testing.assert_array_equal(got["info"][:, 0], np.zeros(B, dtype=np.int32))
    np.testing.assert_allclose(got["tau"], want["tau"], err_msg="tau", **ZT)
    for k in ("lam", "nu", "slack"):
        np.testing.assert_allclose(got[k], want[k], err_msg=k, **DT)
    for k in GRADS:
        np.testing.assert_allclose(got[k], want[k], err_msg=k, **GT)


@pytest.mark.parametrize("route,n,m,T,B,layout", VARYING)
def test_varying_bounds_vs_cpu_oracle(route, n, m, T, B, layout):
    """Bounds that differ for every element of the layout, every sample compared (no convergence mask): solution, duals
    and the five gradients against oracle.dense_forward / dense_backward on the QP whose h numpy wrote per (b, t, k)."""
    seed = 100 * n + 10 * m + T + B
    data = problem(n, m, T, B, seed=seed)
    lo, hi, strides, lo_f, hi_f = bounds(layout, m, T, B, seed=seed + 1)
    w = weights(B, T, n + m)
    want = oracle_solve((n, m, T, B, layout), data, lo_f, hi_f, w)
    gap = np.minimum(hi_f - want["tau"][..., n:].transpose(1, 0, 2), want["tau"][..., n:].transpose(1, 0, 2) - lo_f)
    assert gap.min() <= 1e-6 and gap.max() >= 0.02                # some rows active, some not
    got = capi_solve(route, n, m, T, data, lo, hi, strides, w)
    assert bool(_strided_kernels(got["kernels"])) == (route != "nullspace"), got["kernels"]
    if route in ("stage_lds", "stage_global") and (n, m, T) == (3, 1, 10):
        lds_resident = any("Cfg<3, 1, true>" in k for k in _strided_kernels(got["kernels"]))
        assert lds_resident == (route == "stage_lds"), got["kernels"]
    _check(got, want, B)


def test_varying_bounds_per_problem_termination_through_the_python_layer():
    """_MPCQP with (T, B, m) bounds under qp.TERMINATION = "per_problem" at (3, 1), T 14 -- no null-space kernel has this
    QP size, so forward and backward both take the stage-wise kernels: the solution and the gradients against the same
    oracle run."""
    from diff_qp_mpc_amd import _lib, qp as qpmod, qp_wrapper
    n, m, T, B = 3, 1, 14, 8
    seed = 100 * n + 10 * m + T + B
    data = problem(n, m, T, B, seed=seed)
    lo, hi, _, lo_f, hi_f = bounds("time_major", m, T, B, seed=seed + 1)
    w = weights(B, T, n + m)
    want = oracle_solve((n, m, T, B, "time_major"), data, lo_f, hi_f, w)
    ins = [dev(a, grad=True) for a in data]
    old = qpmod.TERMINATION
    qpmod.TERMINATION = "per_problem"
    try:
        with _lib.trace(64) as tr:
            tau = qp_wrapper._MPCQP.apply(*ins, dev(lo), dev(hi), n, m, T)
            torch.cuda.synchronize()
    finally:
        qpmod.TERMINATION = old
    assert _strided_kernels([k for k, _ in tr.records])
    (tau * dev(w)).sum().backward()
    np.testing.assert_allclose(tau.detach().cpu().numpy(), want["tau"], **ZT)
    for t, k in zip(ins, GRADS):
        np.testing.assert_allclose(t.grad.cpu().numpy(), want[k], err_msg=k, **GT)


# ------------------------------------------------------------------ 4. registered-model residual
def test_true_dynamics_residual_with_varying_bounds_stagewise_equals_dense():
    """pendulum_dx, T 10, B 6, (T, B, m) bounds: the stage-wise kernels with the model's own step as equality residual
    against the dense route with the DynamicsResidual closure (test_gpu_ric.py::
    test_true_dynamics_residual_stagewise_equals_dense, its rtol 1e-5 / atol 1e-7)."""
    from diff_qp_mpc_amd import _lib, qp_wrapper
    from diff_qp_mpc_amd.dynamics import DeviceDynamics
    dyn = DeviceDynamics("pendulum_dx")
    n, m, T, B = dyn.n_state, dyn.n_ctrl, 10, 6
    gen = torch.Generator().manual_seed(T)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64).cuda()
    x0 = 0.3 * rnd(B, n)
    x0[:, :2] = torch.nn.functional.normalize(x0[:, :2] + torch.tensor([1.0, 0.0]).cuda(), dim=1)
    L = 0.3 * rnd(T, B, n + m, n + m)
    lo, hi, _, _, _ = bounds("time_major", m, T, B, seed=5)
    outs, names = {}, {}
    for fused in (True, False):
        qp_wrapper.FUSED_MPC_QP = fused
        try:
            C = (L @ L.transpose(2, 3) + torch.eye(n + m, dtype=torch.float64, device="cuda")).requires_grad_()
            c = (0.2 * torch.ones(T, B, n + m, dtype=torch.float64, device="cuda")).requires_grad_()
            mpc = qp_wrapper.MPC(n, m, T, u_lower=dev(lo), u_upper=dev(hi), n_batch=B, verbose=-1, single_qp_solve=True)
            with _lib.trace(256) as tr:
                x, u = mpc(x0, qp_wrapper.QuadCost(C, c), dyn, dyn.jac)
                torch.cuda.synchronize()
            (x.sum() + 2.0 * u.sum()).backward()
            outs[fused] = [t.detach().cpu().numpy() for t in (x, u, C.grad, c.grad)]
            names[fused] = [k for k, _ in tr.records]
        finally:
            qp_wrapper.FUSED_MPC_QP = True
    assert _strided_kernels(names[True]) and not _strided_kernels(names[False])
    assert any("assemble_bounds_kernel" in k for k in names[False])
    for a, b, k in zip(outs[True], outs[False], ("x", "u", "dC", "dc")):
        np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-7, err_msg=k)


# ------------------------------------------------------------------ 5. the reference's golden, and a captured SQP run
def test_mpc_mirror_vs_reference_with_time_major_bounds():
    from diff_qp_mpc_amd.qp_wrapper import MPC, QuadCost, LinDx
    g = dict(np.load(GOLDEN, allow_pickle=False))
    T, B, m = g["in_u_lower"].shape
    n = g["in_x0"].shape[1]
    C, c, F, f, x0 = [dev(g["in_" + k], grad=True) for k in ("C", "c", "F", "f", "x0")]
    mpc = MPC(n, m, T, u_lower=dev(g["in_u_lower"]), u_upper=dev(g["in_u_upper"]), n_batch=B, verbose=-1, single_qp_solve=True)
    x, u = mpc(x0, QuadCost(C, c), LinDx(F, f), None)
    np.testing.assert_allclose(x.detach().cpu().numpy(), g["single_x"], **ZT)
    np.testing.assert_allclose(u.detach().cpu().numpy(), g["single_u"], **ZT)
    (x.sum() + 2.0 * u.sum()).backward()
    for k, t in (("C", C), ("c", c), ("F", F), ("f", f), ("x0", x0)):
        np.testing.assert_allclose(t.grad.cpu().numpy(), g["single_d" + k], err_msg="d" + k, **GT)


def test_graphed_sqp_with_per_sample_bounds_replays_bitwise():
    """qp_iter = 3 with (1, B, m) bounds: GraphedMPC's replay (forward and backward) equals the eager call bit for bit; the
    bounds are read from the caller's tensor, which the capture keeps by pointer."""
    from diff_qp_mpc_amd.qp_wrapper import MPC, GraphedMPC, QuadCost, LinDx
    g = dict(np.load(GOLDEN, allow_pickle=False))
    T, B, m = g["in_u_lower"].shape
    n = g["in_x0"].shape[1]
    lo, hi = dev(g["in_u_lower"][:1]), dev(g["in_u_upper"][:1])            # (1, B, m)
    make = lambda: [dev(g["in_" + k], grad=True) for k in ("x0", "C", "c", "F", "f")]

    def eager():
        x0, C, c, F, f = ins = make()
        mpc = MPC(n, m, T, u_lower=lo, u_upper=hi, n_batch=B, verbose=-1, qp_iter=3)
        mpc.capturable = True
        x, u = mpc(x0, QuadCost(C, c), LinDx(F, f), None)
        return [x, u] + list(torch.autograd.grad(x.sum() + 2.0 * u.sum(), ins, allow_unused=True))
    want = eager()
    ins = make()
    gm = GraphedMPC(MPC(n, m, T, u_lower=lo, u_upper=hi, n_batch=B, verbose=-1, qp_iter=3), ins)
    x, u = gm(*ins)
    got = [x, u] + list(torch.autograd.grad(x.sum() + 2.0 * u.sum(), ins, allow_unused=True))
    assert float((u.detach() - lo).abs().min()) < 1e-6 or float((hi - u.detach()).abs().min()) < 1e-6     # a bound is active
    for a, b in zip(got, want):
        assert (a is None) == (b is None)
        if a is not None:
            assert torch.equal(a, b)


# ------------------------------------------------------------------ 6. error paths
def test_rejected_shapes_raise():
    from diff_qp_mpc_amd import sl1qp_mpc
    from diff_qp_mpc_amd.qp_wrapper import MPC, QuadCost, LinDx
    n, m, T, B = 3, 1, 6, 5
    C, c, F, f, x0 = [dev(a) for a in problem(n, m, T, B, seed=1)]
    for shape in ((B, m), (B, T, m), (T, B, m + 1)):
        lo = -torch.ones(*shape, dtype=torch.float64, device="cuda")
        mpc = MPC(n, m, T, u_lower=lo, u_upper=-lo, n_batch=B, verbose=-1, single_qp_solve=True)
        with pytest.raises(ValueError, match="control bounds of shape"):
            mpc(x0, QuadCost(C, c), LinDx(F, f), None)
    mpc = MPC(n, m, T, u_lower=-torch.ones(T, m, dtype=torch.float64, device="cuda"),
              u_upper=torch.ones(T, B, m, dtype=torch.float64, device="cuda"), n_batch=B, verbose=-1, single_qp_solve=True)
    with pytest.raises(ValueError, match="differ in shape"):
        mpc(x0, QuadCost(C, c), LinDx(F, f), None)
    with pytest.raises(ValueError, match=r"bounds of shape \(n_ctrl,\) only"):
        sl1qp_mpc.MPC(n, m, T, u_lower=-torch.ones(T, m, dtype=torch.float64, device="cuda"),
                      u_upper=torch.ones(T, m, dtype=torch.float64, device="cuda"), n_batch=B)
