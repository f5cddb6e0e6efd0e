"""Per-sample, per-knot control bounds of the MPC QP (dqp_mpc_bounds) without a GPU: the header, the binding and the
library have the `_bounds` twins of dqp_mpc_assemble / dqp_mpc_qp_forward / dqp_mpc_qp_forward_stepped, the time-major
layout helper maps each accepted shape to its strides without expanding it, every twin refuses a bad layout and returns
at nbatch == 0 with each accepted one, the old entry points answer null probes as before, and the CPU oracle -- the
reference of test_gpu_mpc_bounds.py -- reproduces the reference's own qp_wrapper.MPC on (T, B, m) bounds
(tests/golden/make_golden_mpc_bounds.py).  Tolerances of test_gpu_ric.py."""
import ctypes
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "MPCB_n3_m1_T6_b6.npz")
ZT = dict(rtol=1e-6, atol=1e-8)
DT = dict(rtol=1e-5, atol=1e-7)
GT = dict(rtol=1e-4, atol=1e-6)
TWINS = ("dqp_mpc_assemble", "dqp_mpc_qp_forward", "dqp_mpc_qp_forward_stepped")
DQP_OK, DQP_ERR_BAD_ARG = 0, -1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from diff_qp_mpc_amd import _lib
    return _lib.load()


def test_header_library_and_binding(lib):
    from diff_qp_mpc_amd import _lib
    header = open(os.path.join(ROOT, "include", "dqp.h")).read()
    assert "typedef dqp_al_bounds dqp_mpc_bounds;" in header
    for s in TWINS:
        assert s + "_bounds(" in header, s
        assert s + "(" in header                    # the old entry point stays declared
        assert s + "_bounds" in _lib.SYMBOLS and s in _lib.SYMBOLS
        assert hasattr(lib, s + "_bounds") and hasattr(lib, s)
    assert "dqp_mpc_qp_backward_bounds" not in header          # the backward reads no bounds
    assert lib.dqp_version() == 303
    assert header.count("#define DQP_VERSION 303") == 1
    assert ctypes.sizeof(_lib.dqp_al_bounds(None, None, 0, 0)) == 32


# ------------------------------------------------------------------ the Python layout helper (time-major)
def _cases(B, T, m):
    base = torch.arange(1.0, T * B * m + 1, dtype=torch.float64).reshape(T, B, m)
    return {"vector": (base[0, 0].clone(), (0, 0), m),
            "per_knot": (base[:, 0].clone(), (0, m), T * m),
            "per_knot_3d": (base[:, :1].clone(), (0, m), T * m),
            "per_sample": (base[:1].clone(), (m, 0), B * m),
            "full": (base.clone(), (m, B * m), T * B * m)}


def test_layout_helper_strides_and_buffers():
    from diff_qp_mpc_amd import al_utils
    B, T, m = 6, 5, 2
    for name, (lo, strides, numel) in _cases(B, T, m).items():
        bd = al_utils.mpc_bounds_layout(lo, lo + 1.0, B, T, m)
        assert (bd.stride_b, bd.stride_t) == strides, name
        assert (bd.c.stride_b, bd.c.stride_t) == strides, name
        assert bd.lower.numel() == numel and bd.upper.numel() == numel, name       # nothing expanded
        assert bd.lower.dtype == torch.float64 and bd.lower.is_contiguous() and bd.upper.is_contiguous()
        assert bd.c.lower == bd.lower.data_ptr() and bd.c.upper == bd.upper.data_ptr()
        assert bd.lower.data_ptr() == lo.data_ptr()            # fp64 contiguous input: passed through, no copy
        # the index formula of include/dqp.h reproduces the broadcast torch does on the time-major tensor
        want = (lo[:, None] if name == "per_knot" else lo).expand(T, B, m)
        flat = bd.lower.reshape(-1)
        for b_, t_, k_ in ((0, 0, 0), (B - 1, T - 1, m - 1), (2, 3, 1), (4, 1, 0)):
            assert flat[b_ * bd.stride_b + t_ * bd.stride_t + k_] == want[t_, b_, k_], name
    full = _cases(B, T, m)["full"][0]
    bd = al_utils.mpc_bounds_layout(full.float(), full.float() + 1, B, T, m)      # converted, still not expanded
    assert bd.lower.dtype == torch.float64 and bd.lower.numel() == T * B * m
    view = full.transpose(0, 1).contiguous().transpose(0, 1)                      # (T, B, m) with batch-major strides
    bd = al_utils.mpc_bounds_layout(view, view + 1, B, T, m)
    assert bd.lower.is_contiguous() and (bd.stride_b, bd.stride_t) == (m, B * m)
    lo_g = full.clone().requires_grad_()
    assert not al_utils.mpc_bounds_layout(lo_g, lo_g.detach() + 1, B, T, m).lower.requires_grad


def test_layout_helper_rejects():
    from diff_qp_mpc_amd import al_utils
    B, T, m = 6, 5, 2
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    bad = [(z(T, B, m), z(T, m)),                 # lower / upper of different shapes
           (z(m), z(1, B, m)),
           (z(B, m), z(B, m)),                    # per sample without its knot axis: ambiguous with (T, m)
           (z(B, T, m), z(B, T, m)),              # batch-major
           (z(B, 1, m), z(B, 1, m)),
           (z(T, B, m + 1), z(T, B, m + 1)),      # wrong trailing size
           (z(T, m + 1), z(T, m + 1)),
           (z(m + 1), z(m + 1)),
           (z(T + 1, B, m), z(T + 1, B, m)),
           (z(1, 1, m), z(1, 1, m))]
    for lo, hi in bad:
        with pytest.raises(ValueError):
            al_utils.mpc_bounds_layout(lo, hi, B, T, m)
    with pytest.raises(ValueError):
        al_utils.mpc_bounds_layout(None, None, B, T, m)


def test_square_batch_reads_a_matrix_as_per_knot():
    """(T, m) is per knot whatever the batch: at T == B the (B, m) array a caller may mean is not told apart, which is why
    per-sample bounds carry their knot axis, (1, B, m)."""
    from diff_qp_mpc_amd import al_utils
    z = torch.zeros(4, 2, dtype=torch.float64)
    bd = al_utils.mpc_bounds_layout(z, z + 1, 4, 4, 2)
    assert (bd.stride_b, bd.stride_t) == (0, 2)


def test_sl1qp_keeps_vector_bounds():
    from diff_qp_mpc_amd import sl1qp_mpc
    T, m = 5, 2
    with pytest.raises(ValueError, match=r"bounds of shape \(n_ctrl,\) only"):
        sl1qp_mpc.MPC(3, m, T, u_lower=-torch.ones(T, m), u_upper=torch.ones(T, m))
    sl1qp_mpc.MPC(3, m, T, u_lower=-torch.ones(m), u_upper=torch.ones(m))
    sl1qp_mpc.MPC(3, m, T, u_lower=-1.0, u_upper=1.0)


# ------------------------------------------------------------------ the twins' argument checks (no launch is reached)
N, M, T, B = 3, 2, 4, 5
ALLOWED = {"vector": (0, 0), "per_knot": (0, M), "per_sample": (M, 0), "time_major": (M, B * M), "batch_major": (T * M, M)}
BAD = [(M + 1, 0), (0, M + 1), (M, M), (-M, 0), (T * M, B * M)]


def _call(lib, name, dims, bounds):
    from diff_qp_mpc_amd import _lib
    z = ctypes.c_void_p(0)
    opts = _lib.dqp_opts(1e-12, 1e-10, 20, 3, 0, 0)
    if name == "dqp_mpc_assemble":
        return lib.dqp_mpc_assemble_bounds(ctypes.byref(dims), z, z, z, z, z, bounds, z, z, z, z, z, z, z)
    if name == "dqp_mpc_qp_forward":
        return lib.dqp_mpc_qp_forward_bounds(ctypes.byref(dims), ctypes.byref(opts), z, z, z, z, z, bounds, *([z] * 9))
    return lib.dqp_mpc_qp_forward_stepped_bounds(ctypes.byref(dims), ctypes.byref(opts), z, z, z, z, z, bounds, z, 0, 0, *([z] * 9))


@pytest.mark.parametrize("name", TWINS)
def test_twins_refuse_bad_layouts(name, lib):
    from diff_qp_mpc_amd import _lib
    for nb in (B, 0):                       # struct and strides are checked in front of the nbatch == 0 return
        dims = _lib.dqp_mpc_dims(nb, N, M, T, 1, 0)
        for sb, st in BAD:
            bd = _lib.dqp_al_bounds(None, None, sb, st)
            assert _call(lib, name, dims, ctypes.byref(bd)) == DQP_ERR_BAD_ARG, (nb, sb, st)
        assert _call(lib, name, dims, None) == DQP_ERR_BAD_ARG          # null struct
    dims = _lib.dqp_mpc_dims(B, N, M, T, 1, 0)
    for sb, st in ALLOWED.values():         # null lower / upper at nbatch > 0
        bd = _lib.dqp_al_bounds(None, None, sb, st)
        assert _call(lib, name, dims, ctypes.byref(bd)) == DQP_ERR_BAD_ARG


@pytest.mark.parametrize("name", TWINS)
def test_twins_return_ok_on_an_empty_batch(name, lib):
    from diff_qp_mpc_amd import _lib
    dims = _lib.dqp_mpc_dims(0, N, M, T, 1, 0)
    for key, (sb, st) in ALLOWED.items():
        if key == "time_major":
            st = 0 * M                      # (m, B m) at B == 0: the per-sample pair
        bd = _lib.dqp_al_bounds(None, None, sb, st)
        assert _call(lib, name, dims, ctypes.byref(bd)) == DQP_OK, key


def test_old_entry_points_keep_their_null_probe_codes(lib):
    from diff_qp_mpc_amd import _lib
    z = ctypes.c_void_p(0)
    opts = _lib.dqp_opts(1e-12, 1e-10, 20, 3, 0, 0)
    for nb, want in ((0, DQP_OK), (B, DQP_ERR_BAD_ARG)):
        dims = _lib.dqp_mpc_dims(nb, N, M, T, 1, 0)
        assert lib.dqp_mpc_assemble(ctypes.byref(dims), *([z] * 14)) == want
        assert lib.dqp_mpc_qp_forward(ctypes.byref(dims), ctypes.byref(opts), *([z] * 16)) == want
        assert lib.dqp_mpc_qp_forward_stepped(ctypes.byref(dims), ctypes.byref(opts), *([z] * 8), 0, 0, *([z] * 9)) == want
    assert lib.dqp_mpc_assemble(None, *([z] * 14)) == DQP_ERR_BAD_ARG
    assert lib.dqp_mpc_qp_forward(None, ctypes.byref(opts), *([z] * 16)) == DQP_ERR_BAD_ARG
    bad_T = _lib.dqp_mpc_dims(B, N, M, 1, 1, 0)
    assert lib.dqp_mpc_assemble(ctypes.byref(bad_T), *([z] * 14)) == DQP_ERR_BAD_ARG
    # the queries do not depend on the layout: same answers as before
    dims = _lib.dqp_mpc_dims(B, 3, 1, 10, 1, 0)
    assert lib.dqp_mpc_qp_supported(ctypes.byref(dims)) == 1
    assert lib.dqp_mpc_qp_workspace_bytes(ctypes.byref(dims)) > 0


# ------------------------------------------------------------------ the oracle on the reference's golden
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


def test_golden_has_active_and_inactive_rows_in_every_sample():
    g = dict(np.load(GOLDEN, allow_pickle=False))
    lo, hi, u = g["in_u_lower"], g["in_u_upper"], g["single_u"]
    Tg, Bg, mg = u.shape
    assert lo.shape == (Tg, Bg, mg) and (lo < hi).all()
    assert np.ptp(lo, axis=0).min() > 0 and np.ptp(lo, axis=1).min() > 0         # varies along the horizon and the batch
    gap = np.minimum(hi - u, u - lo).transpose(1, 0, 2).reshape(Bg, -1)
    assert (gap.min(1) <= 1e-6).all() and (gap.max(1) >= 0.02).all()
    assert (gap > -1e-9).all()


def test_oracle_reproduces_the_reference_golden(lib):
    """oracle.dense_forward / dense_backward on the numpy-assembled QP with h per (b, t, k) against the reference's
    qp_wrapper.MPC(single_qp_solve=True) run on the same bounds (the line search accepts the full step, so the returned
    trajectory is the QP solution and the gradients are those of the one QP)."""
    from oracle import oracle
    g = dict(np.load(GOLDEN, allow_pickle=False))
    C, c, F, f, x0 = [g["in_" + k] for k in ("C", "c", "F", "f", "x0")]
    Tg, Bg, nt = c.shape
    n = x0.shape[1]
    Q, p, G, h, A, b = assemble(C, c, F, f, x0, g["in_u_lower"], g["in_u_upper"])
    o = oracle.dense_forward(Q, p, G, h, A, b)
    tau = o["zhat"].reshape(Bg, Tg, nt)
    np.testing.assert_allclose(tau[..., :n].transpose(1, 0, 2), g["single_x"], **ZT)
    np.testing.assert_allclose(tau[..., n:].transpose(1, 0, 2), g["single_u"], **ZT)
    w = np.concatenate([np.ones((Bg, Tg, n)), 2.0 * np.ones((Bg, Tg, nt - n))], axis=-1)      # d(x.sum() + 2 u.sum())
    og = oracle.dense_backward(o["K"], o["zhat"], o["lam"], o["nu"], w.reshape(Bg, -1))
    dC = np.stack([og["dQ"][:, t * nt:(t + 1) * nt, t * nt:(t + 1) * nt] for t in range(Tg)])
    dc = np.stack([og["dp"][:, t * nt:(t + 1) * nt] for t in range(Tg)])
    dF = np.stack([og["dA"][:, t * n:(t + 1) * n, t * nt:(t + 1) * nt] for t in range(Tg - 1)])
    df = np.stack([-og["db"][:, t * n:(t + 1) * n] for t in range(Tg - 1)])
    dx0 = og["db"][:, (Tg - 1) * n:]
    for k, want in zip(("C", "c", "F", "f", "x0"), (dC, dc, dF, df, dx0)):
        np.testing.assert_allclose(want, g["single_d" + k], err_msg="d" + k, **GT)
