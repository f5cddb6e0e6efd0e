"""The null-space DPP-row kernels' context copies (csrc/dqp_r16n.hip: ctx_fetch / ctx_stash / lds_to_ctx): the
packed Lq and the reflector tails travel between the caller's workspace and LDS in fixed-trip-count bursts whose
last chunk is partial (metric size: tri(30) = 465 and tailsz = 330 are no multiples of 16), so these tests pin,
straight through the C ABI,
  * forward and backward against the CPU oracle at the metric size and at the smallest compiled null-space size,
    with B = 4 (one full wavefront) and B = 5 (a second wavefront with three dead QP rows, which re-run QP B - 1),
    under both termination modes;
  * a workspace and gradient outputs that are 8-byte but not 16-byte aligned: bit-identical to the aligned call;
  * the batch rule's finish pass (finish_kernel restarts from the context) on a batch where it has work to do.
Tolerances and problem families are those of tests/test_gpu_parity.py."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import oracle
from families import family_mpc
from test_gpu_parity import ZT, DT, GT, dev, family_R, reference_outputs

pytestmark = pytest.mark.gpu

METRIC = (30, 30, 15)
MAX_ITER, NOT_IMPROVED_LIM = 20, 3


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need a GPU"
    from diff_qp_mpc_amd import _lib
    return _lib.load()


def smallest_nullspace_size():
    from diff_qp_mpc_amd import _build
    return min(_build.R16N_SIZES)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() > 0 else ctypes.c_void_p(0)


def _offset_empty(numel, off, **kw):
    """`numel` elements that start `off` elements into a fresh allocation."""
    return torch.empty(numel + off, **kw)[off:]


def c_forward(lib, ins, termination, ws_off=0):
    """dqp_qp_forward on device tensors -> (dict of numpy outputs, dims, the workspace it filled)"""
    from diff_qp_mpc_amd import _lib
    Q, p, G, h, A, b = ins
    B, nz = p.shape
    nineq, neq = h.shape[1], b.shape[1]
    dims = _lib.dqp_dims(B, nz, nineq, neq, nz * nz, nz, nineq * nz, nineq, neq * nz, neq)
    flags = _lib.DQP_FLAG_BATCH_TERMINATION if termination == "batch" else 0
    opts = _lib.dqp_opts(1e-12, 1e-10, MAX_ITER, NOT_IMPROVED_LIM, flags, 0)
    kw = dict(dtype=torch.float64, device="cuda")
    zhat, lam, nu, slack = (torch.empty(B, n, **kw) for n in (nz, nineq, neq, nineq))
    info = torch.empty(B, 2, dtype=torch.int32, device="cuda")
    resid = torch.empty(B, **kw)
    wsb = int(lib.dqp_workspace_bytes(ctypes.byref(dims)))
    assert wsb > 0, "no null-space kernel for this size"
    ws = _offset_empty(wsb // 8, ws_off, **kw)
    assert ws.data_ptr() % 16 == 8 * (ws_off % 2)
    tb = int(lib.dqp_termination_bytes(ctypes.byref(dims), ctypes.byref(opts)))
    term = torch.empty((tb + 7) // 8, **kw) if tb > 0 else None
    rc = lib.dqp_qp_forward(ctypes.byref(dims), ctypes.byref(opts), _p(Q), _p(p), _p(G), _p(h), _p(A), _p(b),
                            _p(zhat), _p(lam), _p(nu), _p(slack), _p(info), _p(resid), _p(ws), _p(term), None)
    assert rc == 0
    torch.cuda.synchronize()
    out = dict(zhat=zhat, lam=lam, nu=nu, slack=slack, info=info, resid=resid)
    return {k: v.cpu().numpy() for k, v in out.items()}, dims, ws


def c_backward(lib, ins, dims, ws, point, ct, grad_off=0):
    """dqp_qp_backward restarting from the context in `ws`, at the forward point `point` (numpy zhat, lam, nu,
    slack) -> dict of numpy gradients"""
    from diff_qp_mpc_amd import _lib
    Q, _, G, _, A, _ = ins
    B, nz, nineq, neq = dims.nbatch, dims.nz, dims.nineq, dims.neq
    opts = _lib.dqp_opts(0.0, 0.0, 0, 0, _lib.DQP_FLAG_BACKWARD_CTX, 0)
    kw = dict(dtype=torch.float64, device="cuda")
    shapes = dict(dQ=(B, nz, nz), dp=(B, nz), dG=(B, nineq, nz), dh=(B, nineq), dA=(B, neq, nz), db=(B, neq))
    gr = {k: _offset_empty(int(np.prod(s)), grad_off, **kw) for k, s in shapes.items()}
    for t in gr.values():
        assert t.data_ptr() % 16 == 8 * (grad_off % 2)
    pt = [dev(point[k], grad=False) for k in ("zhat", "lam", "nu", "slack")]
    g = dev(ct, grad=False)
    rc = lib.dqp_qp_backward(ctypes.byref(dims), ctypes.byref(opts), _p(Q), _p(G), _p(A), *[_p(t) for t in pt], _p(g),
                             *[_p(gr[k]) for k in ("dQ", "dp", "dG", "dh", "dA", "db")], None, _p(ws), None)
    assert rc == 0
    torch.cuda.synchronize()
    return {k: gr[k].cpu().numpy().reshape(shapes[k]) for k in gr}


_ref = {}


def reference(shape, B):
    """family R inputs, cotangent, oracle forward and oracle backward: computed once per (shape, B), read-only"""
    if (shape, B) not in _ref:
        nz, nineq, neq = shape
        ins = family_R(7, B, nz, nineq, neq)
        ct = np.random.default_rng(1).standard_normal((B, nz))
        o = oracle.qp_forward(*ins)
        og = oracle.qp_backward(ins[0], ins[2], ins[4], o["zhat"], o["lam"], o["nu"], o["slack"], ct)
        for a in list(ins) + [ct] + list(og.values()) + [v for v in o.values() if isinstance(v, np.ndarray)]:
            a.setflags(write=False)
        _ref[(shape, B)] = (ins, ct, o, og)
    return _ref[(shape, B)]


@pytest.mark.parametrize("termination", ["batch", "per_problem"])
@pytest.mark.parametrize("B", [4, 5])
@pytest.mark.parametrize("shape", ["metric", "smallest"])
def test_forward_backward_vs_oracle(lib, shape, B, termination):
    shape = METRIC if shape == "metric" else smallest_nullspace_size()
    ins_np, ct, o, og = reference(shape, B)
    ins = [dev(a, grad=False) for a in ins_np]
    out, dims, ws = c_forward(lib, ins, termination)
    assert int(np.abs(out["info"][:, 0]).max()) == 0
    cm = o["best_resid"] < 1e-8
    assert cm.all(), "the reference itself did not converge on %s" % np.nonzero(~cm)[0]
    np.testing.assert_allclose(out["zhat"], o["zhat"], **ZT)
    for k in ("lam", "nu", "slack"):
        np.testing.assert_allclose(out[k], o[k], err_msg=k, **DT)
    # the backward kernel restarts from the context this forward left, at the oracle's forward point: every
    # problem is compared (a gradient taken at the kernels' own point moves with d = lam / slack of weakly
    # active constraints, tests/test_gpu_parity.py::test_ragged_batches_at_dpp_row_size)
    gr = c_backward(lib, ins, dims, ws, o, ct)
    for k in og:
        np.testing.assert_allclose(gr[k], og[k], err_msg=k, **GT)


def test_misaligned_workspace_and_gradients_bit_identical(lib):
    """A workspace view and gradient outputs one double into their allocations (8-byte, not 16-byte aligned)."""
    ins_np, ct, _, _ = reference(METRIC, 5)
    ins = [dev(a, grad=False) for a in ins_np]
    runs = []
    for off in (0, 1):
        out, dims, ws = c_forward(lib, ins, "batch", ws_off=off)
        gr = c_backward(lib, ins, dims, ws, out, ct, grad_off=off)
        runs.append((out, gr))
    (out0, gr0), (out1, gr1) = runs
    for k in out0:
        assert np.array_equal(out0[k], out1[k]), k
    for k in gr0:
        assert np.array_equal(gr0[k], gr1[k]), k
    assert np.isfinite(gr0["dQ"]).all()


def test_finish_pass_from_context(lib):
    """Family M under the batch rule: the rule stops early and problems whose best iterate came at or after the
    stop I* are taken back by finish_kernel, which loads the context (load_ctx) and runs the epilogue only."""
    B, seed = 8, 0
    ins_np = family_mpc(seed, B)
    assert ins_np[1].shape[1:] == (METRIC[0],) and ins_np[3].shape[1] == METRIC[1] and ins_np[5].shape[1] == METRIC[2]
    ct = np.random.default_rng(seed).standard_normal((B, METRIC[0]))
    o, differ, og = reference_outputs(ins_np, ct)
    assert not differ.any(), "seed on which the reference's two step rules part ways"
    istar = oracle.qp_forward(*ins_np)["iters"]
    assert istar < MAX_ITER
    # Pass 1 on the device runs every problem to maxIter and keeps its best iterate of all of them; the same on
    # the oracle: no rule can fire (eps = 0, no-improvement limit out of reach), with the guarded step the
    # kernels use (the literal get_step freezes a problem on an exactly-zero step component)
    full = oracle.qp_forward(*ins_np, eps=0.0, notImprovedLim=10 ** 6, guard=True)
    assert full["iters"] == MAX_ITER
    hist = np.where(np.isnan(full["resid_hist"]), np.inf, full["resid_hist"])
    flagged = hist.argmin(1) >= istar
    print("I* = %d, own best iterations %s" % (istar, hist.argmin(1)))
    assert flagged.any()
    ins = [dev(a, grad=False) for a in ins_np]
    out, dims, ws = c_forward(lib, ins, "batch")
    assert int(np.abs(out["info"][:, 0]).max()) == 0
    cm = o["best_resid"] < 1e-8
    assert cm.all()
    np.testing.assert_allclose(out["zhat"], o["zhat"], **ZT)
    for k in ("lam", "nu", "slack"):
        np.testing.assert_allclose(out[k], o[k], err_msg=k, **DT)
    gr = c_backward(lib, ins, dims, ws, out, ct)
    # gradients where strict complementarity holds (tests/test_gpu_parity.py::test_stress_families_metric_shape)
    gm = np.maximum(o["lam"], o["slack"]).min(1) > 1e-5
    assert gm.sum() >= B - 1
    for k in og:
        np.testing.assert_allclose(gr[k][gm], og[k][gm], err_msg=k, **GT)
