"""Memory traffic at the two ends of r16n::backward_kernel (csrc/dqp_r16n.hip): the caller's vectors (zhat, the
cotangent, lam, slack, nu) and the factorisation context at its head, the gradient rows at its tail.  What can go wrong
there is a lane past the end of a vector (sizes that are no multiple of 16: every compiled one), a dead QP row (B no
multiple of 4) and an output that is only 8-byte aligned, so these tests pin
  * gradients against the CPU oracle under a random cotangent at (30, 30, 15) with B = 1, 4, 5, at (10, 5, 3) with
    B = 3 and at (20, 10, 15) with B = 5, where strict complementarity holds (tests/test_gpu_parity.py);
  * dQ, dG, dA as views 8 bytes into their allocations: bit-identical to the aligned call;
  * the QPFunction path, forward and backward, on a batch where the finish pass has nothing to do and on one where it
    takes most problems back (finish_kernel then runs the epilogue from the context the backward kernel reads next).
They were written for a reordering of the head loads and 16-byte gradient stores, both measured and dropped
(DESIGN.md section 4.2), and stay as the net under the next attempt.
Tolerances and problem families are those of tests/test_gpu_parity.py."""
import ctypes

import numpy as np
import pytest
import torch

from test_gpu_parity import ZT, GT, dev
from test_gpu_r16n_ctx_loads import METRIC, _p, c_forward, reference

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need a GPU"
    from diff_qp_mpc_amd import _lib
    return _lib.load()


def backward(lib, ins, dims, ws, point, ct, off=()):
    """dqp_qp_backward from the context in `ws`; the outputs named in `off` start one double into their allocation"""
    from diff_qp_mpc_amd import _lib
    Q, _, G, _, A, _ = ins
    B, nz, nineq, neq = dims.nbatch, dims.nz, dims.nineq, dims.neq
    opts = _lib.dqp_opts(0.0, 0.0, 0, 0, _lib.DQP_FLAG_BACKWARD_CTX, 0)
    kw = dict(dtype=torch.float64, device="cuda")
    shapes = dict(dQ=(B, nz, nz), dp=(B, nz), dG=(B, nineq, nz), dh=(B, nineq), dA=(B, neq, nz), db=(B, neq))
    gr = {}
    for k, s in shapes.items():
        o = 1 if k in off else 0
        gr[k] = torch.empty(int(np.prod(s)) + 2, **kw)[o:o + int(np.prod(s))]
        assert gr[k].data_ptr() % 16 == 8 * o
    pt = [dev(point[k], grad=False) for k in ("zhat", "lam", "nu", "slack")]
    rc = lib.dqp_qp_backward(ctypes.byref(dims), ctypes.byref(opts), _p(Q), _p(G), _p(A), *[_p(t) for t in pt],
                             _p(dev(ct, grad=False)), *[_p(gr[k]) for k in ("dQ", "dp", "dG", "dh", "dA", "db")], None,
                             _p(ws), None)
    assert rc == 0
    torch.cuda.synchronize()
    return {k: gr[k].cpu().numpy().reshape(shapes[k]) for k in gr}


@pytest.mark.parametrize("shape,B", [(METRIC, 1), (METRIC, 4), (METRIC, 5), ((10, 5, 3), 3), ((20, 10, 15), 5)])
def test_gradients_vs_oracle(lib, shape, B):
    ins_np, ct, o, og = reference(shape, B)
    assert (o["best_resid"] < 1e-8).all()
    ins = [dev(a, grad=False) for a in ins_np]
    _, dims, ws = c_forward(lib, ins, "batch")
    gr = backward(lib, ins, dims, ws, o, ct)
    gm = np.maximum(o["lam"], o["slack"]).min(1) > 1e-5
    assert gm.sum() >= B - 1 and gm.any()
    for k in og:
        assert np.isfinite(gr[k]).all(), k
        np.testing.assert_allclose(gr[k][gm], og[k][gm], err_msg=k, **GT)


def test_matrix_gradients_8_byte_aligned_bit_identical(lib):
    ins_np, ct, o, _ = reference(METRIC, 5)
    ins = [dev(a, grad=False) for a in ins_np]
    _, dims, ws = c_forward(lib, ins, "batch")
    a = backward(lib, ins, dims, ws, o, ct)
    b = backward(lib, ins, dims, ws, o, ct, off=("dQ", "dG", "dA"))
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert np.isfinite(a["dQ"]).all() and np.abs(a["dQ"]).max() > 0


@pytest.mark.parametrize("which", ["R", "M"])
def test_qpfunction_forward_and_backward(lib, which):
    """R: B = 5, the finish pass returns at once; M: the batch of tests/test_gpu_term_consumer_decide.py, where
    finish_kernel restarts most problems from the context before the backward kernel reads it."""
    import diff_qp_mpc_amd as dqp
    if which == "R":
        ins_np, ct, o, og = reference(METRIC, 5)
    else:
        from test_gpu_term_consumer_decide import batch_M
        ins_np, ct, o, og = batch_M()[:4]
    ins = [dev(a) for a in ins_np]
    zhat = dqp.QPFunction(verbose=-1)(*ins)
    zhat.backward(dev(ct, grad=False))
    torch.cuda.synchronize()
    np.testing.assert_allclose(zhat.detach().cpu().numpy(), o["zhat"], **ZT)
    gm = np.maximum(o["lam"], o["slack"]).min(1) > 1e-5
    assert gm.sum() >= len(gm) - 2
    for k, t in zip("QpGhAb", ins):
        np.testing.assert_allclose(t.grad.cpu().numpy()[gm], og["d" + k][gm], err_msg="d" + k, **GT)
