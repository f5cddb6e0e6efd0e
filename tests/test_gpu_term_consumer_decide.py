"""The batch rule's stop I* is decided where it is consumed (csrc/dqp_common.h: term_cap): term_scan_kernel leaves the
three iteration masks, every pass-2 wavefront replays the reference's rule on them, and the first lane of pass 2 writes
I* into the header.  Expected values come from the CPU oracle, never from the kernels:
  * family M at the metric size, B = 65 (two scan blocks, the second a single lane; 17 pass-2 wavefronts, the last with
    three dead rows): the rule stops early and most problems are taken back by the finish pass;
  * family R at the metric size, B = 5, with the rule out of reach (I* = max_iter, nothing flagged).  A batch of 5
    random QPs converges and stops at iteration 11-13 for every seed tried (0..29), so this case runs with
    max_iter = 10: the oracle's own run is asserted to use all 10 iterations and to flag nothing;
  * the same through the families that solve again in pass 2 (dqp_r16.hip, dqp_pdipm.hip) and the stage-wise path
    (dqp_ric_kernels.h);
  * a header left by an earlier call on the same termination buffer, eagerly and under graph capture and replay;
  * the multi-device entry points on one device (a positive header, written by term_decide_kernel).
The kernels use the guarded step (batch_LU.py:203-214; tests/test_gpu_parity.py::reference_outputs), so the stop
iteration is the guarded oracle's; on the dense batches the rule fires on best_resids.max() < eps with the maximum a
factor of 10 below eps at I* and a factor of 10 above it one iteration earlier (asserted below), far from round-off.
Tolerances and families are those of tests/test_gpu_parity.py."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import oracle
from families import family, family_mpc
from test_gpu_parity import ZT, DT, GT, dev, reference_outputs
from test_gpu_r16n_ctx_loads import c_backward
from test_gpu_ric import assemble, problem

pytestmark = pytest.mark.gpu

METRIC = (30, 30, 15)
EPS, NOT_IMPROVED_LIM = 1e-12, 3
M_SEED, R_SEED = 6, 7


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need a GPU"
    from diff_qp_mpc_amd import _lib
    return _lib.load()


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() > 0 else ctypes.c_void_p(0)


def header0(term, B, max_iter):
    """I* as the call left it in the termination buffer (csrc/dqp_term.hip: history, 24 bytes of masks, header)"""
    torch.cuda.synchronize()
    return int(term.view(torch.int32)[(max_iter * B * 16 + 24) // 4])


class Call:
    """dqp_qp_forward on device tensors through the C ABI, with its buffers kept so that a second call can reuse them"""

    def __init__(self, lib, ins, max_iter, flags=0):
        from diff_qp_mpc_amd import _lib
        self.lib, self.ins, self.max_iter = lib, ins, max_iter
        B, nz = ins[1].shape
        nineq, neq = ins[3].shape[1], ins[5].shape[1]
        self.B = B
        self.dims = _lib.dqp_dims(B, nz, nineq, neq, nz * nz, nz, nineq * nz, nineq, neq * nz, neq)
        self.opts = _lib.dqp_opts(EPS, 1e-10, max_iter, NOT_IMPROVED_LIM, _lib.DQP_FLAG_BATCH_TERMINATION | flags, 0)
        kw = dict(dtype=torch.float64, device="cuda")
        self.out = dict(zhat=torch.empty(B, nz, **kw), lam=torch.empty(B, nineq, **kw), nu=torch.empty(B, neq, **kw),
                        slack=torch.empty(B, nineq, **kw), info=torch.empty(B, 2, dtype=torch.int32, device="cuda"),
                        resid=torch.empty(B, **kw))
        wsb = int(lib.dqp_workspace_bytes(ctypes.byref(self.dims)))
        self.ws = torch.empty(max(wsb // 8, 1), **kw)
        self.tb = int(lib.dqp_termination_bytes(ctypes.byref(self.dims), ctypes.byref(self.opts)))
        assert self.tb > 0
        self.term = torch.zeros((self.tb + 7) // 8, **kw)

    def args(self, term=None):
        o = self.out
        return ([_p(t) for t in self.ins] + [_p(o[k]) for k in ("zhat", "lam", "nu", "slack", "info", "resid")] +
                [_p(self.ws), _p(self.term if term is None else term)])

    def run(self, term=None):
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert self.lib.dqp_qp_forward(ctypes.byref(self.dims), ctypes.byref(self.opts), *self.args(term), st) == 0
        return self

    def numpy(self):
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in self.out.items()}

    def header0(self, term=None):
        return header0(self.term if term is None else term, self.B, self.max_iter)


_ref = {}


def stop_of(ins, max_iter, forward=oracle.qp_forward, **kw):
    """-> (I* of the oracle's guarded run, per-problem flags of pass 2, margin of the deciding test), the last as
    (best_resids.max() one iteration before the stop, at the stop)"""
    stop = forward(*ins, maxIter=max_iter, **kw)["iters"]
    full = oracle.qp_forward(*ins, eps=0.0, notImprovedLim=10 ** 6, maxIter=max_iter, guard=True)
    assert full["iters"] == max_iter
    hist = np.where(np.isnan(full["resid_hist"]), np.inf, full["resid_hist"])
    worst = np.minimum.accumulate(hist, axis=1).max(0)
    return stop, hist.argmin(1) >= stop, (worst[stop - 2], worst[stop - 1])


def batch_M():
    """family M, B = 65 at the metric size: I* < max_iter, problems flagged"""
    if "M" not in _ref:
        B, max_iter = 65, 20
        ins = family_mpc(M_SEED, B)
        assert (ins[1].shape[1], ins[3].shape[1], ins[5].shape[1]) == METRIC
        ct = np.random.default_rng(M_SEED).standard_normal((B, METRIC[0]))
        o, differ, og = reference_outputs(ins, ct)
        istar, flagged, (before, at) = stop_of(ins, max_iter, guard=True)
        assert istar < max_iter and flagged.any()
        assert before > 10 * EPS and at < EPS / 10, (before, at)       # the stop is no matter of round-off
        assert (o["best_resid"] < 1e-8).all()
        _ref["M"] = (ins, ct, o, og, istar, max_iter)
    return _ref["M"]


def batch_R():
    """family R, B = 5 at the metric size, max_iter = 10: the rule never fires and nothing is taken back"""
    if "R" not in _ref:
        B, max_iter = 5, 10
        ins = family(R_SEED, B, *METRIC)
        ct = np.random.default_rng(R_SEED).standard_normal((B, METRIC[0]))
        o = oracle.qp_forward(*ins, maxIter=max_iter, guard=True)
        lit = oracle.qp_forward(*ins, maxIter=max_iter)
        assert all(np.array_equal(o[k], lit[k]) for k in ("zhat", "lam", "nu", "slack")), "step rules part ways"
        og = oracle.qp_backward(ins[0], ins[2], ins[4], o["zhat"], o["lam"], o["nu"], o["slack"], ct)
        istar, flagged, _ = stop_of(ins, max_iter, guard=True)
        assert istar == max_iter and not flagged.any()
        _ref["R"] = (ins, ct, o, og, istar, max_iter)
    return _ref["R"]


def check_outputs(out, o):
    assert int(np.abs(out["info"][:, 0]).max()) == 0
    np.testing.assert_allclose(out["zhat"], o["zhat"], **ZT)
    for k in ("lam", "nu", "slack"):
        np.testing.assert_allclose(out[k], o[k], err_msg=k, **DT)


@pytest.mark.parametrize("which", ["M", "R"])
def test_nullspace_kernels_decide_in_finish_pass(lib, which):
    ins_np, ct, o, og, istar, max_iter = batch_M() if which == "M" else batch_R()
    ins = [dev(a, grad=False) for a in ins_np]
    c = Call(lib, ins, max_iter).run()
    out = c.numpy()
    print("oracle I* = %d, header %d, iterations %s" % (istar, c.header0(), out["info"][:, 1]))
    assert c.header0() == istar
    check_outputs(out, o)
    # a problem taken back reports I*, every other one the max_iter iterations of pass 1
    assert set(np.unique(out["info"][:, 1])) <= {istar, max_iter}
    assert int(out["info"][:, 1].min()) == istar
    # gradients at the oracle's point, where strict complementarity holds (test_gpu_parity.py)
    gr = c_backward(lib, ins, c.dims, c.ws, o, ct)
    gm = np.maximum(o["lam"], o["slack"]).min(1) > 1e-5
    assert gm.sum() >= len(gm) - 2
    for k in og:
        np.testing.assert_allclose(gr[k][gm], og[k][gm], err_msg=k, **GT)


@pytest.mark.parametrize("which", ["M", "R"])
def test_row_kernels_solve_again_up_to_the_stop(lib, which):
    """DQP_FLAG_NO_NULLSPACE: dqp_r16.hip, whose pass 2 is a second solve clamped to I*"""
    from diff_qp_mpc_amd import _lib
    ins_np, _, o, _, istar, max_iter = batch_M() if which == "M" else batch_R()
    c = Call(lib, [dev(a, grad=False) for a in ins_np], max_iter, _lib.DQP_FLAG_NO_NULLSPACE).run()
    assert c.header0() == istar
    check_outputs(c.numpy(), o)


@pytest.mark.parametrize("max_iter", [20, 6])
def test_generic_kernels_solve_again_up_to_the_stop(lib, max_iter):
    """DQP_FLAG_GENERIC_ONLY at (10, 5, 3), B = 9: dqp_pdipm.hip.  max_iter = 20: the rule fires early; 6: never."""
    from diff_qp_mpc_amd import _lib
    ins_np = family(0, 9, 10, 5, 3)
    istar, flagged, (before, at) = stop_of(ins_np, max_iter, guard=True)
    if max_iter == 20:
        o, _ = reference_outputs(ins_np)
        assert istar < max_iter and flagged.any()
        assert before > 10 * EPS and at < EPS / 10, (before, at)
    else:
        o = oracle.qp_forward(*ins_np, maxIter=max_iter, guard=True)
        assert istar == max_iter and not flagged.any()
    c = Call(lib, [dev(a, grad=False) for a in ins_np], max_iter, _lib.DQP_FLAG_GENERIC_ONLY).run()
    assert c.header0() == istar
    check_outputs(c.numpy(), o)


@pytest.mark.parametrize("max_iter", [20, 6])
def test_stagewise_kernels_finish_at_the_stop(lib, max_iter):
    """dqp_mpc_qp_forward on the stage-wise kernels (dqp_ric_kernels.h) at n 3, m 3, T 5, B = 9, against the oracle's
    DenseQPFunction restatement on the assembled QP (tests/test_gpu_ric.py)."""
    from diff_qp_mpc_amd import _lib
    n, m, T, B = 3, 3, 5, 9
    data = problem(n, m, T, B, seed=5, active=0.2)
    o = oracle.dense_forward(*assemble(*data), maxIter=max_iter)
    istar = o["iters"]
    assert istar < max_iter if max_iter == 20 else istar == max_iter
    C, c, F, f, x0, lo, hi = [dev(a, grad=False) for a in data]
    dims = _lib.dqp_mpc_dims(B, n, m, T, 1, 0)
    opts = _lib.dqp_opts(EPS, 1e-10, max_iter, NOT_IMPROVED_LIM, _lib.DQP_FLAG_BATCH_TERMINATION | _lib.DQP_FLAG_STAGEWISE, 0)
    kw = dict(dtype=torch.float64, device="cuda")
    tau, lam, nu, slack = (torch.empty(B, k, **kw) for k in (T * (n + m), 2 * T * m, T * n, 2 * T * m))
    info, resid = torch.empty(B, 2, dtype=torch.int32, device="cuda"), torch.empty(B, **kw)
    ws = torch.empty(int(lib.dqp_mpc_qp_workspace_bytes(ctypes.byref(dims))) // 8 + 1, **kw)
    term = torch.zeros(int(lib.dqp_mpc_qp_termination_bytes(ctypes.byref(dims), ctypes.byref(opts))) // 8 + 1, **kw)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.dqp_mpc_qp_forward(ctypes.byref(dims), ctypes.byref(opts), *[_p(t) for t in (C, c, F, f, x0, lo, hi)],
                                  *[_p(t) for t in (tau, lam, nu, slack, info, resid)], _p(ws), _p(term), st) == 0
    assert header0(term, B, max_iter) == istar
    assert int(info[:, 0].abs().max()) == 0
    np.testing.assert_allclose(tau.cpu().numpy(), o["zhat"], **ZT)


def _pair(lib):
    """the two metric-size calls of the stale-header test, sharing the larger call's termination buffer"""
    m, r = batch_M(), batch_R()
    cm = Call(lib, [dev(a, grad=False) for a in m[0]], m[5])
    cr = Call(lib, [dev(a, grad=False) for a in r[0]], r[5])
    assert cm.tb >= cr.tb
    return cm, cr, r[4]


def test_header_of_an_earlier_call_is_not_read(lib):
    """I* < max_iter stays in the header after a call; the next call on the same buffer must decide for itself."""
    cm, cr, istar_r = _pair(lib)
    fresh = {k: v.clone() for k, v in cr.run().out.items()}       # on its own zeroed buffer
    assert cr.header0() == istar_r
    cm.run()
    assert 0 < cm.header0() < cm.max_iter
    cr.run(term=cm.term)
    assert cr.header0(cm.term) == istar_r
    for k, v in fresh.items():
        assert torch.equal(cr.out[k], v), k


def test_header_of_an_earlier_call_under_graph_replay(lib):
    cm, cr, istar_r = _pair(lib)
    fresh = {k: v.clone() for k, v in cr.run().out.items()}
    want_m = {k: v.clone() for k, v in cm.run().out.items()}
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        cm.run()
        cr.run(term=cm.term)                 # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cm.run()
        cr.run(term=cm.term)
    for _ in range(2):
        for c in (cm, cr):
            for v in c.out.values():
                v.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert cr.header0(cm.term) == istar_r
        for k, v in fresh.items():
            assert torch.equal(cr.out[k], v), k
        for k, v in want_m.items():
            assert torch.equal(cm.out[k], v), k


def test_multi_device_form_on_one_device(lib):
    """dqp_term_local_masks + dqp_qp_forward_finish with this shard's own masks equal the single call; the header
    they leave is the positive one term_decide_kernel wrote."""
    from diff_qp_mpc_amd import _lib
    ins_np, _, _, _, istar, max_iter = batch_M()
    ins = [dev(a, grad=False) for a in ins_np]
    one = Call(lib, ins, max_iter).run()
    want = {k: v.clone() for k, v in one.out.items()}
    two = Call(lib, ins, max_iter)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    opts1 = _lib.dqp_opts(EPS, 1e-10, max_iter, NOT_IMPROVED_LIM,
                          _lib.DQP_FLAG_BATCH_TERMINATION | _lib.DQP_FLAG_HISTORY_ONLY, 0)
    assert lib.dqp_qp_forward(ctypes.byref(two.dims), ctypes.byref(opts1), *two.args(), st) == 0
    masks = torch.zeros(3, dtype=torch.int64, device="cuda")
    assert lib.dqp_term_local_masks(ctypes.byref(two.dims), ctypes.byref(two.opts), _p(two.term), _p(masks), st) == 0
    assert two.header0() == 0                                    # the scan decides nothing
    assert lib.dqp_qp_forward_finish(ctypes.byref(two.dims), ctypes.byref(two.opts), *two.args(), _p(masks), st) == 0
    assert two.header0() == istar
    for k, v in want.items():
        assert torch.equal(two.out[k], v), k
