"""The DPP-row kernels' T solve after three reorderings that change no floating-point operation (csrc/dqp_r16_prims.h,
dqp_r16n.hip, dqp_r16.hip): the PDIPM loop leaves before the Newton step that follows the last residual, lu_rows takes
the next pivot's reciprocal a step ahead, and the L sweep of a right-hand side known before the factorisation rides in
the trailing update (lu_rows_rhs + lu_solve_U).  Straight through the C ABI:
  * forward and backward against the CPU oracle at every compiled null-space size whose M takes another mask path --
    (10,5,3) one slot with M < 16, (20,10,15), (40,20,30) two slots partly filled, (30,30,15) -- with B = 4 and B = 5
    (a second wavefront with three dead QP rows), under both termination modes;
  * the early exit at its edges, max_iter = 1, 2 and 20: outputs and iteration counts against the oracle at the same
    max_iter, the backward from a max_iter = 1 context, DQP_FLAG_STRICT_GET_STEP at max_iter = 2, the recorded history
    up to and including the last iteration, and the batch rule's finish pass on a batch where it has work;
  * the kernels that run without a workspace (dqp_r16.hip), at (12,8,0) and (30,30,15).
Tolerances and problem families are those of tests/test_gpu_parity.py.

Iteration counts.  info[:, 1] is per problem.  At max_iter = 1 and 2 no rule of either mode can fire on these
families (no problem is below eps after one step, and the no-improvement limit is 3), so every problem reports
max_iter, which is also the oracle's count.  At max_iter = 20 the batch rule reports the batch's stop I* (the oracle's
count on family R) for the problems the finish pass took back and max_iter (pass 1 ran them all the way) for the
others; the per-problem mode stops each problem on its own, somewhere in 1..20."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import oracle
from families import family_mpc
from test_gpu_parity import ZT, DT, GT, dev, family_R, over_tolerance, reference_outputs
from test_gpu_r16n_ctx_loads import _p, c_backward

pytestmark = pytest.mark.gpu

METRIC = (30, 30, 15)
SMALL = (10, 5, 3)
NOT_IMPROVED_LIM = 3


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need a GPU"
    from diff_qp_mpc_amd import _lib
    return _lib.load()


def c_forward(lib, ins, termination, max_iter=20, flags=0, use_ws=True, want_term=False):
    """dqp_qp_forward on device tensors -> (dict of numpy outputs, dims, the workspace it filled[, termination])"""
    from diff_qp_mpc_amd import _lib
    Q, p, G, h, A, b = ins
    B, nz = p.shape
    nineq, neq = h.shape[1], b.shape[1]
    dims = _lib.dqp_dims(B, nz, nineq, neq, nz * nz, nz, nineq * nz, nineq, neq * nz, neq)
    flags |= _lib.DQP_FLAG_BATCH_TERMINATION if termination == "batch" else 0
    opts = _lib.dqp_opts(1e-12, 1e-10, max_iter, NOT_IMPROVED_LIM, flags, 0)
    kw = dict(dtype=torch.float64, device="cuda")
    zhat, lam, nu, slack = (torch.empty(B, n, **kw) for n in (nz, nineq, neq, nineq))
    info = torch.empty(B, 2, dtype=torch.int32, device="cuda")
    resid = torch.empty(B, **kw)
    ws = None
    if use_ws:
        wsb = int(lib.dqp_workspace_bytes(ctypes.byref(dims)))
        assert wsb > 0, "no null-space kernel for this size"
        ws = torch.empty(wsb // 8, **kw)
    tb = int(lib.dqp_termination_bytes(ctypes.byref(dims), ctypes.byref(opts)))
    term = torch.full(((tb + 7) // 8,), float("nan"), **kw) if tb > 0 else None
    rc = lib.dqp_qp_forward(ctypes.byref(dims), ctypes.byref(opts), _p(Q), _p(p), _p(G), _p(h), _p(A), _p(b),
                            _p(zhat), _p(lam), _p(nu), _p(slack), _p(info), _p(resid), _p(ws), _p(term), None)
    assert rc == 0
    torch.cuda.synchronize()
    out = dict(zhat=zhat, lam=lam, nu=nu, slack=slack, info=info, resid=resid)
    out = {k: v.cpu().numpy() for k, v in out.items()}
    return (out, dims, ws, term) if want_term else (out, dims, ws)


def c_backward_no_workspace(lib, ins, dims, point, ct):
    """dqp_qp_backward with a null workspace and without DQP_FLAG_BACKWARD_CTX (r16::backward_kernel refactors), at
    the forward point `point` -> dict of numpy gradients"""
    from diff_qp_mpc_amd import _lib
    Q, _, G, _, A, _ = ins
    B, nz, nineq, neq = dims.nbatch, dims.nz, dims.nineq, dims.neq
    opts = _lib.dqp_opts(0.0, 0.0, 0, 0, 0, 0)
    kw = dict(dtype=torch.float64, device="cuda")
    shapes = dict(dQ=(B, nz, nz), dp=(B, nz), dG=(B, nineq, nz), dh=(B, nineq), dA=(B, neq, nz), db=(B, neq))
    gr = {k: torch.empty(max(int(np.prod(s)), 1), **kw)[:int(np.prod(s))] for k, s in shapes.items()}
    pt = [dev(point[k], grad=False) for k in ("zhat", "lam", "nu", "slack")]
    g = dev(ct, grad=False)
    rc = lib.dqp_qp_backward(ctypes.byref(dims), ctypes.byref(opts), _p(Q), _p(G), _p(A), *[_p(t) for t in pt], _p(g),
                             *[_p(gr[k]) for k in ("dQ", "dp", "dG", "dh", "dA", "db")], None, None, None)
    assert rc == 0
    torch.cuda.synchronize()
    return {k: gr[k].cpu().numpy().reshape(shapes[k]) for k in gr}


_ref = {}


def reference(shape, B, max_iter=20):
    """family R inputs, cotangent, oracle forward at max_iter and oracle backward from it: computed once per key,
    read-only.  The literal and the guarded step rule must agree on the case (tests/test_gpu_parity.py:
    reference_outputs), so the expectation does not hang on an exactly-zero step component."""
    key = (shape, B, max_iter)
    if key not in _ref:
        nz, nineq, neq = shape
        ins = family_R(7, B, nz, nineq, neq)
        ct = np.random.default_rng(1).standard_normal((B, nz))
        o = oracle.qp_forward(*ins, maxIter=max_iter)
        assert not over_tolerance(o, oracle.qp_forward(*ins, maxIter=max_iter, guard=True)).any()
        og = oracle.qp_backward(ins[0], ins[2], ins[4], o["zhat"], o["lam"], o["nu"], o["slack"], ct)
        for a in list(ins) + [ct] + list(og.values()) + [v for v in o.values() if isinstance(v, np.ndarray)]:
            a.setflags(write=False)
        _ref[key] = (ins, ct, o, og)
    return _ref[key]


def check_forward(out, o):
    assert int(np.abs(out["info"][:, 0]).max()) == 0
    np.testing.assert_allclose(out["zhat"], o["zhat"], **ZT)
    for k in ("lam", "nu", "slack"):
        np.testing.assert_allclose(out[k], o[k], err_msg=k, **DT)


STALL_TOL = 1e-10                      # c_forward's dqp_opts
RESID_FLOOR = 1e-11                    # ten times the largest residual the oracle converges to on these families (8e-13)


def per_problem_bounds(ins_np, max_iter):
    """The per-problem mode stops a problem at the first count at which its best residual is below 0.1 eps = 1e-13
    (csrc/dqp_pdipm.hip: fill_opts), or below stall_tol with no improvement for the limit (include/dqp.h).  1e-13 is
    the level the residuals of these families converge to, so which of the two fires, and when, moves with the
    coordinates the residual is computed in; what each problem's own oracle history pins (no rule able to fire, guarded
    step: the problems do not interact, so this is the batch-of-one run of each) is a window:
      * lo: every rule needs the best residual below stall_tol, so the count is at least the one at which the oracle's
        first falls below it, widened by the level at which two coordinate systems differ (RESID_FLOOR);
      * hi: from the count at which the oracle's best is within RESID_FLOOR of its final value, any further
        improvement is round-off; the no-improvement rule then fires after the limit, plus one count for one such
        improvement.
    The window is five to six counts wide at 8 to 14 iterations: it catches a count left at an early value or a
    problem run on to max_iter, not a count that is off by one (max_iter = 1 and 2, where the count is exact, and the
    bit-identity of info with the parent build pin that).
    -> (lo, hi), each (B,)"""
    key = ("bounds", id(ins_np), max_iter)
    if key not in _ref:
        full = oracle.qp_forward(*ins_np, eps=0.0, notImprovedLim=10 ** 6, maxIter=max_iter, guard=True)
        best = np.minimum.accumulate(np.where(np.isnan(full["resid_hist"]), np.inf, full["resid_hist"]), 1)

        def first(mask):
            return np.where(mask.any(1), mask.argmax(1) + 1, max_iter)
        lo = first(best < STALL_TOL + RESID_FLOOR)
        hi = np.minimum(max_iter, first(best - best[:, -1:] < RESID_FLOOR) + NOT_IMPROVED_LIM + 1)
        _ref[key] = (lo, hi, ins_np)      # (keeps ins_np's id alive)
    return _ref[key][:2]


def check_iterations(out, o, termination, max_iter, ins_np):
    it = out["info"][:, 1]
    if max_iter <= 2:
        assert int(o["iters"]) == max_iter
        assert (it == max_iter).all(), it
    elif termination == "batch":
        assert np.isin(it, (int(o["iters"]), max_iter)).all(), (it, o["iters"])
    else:
        lo, hi = per_problem_bounds(ins_np, max_iter)
        print("per-problem iterations %s, oracle bounds lo %s hi %s" % (it, lo, hi))
        assert ((lo <= it) & (it <= hi)).all(), (it, lo, hi)


@pytest.mark.parametrize("termination", ["batch", "per_problem"])
@pytest.mark.parametrize("B", [4, 5])
@pytest.mark.parametrize("shape", [SMALL, (20, 10, 15), (40, 20, 30), METRIC], ids=lambda s: "%dx%dx%d" % s)
def test_forward_backward_vs_oracle(lib, shape, B, termination):
    from diff_qp_mpc_amd import _build
    assert shape in _build.R16N_SIZES
    ins_np, ct, o, og = reference(shape, B)
    ins = [dev(a, grad=False) for a in ins_np]
    out, dims, ws = c_forward(lib, ins, termination)
    cm = o["best_resid"] < 1e-8
    assert cm.all(), "the reference itself did not converge on %s" % np.nonzero(~cm)[0]
    check_forward(out, o)
    check_iterations(out, o, termination, 20, ins_np)
    # backward restarts from the context this forward left, at the oracle's forward point (a gradient taken at the
    # kernels' own point moves with d = lam / slack of weakly active constraints)
    gr = c_backward(lib, ins, dims, ws, o, ct)
    for k in og:
        np.testing.assert_allclose(gr[k], og[k], err_msg=k, **GT)


@pytest.mark.parametrize("termination", ["batch", "per_problem"])
@pytest.mark.parametrize("max_iter", [1, 2, 20])
@pytest.mark.parametrize("shape", [SMALL, METRIC], ids=lambda s: "%dx%dx%d" % s)
def test_early_exit_at_its_edges(lib, shape, max_iter, termination):
    """max_iter = 1: the loop runs the residual and the bookkeeping of the initial point and leaves -- the result is
    the initial point, and the backward kernel still finds a complete context.  max_iter = 2: one step is taken,
    the one after the second residual is not."""
    B = 5
    ins_np, ct, o, og = reference(shape, B, max_iter)
    ins = [dev(a, grad=False) for a in ins_np]
    out, dims, ws = c_forward(lib, ins, termination, max_iter=max_iter)
    check_forward(out, o)
    check_iterations(out, o, termination, max_iter, ins_np)
    np.testing.assert_allclose(out["resid"], o["best_resid"], rtol=1e-5, atol=1e-9)
    gr = c_backward(lib, ins, dims, ws, o, ct)
    for k in og:
        np.testing.assert_allclose(gr[k], og[k], err_msg=k, **GT)


def test_strict_get_step_at_max_iter_2(lib):
    """DQP_FLAG_STRICT_GET_STEP only ever freezes a problem after a step; the step after the last residual is not
    taken any more, and nothing read its freeze.  On a case where the literal and the guarded oracle agree (no
    exactly-zero step component in the reference's arithmetic) the flag changes nothing within the tolerances."""
    from diff_qp_mpc_amd import _lib
    ins_np, _, o, _ = reference(METRIC, 5, 2)
    ins = [dev(a, grad=False) for a in ins_np]
    for termination in ("batch", "per_problem"):
        out, _, _ = c_forward(lib, ins, termination, max_iter=2, flags=_lib.DQP_FLAG_STRICT_GET_STEP)
        check_forward(out, o)
        # no freeze can occur before the second residual on this batch, and the one after it is no longer computed:
        # the count is the oracle's, 2, in both modes
        assert int(o["iters"]) == 2
        assert (out["info"][:, 1] == 2).all(), out["info"][:, 1]


def test_history_includes_the_last_iteration(lib):
    """Pass 1 of the batch rule records (resid, mu) of every iteration it ran, the last one included (hist_put comes
    before the exit), against the oracle run to max_iter with no rule able to fire."""
    from diff_qp_mpc_amd import _lib
    B, max_iter = 5, 20
    ins_np = reference(METRIC, B)[0]
    full = oracle.qp_forward(*ins_np, eps=0.0, notImprovedLim=10 ** 6, guard=True)
    assert full["iters"] == max_iter
    ins = [dev(a, grad=False) for a in ins_np]
    out, _, _, term = c_forward(lib, ins, "batch", flags=_lib.DQP_FLAG_HISTORY_ONLY, want_term=True)
    hist = term[:max_iter * B * 2].cpu().numpy().reshape(max_iter, B, 2)[:, :, 0].T      # (B, max_iter)
    assert np.isfinite(hist).all(), "an iteration left no history"
    assert (out["info"][:, 1] == max_iter).all()
    ref = full["resid_hist"]
    big = ref > 1e-7             # below that a residual is round-off of the coordinates it is computed in
    assert big[:, :4].all()
    np.testing.assert_allclose(hist[big], ref[big], rtol=1e-4)
    np.testing.assert_allclose(out["resid"], hist.min(1), rtol=0, atol=0)


def test_finish_pass_has_work(lib):
    """Family M under the batch rule: the rule stops at I* < max_iter and finish_kernel takes back the problems whose
    best iterate came at or after I* (as tests/test_gpu_r16n_ctx_loads.py builds it)."""
    B, seed, max_iter = 8, 0, 20
    ins_np = family_mpc(seed, B)
    ct = np.random.default_rng(seed).standard_normal((B, METRIC[0]))
    o, differ, og = reference_outputs(ins_np, ct)
    assert not differ.any()
    istar = oracle.qp_forward(*ins_np)["iters"]
    assert istar < max_iter
    full = oracle.qp_forward(*ins_np, eps=0.0, notImprovedLim=10 ** 6, guard=True)
    hist = np.where(np.isnan(full["resid_hist"]), np.inf, full["resid_hist"])
    flagged = hist.argmin(1) >= istar
    assert flagged.any()
    ins = [dev(a, grad=False) for a in ins_np]
    out, dims, ws = c_forward(lib, ins, "batch")
    assert (o["best_resid"] < 1e-8).all()
    check_forward(out, o)
    # the finish pass had work: the problems it took back report the batch's stop, the others pass 1's max_iter.  (The
    # stop itself is not compared with the oracle's: on this family the rule that fires is best_resids.max() < eps on
    # residuals at round-off level, 1e-13, so the iteration it fires at moves with the coordinates the residual is
    # computed in; the outputs above are what the rule is for.)
    it = out["info"][:, 1]
    taken_back = it < max_iter
    assert taken_back.any() and len(set(it[taken_back])) == 1 and int(it[taken_back][0]) >= 1, it
    gr = c_backward(lib, ins, dims, ws, out, ct)
    gm = np.maximum(o["lam"], o["slack"]).min(1) > 1e-5          # where strict complementarity holds
    assert gm.sum() >= B - 1
    for k in og:
        np.testing.assert_allclose(gr[k][gm], og[k][gm], err_msg=k, **GT)


@pytest.mark.parametrize("termination", ["batch", "per_problem"])
@pytest.mark.parametrize("shape", [(12, 8, 0), METRIC], ids=lambda s: "%dx%dx%d" % s)
def test_without_a_workspace(lib, shape, termination):
    """The equality-row kernels (dqp_r16.hip) run when no workspace is given: same early exit, same folded sweep in
    the forward and in the backward kernel (which refactors: no context, no DQP_FLAG_BACKWARD_CTX)."""
    from diff_qp_mpc_amd import _build
    assert shape in _build.R16_SIZES
    B = 5
    nz, nineq, neq = shape
    key = (shape, B, "r16")
    if key not in _ref:
        ins_np = family_R(7, B, nz, nineq, neq)
        o = oracle.qp_forward(*ins_np)
        assert not over_tolerance(o, oracle.qp_forward(*ins_np, guard=True)).any()
        ct = np.random.default_rng(1).standard_normal((B, nz))
        og = oracle.qp_backward(ins_np[0], ins_np[2], ins_np[4], o["zhat"], o["lam"], o["nu"], o["slack"], ct)
        _ref[key] = (ins_np, o, ct, og)
    ins_np, o, ct, og = _ref[key]
    assert (o["best_resid"] < 1e-8).all()
    ins = [dev(a, grad=False) for a in ins_np]
    out, dims, _ = c_forward(lib, ins, termination, use_ws=False)
    check_forward(out, o)
    check_iterations(out, o, termination, 20, ins_np)
    gr = c_backward_no_workspace(lib, ins, dims, o, ct)
    for k in og:
        np.testing.assert_allclose(gr[k], og[k], err_msg=k, **GT)
    out1, _, _ = c_forward(lib, ins, termination, max_iter=1, use_ws=False)
    o1 = oracle.qp_forward(*ins_np, maxIter=1)
    check_forward(out1, o1)
    assert (out1["info"][:, 1] == 1).all()
