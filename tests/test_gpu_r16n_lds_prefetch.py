"""The LDS operand prefetch of the DPP-row kernels (csrc/dqp_r16_prims.h: the column ring of tri_solve / tri_solve_T /
tri_mv; csrc/dqp_r16n.hip: the next reflector's tail in apply_Qf / apply_QfT, the 8-double stream of Lq entries in
the setup's row solves, the epilogue's parked iterate read ahead of the tails' barriers).  The prefetched forms run the
same floating-point operations on the same values as the plain ones (which the three-slot sizes keep), so these tests pin,
straight through the C ABI,
  * forward and context backward against the CPU oracle at every compiled null-space size -- the two-slot sizes, the
    two three-slot sizes whose setup does the G pass on its own, and (10, 5, 3), whose ring of four columns is longer
    than its 3 x 3 triangle -- with B = 4 (one full wavefront) and B = 5 (a second wavefront with three dead QP rows),
    under both termination modes;
  * the kernels that keep the equality rows (no workspace: r16::forward_kernel / backward_kernel share the prims) at
    the metric size and at (12, 8, 0), which has no equalities;
  * the batch rule's finish pass (load_ctx, then the epilogue) on a batch where it has work to do;
  * bit identity with the build before the prefetch: tests/golden/r16n_parent_b4.npz holds what that build wrote for
    family R, seed 0, B = 4 -- the twelve outputs of a forward + context backward at the metric size under the batch
    rule, and the four forward outputs at (40, 20, 30).
Tolerances and problem families are those of tests/test_gpu_parity.py."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import oracle
from families import family_mpc
from test_gpu_parity import ZT, DT, GT, GOLDEN, dev, family_R, reference_outputs
from test_gpu_r16n_ctx_loads import METRIC, MAX_ITER, NOT_IMPROVED_LIM, _p, c_backward, c_forward
from test_gpu_r16n_ctx_loads import lib  # noqa: F401  (the module's fixture)

pytestmark = pytest.mark.gpu

PARENT = os.path.join(GOLDEN, "r16n_parent_b4.npz")
THREE_SLOT = (40, 20, 30)
FORWARD_KEYS = ("zhat", "lam", "nu", "slack")


def nullspace_sizes():
    from diff_qp_mpc_amd import _build
    return sorted(_build.R16N_SIZES)


_ref = {}


def reference(shape, B):
    """family R inputs (no equalities: A, b empty), cotangent, oracle forward, which samples the literal and the
    guarded reference disagree on, oracle backward: computed once per (shape, B), read-only"""
    if (shape, B) not in _ref:
        nz, nineq, neq = shape
        ins = list(family_R(11, B, nz, nineq, max(neq, 1)))
        if neq == 0:
            ins[4], ins[5] = np.zeros((B, 0, nz)), np.zeros((B, 0))
        ct = np.random.default_rng(2).standard_normal((B, nz))
        o, differ, og = reference_outputs(ins, ct)
        for a in list(ins) + [ct, differ] + list(og.values()) + [v for v in o.values() if isinstance(v, np.ndarray)]:
            a.setflags(write=False)
        _ref[(shape, B)] = (ins, ct, o, differ, og)
    return _ref[(shape, B)]


def check_forward(out, o):
    assert int(np.abs(out["info"][:, 0]).max()) == 0
    cm = o["best_resid"] < 1e-8
    assert cm.all(), "the reference itself did not converge on %s" % np.nonzero(~cm)[0]
    np.testing.assert_allclose(out["zhat"], o["zhat"], **ZT)
    for k in ("lam", "nu", "slack"):
        np.testing.assert_allclose(out[k], o[k], err_msg=k, **DT)


@pytest.mark.parametrize("termination", ["batch", "per_problem"])
@pytest.mark.parametrize("B", [4, 5])
@pytest.mark.parametrize("shape", nullspace_sizes(), ids=lambda s: "%dx%dx%d" % s)
def test_nullspace_sizes_vs_oracle(lib, shape, B, termination):  # noqa: F811
    ins_np, ct, o, differ, og = reference(shape, B)
    assert not differ.any(), "seed on which the reference's two step rules part ways"
    ins = [dev(a, grad=False) for a in ins_np]
    out, dims, ws = c_forward(lib, ins, termination)
    check_forward(out, o)
    # the backward kernel restarts from the context this forward left, at the oracle's forward point (a gradient
    # taken at the kernels' own point moves with d = lam / slack of weakly active constraints)
    gr = c_backward(lib, ins, dims, ws, o, ct)
    for k in og:
        np.testing.assert_allclose(gr[k], og[k], err_msg=k, **GT)


def forward_backward_without_workspace(lib, ins, point, ct):  # noqa: F811
    """dqp_qp_forward / dqp_qp_backward with no workspace: the kernels that keep the equality rows"""
    from diff_qp_mpc_amd import _lib
    Q, p, G, h, A, b = ins
    B, nz = p.shape
    nineq, neq = h.shape[1], b.shape[1]
    dims = _lib.dqp_dims(B, nz, nineq, neq, nz * nz, nz, nineq * nz, nineq, neq * nz, neq)
    opts = _lib.dqp_opts(1e-12, 1e-10, MAX_ITER, NOT_IMPROVED_LIM, 0, 0)
    kw = dict(dtype=torch.float64, device="cuda")
    zhat, lam, nu, slack = (torch.empty(B, n, **kw) for n in (nz, nineq, neq, nineq))
    info = torch.empty(B, 2, dtype=torch.int32, device="cuda")
    resid = torch.empty(B, **kw)
    rc = lib.dqp_qp_forward(ctypes.byref(dims), ctypes.byref(opts), _p(Q), _p(p), _p(G), _p(h), _p(A), _p(b),
                            _p(zhat), _p(lam), _p(nu), _p(slack), _p(info), _p(resid), None, None, None)
    assert rc == 0
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in dict(zhat=zhat, lam=lam, nu=nu, slack=slack, info=info).items()}
    bopts = _lib.dqp_opts(0.0, 0.0, 0, 0, 0, 0)
    shapes = dict(dQ=(B, nz, nz), dp=(B, nz), dG=(B, nineq, nz), dh=(B, nineq), dA=(B, neq, nz), db=(B, neq))
    gr = {k: torch.empty(s, **kw) for k, s in shapes.items()}
    pt = [dev(point[k], grad=False) for k in FORWARD_KEYS]
    rc = lib.dqp_qp_backward(ctypes.byref(dims), ctypes.byref(bopts), _p(Q), _p(G), _p(A), *[_p(t) for t in pt],
                             _p(dev(ct, grad=False)), *[_p(gr[k]) for k in ("dQ", "dp", "dG", "dh", "dA", "db")],
                             None, None, None)
    assert rc == 0
    torch.cuda.synchronize()
    return out, {k: v.cpu().numpy() for k, v in gr.items()}


@pytest.mark.parametrize("shape", [METRIC, (12, 8, 0)], ids=lambda s: "%dx%dx%d" % s)
def test_without_workspace_vs_oracle(lib, shape):  # noqa: F811
    ins_np, ct, o, differ, og = reference(shape, 5)
    assert not differ.any()
    out, gr = forward_backward_without_workspace(lib, [dev(a, grad=False) for a in ins_np], o, ct)
    check_forward(out, o)
    for k in og:
        if shape[2] == 0 and k in ("dA", "db"):
            continue
        np.testing.assert_allclose(gr[k], og[k], err_msg=k, **GT)


def test_finish_pass_epilogue(lib):  # noqa: F811
    """MPC-structured batch under the batch rule with I* < maxIter: the problems whose best iterate came at or after
    the stop go through finish_kernel, i.e. load_ctx and then the epilogue alone."""
    B, seed = 8, 0
    ins_np = family_mpc(seed, B)
    assert (ins_np[1].shape[1], ins_np[3].shape[1], ins_np[5].shape[1]) == METRIC
    ct = np.random.default_rng(seed).standard_normal((B, METRIC[0]))
    o, differ, og = reference_outputs(ins_np, ct)
    assert not differ.any()
    istar = oracle.qp_forward(*ins_np)["iters"]
    assert istar < MAX_ITER
    full = oracle.qp_forward(*ins_np, eps=0.0, notImprovedLim=10 ** 6, guard=True)
    hist = np.where(np.isnan(full["resid_hist"]), np.inf, full["resid_hist"])
    assert (hist.argmin(1) >= istar).any(), "nothing for the finish pass to do"
    ins = [dev(a, grad=False) for a in ins_np]
    out, dims, ws = c_forward(lib, ins, "batch")
    check_forward(out, o)
    gr = c_backward(lib, ins, dims, ws, out, ct)
    gm = np.maximum(o["lam"], o["slack"]).min(1) > 1e-5      # strict complementarity (tests/test_gpu_parity.py)
    assert gm.sum() >= B - 1
    for k in og:
        np.testing.assert_allclose(gr[k][gm], og[k][gm], err_msg=k, **GT)


def parent_arrays(lib):  # noqa: F811
    """What tests/golden/r16n_parent_b4.npz records (it was written from this function, on the build before the
    prefetch): family R, seed 0, B = 4, batch rule; backward at the kernels' own forward point."""
    B = 4
    got = {}
    ins = [dev(a, grad=False) for a in family_R(0, B, *METRIC)]
    out, dims, ws = c_forward(lib, ins, "batch")
    ct = np.random.default_rng(1).standard_normal((B, METRIC[0]))
    got.update(out)
    got.update(c_backward(lib, ins, dims, ws, out, ct))
    ins = [dev(a, grad=False) for a in family_R(0, B, *THREE_SLOT)]
    out, _, _ = c_forward(lib, ins, "batch")
    got.update({"f40_" + k: out[k] for k in FORWARD_KEYS})
    return got


def test_bit_identical_to_the_build_before(lib):  # noqa: F811
    want = np.load(PARENT, allow_pickle=False)
    got = parent_arrays(lib)
    assert sorted(want.files) == sorted(got) and len(got) == 16
    for k in want.files:
        assert want[k].dtype == got[k].dtype and np.array_equal(want[k], got[k]), k
