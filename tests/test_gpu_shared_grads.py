"""Gradients of shared parameters summed on the device (dqp_qp_backward_shared, csrc/dqp_shared_grad.hip).

Against the per-sample path through the C ABI: `want` = dqp_qp_backward's per-sample gradients summed by torch in
fp64.  Both are sums of the same B terms in different orders, so the bound is elementwise and comes from the
per-sample tensors, |got - want| <= 4 B 2^-53 sum_b |g_b|; there is no fixed rtol.  Outputs of parameters that are
not shared come from the same kernel in both calls and must be bit-identical.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GT = dict(rtol=1e-4, atol=1e-6)
U = 2.0 ** -53
NAMES = "QpGhAb"

PATTERNS = {
    "all": (1, 1, 1, 1, 1, 1),
    "QGA": (1, 0, 1, 0, 1, 0),
    "h": (0, 0, 0, 1, 0, 0),
    "A": (0, 0, 0, 0, 1, 0),
    "none": (0, 0, 0, 0, 0, 0),
}


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "these tests need a GPU"
    import diff_qp_mpc_amd
    from diff_qp_mpc_amd import _lib, qp as qpmod
    return diff_qp_mpc_amd, _lib, qpmod, _lib.load()


def make_inputs(seed, B, nz, nineq, neq, share):
    """Family R (random dense QP, Q = L L^T + 1e-3 I), all six batched, with the parameters marked in `share` equal
    over the batch (row 0 is the shared value); every problem is feasible: h >= G z0, b = A z0 at a point z0 (one
    point for the whole batch when b is shared)."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    L = rn(B, nz, nz)
    Q = L @ L.transpose(1, 2) + 1e-3 * torch.eye(nz, dtype=torch.float64)
    G, A, p, z0 = rn(B, nineq, nz), rn(B, neq, nz), rn(B, nz), rn(B, nz)
    s0 = torch.rand(B, nineq, generator=g, dtype=torch.float64)
    sQ, sp, sG, sh, sA, sb = share
    if sQ: Q = Q[:1].expand(B, nz, nz)
    if sp: p = p[:1].expand(B, nz)
    if sG: G = G[:1].expand(B, nineq, nz)
    if sA: A = A[:1].expand(B, neq, nz)
    if sb: z0 = z0[:1].expand(B, nz)
    Gz = (G @ z0.unsqueeze(-1)).squeeze(-1)
    h = (Gz.max(0).values + s0[0]).expand(B, nineq) if sh else Gz + s0
    b = (A @ z0.unsqueeze(-1)).squeeze(-1)
    return [t.contiguous().cuda() if t.numel() > 0 else torch.empty(0, dtype=torch.float64, device="cuda")
            for t in (Q, p, G, h, A, b)]


def c_backward(_lib, lib, saved, fwd, ct, flags, reduce, use_ctx, null=()):
    """One call of dqp_qp_backward (reduce=False) or dqp_qp_backward_shared -> six tensors (None where NULL)."""
    Q, G, A, dims, ctx_ws = saved
    zhat, lam, nu, slack = fwd
    B, nz, nineq, neq = dims.nbatch, dims.nz, dims.nineq, dims.neq
    strides = (dims.stride_Q, dims.stride_p, dims.stride_G, dims.stride_h, dims.stride_A, dims.stride_b)
    shapes = ((nz, nz), (nz,), (nineq, nz), (nineq,), (neq, nz), (neq,))
    outs = []
    for i, shp in enumerate(shapes):
        if i in null or (i >= 4 and neq == 0):
            outs.append(None)
            continue
        lead = () if (reduce and strides[i] == 0) else (B,)
        outs.append(torch.full(lead + shp, float("nan"), dtype=torch.float64, device="cuda"))
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() > 0 else ctypes.c_void_p(0)
    big = max(nz, nineq, neq) > _lib.DQP_MAX_DIM
    ws = ctx_ws if (use_ctx or big) else None
    opts = _lib.dqp_opts(0.0, 0.0, 0, 0, flags | (_lib.DQP_FLAG_BACKWARD_CTX if use_ctx else 0), 0)
    args = [ctypes.byref(dims), ctypes.byref(opts), P(Q), P(G), P(A), P(zhat), P(lam), P(nu), P(slack), P(ct)] + \
           [P(o) for o in outs] + [None, P(ws)]
    if reduce:
        rb = int(lib.dqp_qp_backward_shared_bytes(ctypes.byref(dims)))
        assert (rb > 0) == any(st == 0 for st, shp in zip(strides, shapes) if shp[0] > 0)
        rws = torch.full((rb // 8,), float("nan"), dtype=torch.float64, device="cuda") if rb else None
        rc = lib.dqp_qp_backward_shared(*args, P(rws), None)
    else:
        rc = lib.dqp_qp_backward(*args, None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return outs, strides


def check_against_per_sample(env, shape, B, pattern, force=0, flags=0, null=(), seed=0, report=None):
    _, _lib, qpmod, lib = env
    nz, nineq, neq = shape
    share = PATTERNS[pattern]
    ins = make_inputs(1000 * seed + 7 * B + nz, B, nz, nineq, neq, share)
    old = qpmod.FORCE_FLAGS
    qpmod.FORCE_FLAGS = force
    try:
        zhat, lam, nu, slack, info, resid, saved = qpmod._forward_impl(*ins, 1e-12, 20, 3)
    finally:
        qpmod.FORCE_FLAGS = old
    assert int(info[:, 0].abs().max()) == 0
    # the same problems with the shared parameters passed once: stride 0 (the forward's context is per problem)
    Q, G, A, dims, ctx_ws = saved
    st = [0 if (s or t.numel() == 0) else t[0].numel() for s, t in zip(share, ins)]
    Q, G, A = [t[0].contiguous() if (s and t.numel() > 0) else t for s, t in zip((share[0], share[2], share[4]), (Q, G, A))]
    saved = (Q, G, A, _lib.dqp_dims(B, nz, nineq, neq, *st), ctx_ws)
    fwd = (zhat, lam, nu, slack)
    ct = torch.randn(B, nz, dtype=torch.float64, generator=torch.Generator().manual_seed(B + 1)).cuda()
    for use_ctx in (True, False):
        per, strides = c_backward(_lib, lib, saved, fwd, ct, flags | force, False, use_ctx, null)
        got, _ = c_backward(_lib, lib, saved, fwd, ct, flags | force, True, use_ctx, null)
        again, _ = c_backward(_lib, lib, saved, fwd, ct, flags | force, True, use_ctx, null)
        for i, (g, g2, ps) in enumerate(zip(got, again, per)):
            if ps is None:
                assert g is None
                continue
            assert not torch.isnan(ps).any()
            if strides[i] != 0:                                   # per-sample output: the same kernel wrote it
                assert torch.equal(g, ps), "d%s differs from dqp_qp_backward (%s, ctx=%s)" % (NAMES[i], pattern, use_ctx)
                continue
            assert g.shape == ps.shape[1:]
            assert torch.equal(g, g2), "d%s is not reproducible" % NAMES[i]
            want = ps.sum(0)
            bound = 4.0 * B * U * ps.abs().sum(0)
            err = (g - want).abs()
            ratio = float((err / bound.clamp_min(1e-300)).max())
            print("shape %s B %d pattern %s ctx %d d%s: max |got - want| / bound = %.3g" %
                  (shape, B, pattern, use_ctx, NAMES[i], ratio))
            if report is not None:
                report.append(ratio)
            assert bool((err <= bound).all()), "d%s: %g of the bound (%s, B=%d, ctx=%s)" % (NAMES[i], ratio, pattern, B, use_ctx)


def kc(_lib):
    return _lib.SHARED_GRAD_KC


def small_shapes():
    from diff_qp_mpc_amd import _build, _lib
    r16 = [s for s in _build.R16_SIZES if s[2] == 0][0]
    assert (30, 30, 15) in _build.R16N_SIZES
    G = _lib.DQP_FLAG_GENERIC_ONLY
    return [((30, 30, 15), 0), (r16, 0), ((50, 37, 11), 0), ((30, 30, 15), G)]


def batch_sizes():
    from diff_qp_mpc_amd import _lib
    K = _lib.SHARED_GRAD_KC
    return [1, 3, K - 1, K + 1, 2 * K + 5]


@pytest.mark.parametrize("B", batch_sizes())
@pytest.mark.parametrize("shape,force", small_shapes())
def test_sum_matches_per_sample_path(env, shape, force, B):
    """One shape per kernel family (null-space DPP rows, DPP rows without equalities, generic, generic forced at the
    metric size), batch sizes around the split-K chunk, every sharing pattern, with and without the forward's context."""
    for pattern in PATTERNS:
        check_against_per_sample(env, shape, B, pattern, force=force)


def test_blocked_kernels(env):
    for pattern in PATTERNS:
        check_against_per_sample(env, (70, 65, 3), 5, pattern)


def test_dense_backward_flag(env):
    _, _lib, _, _ = env
    check_against_per_sample(env, (30, 30, 15), kc(_lib) + 1, "all", flags=_lib.DQP_FLAG_DENSE_BACKWARD)


def test_half_of_the_gradient_pointers_null(env):
    _, _lib, _, _ = env
    check_against_per_sample(env, (30, 30, 15), kc(_lib) + 1, "all", null=(1, 2, 5))
    check_against_per_sample(env, (30, 30, 15), 3, "QGA", null=(0, 3, 4))


def load(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False))


def dev(a, grad=True):
    t = torch.tensor(np.asarray(a), dtype=torch.float64, device="cuda")
    return t.requires_grad_() if grad else t


@pytest.mark.parametrize("name", ["R_shared_QGA_b6", "R_shared_all_but_b_b4"])
def test_qpfunction_vs_reference_golden(env, name):
    """QPFunction with shared parameters against the reference's recorded gradients, with the device reduction and
    with the per-sample + .mean(0) path; the two agree within the summation bound (divided by B: they are means)."""
    dqp, _lib, qpmod, _ = env
    g = load(name)
    B = g["zhat"].shape[0]
    res = {}
    assert qpmod.REDUCE_SHARED_GRADS is True
    try:
        for switch in (True, False):
            qpmod.REDUCE_SHARED_GRADS = switch
            for tag in ("ones", "rand"):
                ins = [dev(g["in_" + k]) for k in NAMES]
                zhat = dqp.QPFunction(check_Q_spd=True, verbose=-1)(*ins)
                zhat.backward(dev(g["ct_" + tag], grad=False))
                for k, t in zip(NAMES, ins):
                    assert t.grad.shape == g["d%s_%s" % (k, tag)].shape
                    np.testing.assert_allclose(t.grad.cpu().numpy(), g["d%s_%s" % (k, tag)],
                                               err_msg="d%s (%s, reduce=%s)" % (k, tag, switch), **GT)
                res[switch, tag] = [t.grad.clone() for t in ins]
    finally:
        qpmod.REDUCE_SHARED_GRADS = True
    for tag in ("ones", "rand"):
        ins = [dev(g["in_" + k], grad=False) for k in NAMES]
        zhat, lam, nu, slack, _, _, saved = qpmod._forward_impl(*ins, 1e-12, 20, 3)
        per = qpmod._backward_impl(saved, zhat, lam, nu, slack, dev(g["ct_" + tag], grad=False), (True,) * 6, 0)
        for i, k in enumerate(NAMES):
            on, off = res[True, tag][i], res[False, tag][i]
            if g["in_" + k].ndim == (3, 2, 3, 2, 3, 2)[i]:
                assert torch.equal(on, off), "per-sample d%s" % k
                continue
            bound = 4.0 * B * U * per[i].abs().sum(0) / B
            assert bool(((on - off).abs() <= bound).all()), "d%s (%s)" % (k, tag)


def test_no_per_sample_temporaries(env):
    """Backward with Q, G, A shared allocates less than ONE per-sample dQ (B nz nz doubles); the per-sample path
    (switch off) allocates at least that."""
    dqp, _lib, qpmod, _ = env
    B, nz, nineq, neq = 512, 30, 30, 15
    growth = {}
    try:
        for switch in (True, False):
            qpmod.REDUCE_SHARED_GRADS = switch
            share = PATTERNS["QGA"]
            ins = [(t[0].contiguous() if s else t).requires_grad_()
                   for t, s in zip(make_inputs(5, B, nz, nineq, neq, share), share)]
            zhat = dqp.QPFunction(check_Q_spd=False, verbose=-1)(*ins)
            ct = torch.ones_like(zhat)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            zhat.backward(ct)
            torch.cuda.synchronize()
            growth[switch] = torch.cuda.max_memory_allocated() - base
            assert ins[0].grad.shape == (nz, nz) and ins[2].grad.shape == (nineq, nz) and ins[4].grad.shape == (neq, nz)
            del ins, zhat, ct
    finally:
        qpmod.REDUCE_SHARED_GRADS = True
    print("peak growth in backward: reduced %d B, per-sample %d B" % (growth[True], growth[False]))
    assert growth[True] < B * nz * nz * 8, growth
    assert growth[False] >= B * nz * nz * 8, growth
