"""Guard-band tests (tests/guardband.py): an entry point reads and writes only inside the extents its arguments declare,
and its results do not depend on a single byte outside them (include/dqp.h, "Extents").

Every case runs the package's own Python layer -- which allocates outputs and workspaces as it does in production,
the workspaces by the `*_bytes` functions of include/dqp.h -- three times under guardband.run_guarded: inputs, outputs
and workspaces sit between guard bands filled with NaN words, NaN words again, then zeros; every guard must be intact
after every run and the outputs of the three runs bit-identical.  The shapes are the smallest at which each kernel
family can still go wrong, the batch never a multiple of the problems a wavefront packs (2, 4 or 8), so idle lanes
exist in every launch.

Values: the outputs of the first run against the reference and at the tolerances of the path's own test --
  dense QPs            oracle.qp_forward / qp_backward, ZT / DT / GT of test_gpu_parity.py
  shared-parameter sums  the oracle's per-sample gradients summed over the batch, GT
  DEQ stages           torch fp64 under the 4x rule of test_gpu_deq_layer.py
  stage-wise MPC QPs   oracle.dense_forward / dense_backward on the numpy-assembled QP (test_gpu_mpc_bounds.py), ZT / DT / GT;
                       the device SQP round against the Python round (test_gpu_mpc_sqp.py, rtol 1e-5 / atol 1e-7)
  NewtonAL / AL_mpc    oracle/al_solve_oracle.py, over the extended rows of tests/al_xbounds_oracle.py with a state box, at
                       test_gpu_al_xbounds.py's mpc_tol; the caller-linearised step against the dense numpy oracle of
                       test_gpu_al_given.py (rtol 1e-8 / atol 1e-10)
  dynamics registry    the recorded outputs of tests/golden/DYN_*.npz at test_gpu_dyn.py's tolerances (states 1e-12,
                       Jacobians 1e-11); the integrator against its closed form (test_gpu_integrator.py)
No convergence masks: the seeds are such that the oracle alone reaches best_resid < 1e-8 on every sample with strict
complementarity (asserted).  Each case also asserts that the workspace it is about really was intercepted: the list of
intercepted allocation sizes contains exactly what the size function returns for the case's dims.  That is a
membership test on byte counts: where the test allocates the buffer itself it only says the test used that value, and
in the Python-layer cases another allocation of equal size could satisfy it; the guard behind the buffer's last byte
is what holds the kernels to the size.

The Python layer of AL_mpc builds some kernel arguments with torch arithmetic that no patch intercepts (the in/out
iterate, the penalty, later multipliers, the contiguous cost diagonal: DESIGN.md 5.1); the AL entry points are
therefore also called through the C ABI with every array guarded.

A guard of finite size shows nothing about stores farther than eight leading-dimension strides away (guardband.py).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import guardband as gb
from families import family
from oracle import oracle

pytestmark = pytest.mark.gpu

ZT = dict(rtol=1e-6, atol=1e-8)
DT = dict(rtol=1e-5, atol=1e-7)
GT = dict(rtol=1e-4, atol=1e-6)
NAMES = "QpGhAb"


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "these tests need a GPU"
    from diff_qp_mpc_amd import _lib, qp as qpmod
    return _lib, qpmod, _lib.load()


def nonzero_finite(a):
    a = np.asarray(a)
    return a.size > 0 and np.isfinite(a).all() and np.abs(a).max() > 0


def np_(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------------------------------ dense QPs
def dense_dims(_lib, B, nz, nineq, neq, shared=(0,) * 6):
    st = [nz * nz, nz, nineq * nz, nineq, neq * nz, neq]
    return _lib.dqp_dims(B, nz, nineq, neq, *[0 if s else v for s, v in zip(shared, st)])


@functools.lru_cache(maxsize=None)
def dense_problem(nz, nineq, neq, B, seed):
    """family R + the oracle's forward and backward, computed once per case and shared by its parametrisations"""
    ins = family(seed, B, nz, nineq, neq, "R")
    o = oracle.qp_forward(*ins)
    ct = np.random.default_rng(seed + 1).standard_normal((B, nz))
    og = oracle.qp_backward(ins[0], ins[2], ins[4], o["zhat"], o["lam"], o["nu"], o["slack"], ct)
    # no masks below: the oracle converges on every sample, with strict complementarity
    assert (o["best_resid"] < 1e-8).all(), o["best_resid"]
    assert np.maximum(o["lam"], o["slack"]).min() > 1e-5
    return ins, o, ct, og


def put_qp(put, ins, ct):
    """six guarded inputs (an empty A / b stays an ordinary empty tensor: the entry takes NULL) + the cotangent"""
    t = [put(a, NAMES[i]) if a.size else torch.zeros(a.shape, dtype=torch.float64, device="cuda")
         for i, a in enumerate(ins)]
    return t + [put(ct, "dl_dzhat")]


def check_forward(out, o, neq):
    zhat, lam, nu, slack, info, resid = [np_(t) for t in out[:6]]
    assert (info[:, 0] == 0).all()
    np.testing.assert_allclose(zhat, o["zhat"], **ZT)
    np.testing.assert_allclose(lam, o["lam"], **DT)
    np.testing.assert_allclose(slack, o["slack"], **DT)
    if neq:
        np.testing.assert_allclose(nu, o["nu"], **DT)
    assert resid.max() < 1e-8
    assert nonzero_finite(zhat) and nonzero_finite(lam)


def check_grads(grads, og, neq, what=""):
    for k, t in zip(NAMES, grads):
        if neq == 0 and k in "Ab":
            assert t is None
            continue
        np.testing.assert_allclose(np_(t), og["d" + k], err_msg="d%s %s" % (k, what), **GT)
    assert nonzero_finite(np_(grads[0]))


def run_dense(env, shape, B, seed, termination, force):
    """forward + backward through qp._forward_impl / _backward_impl under guards -> (outputs, intercepted sizes)"""
    _lib, qpmod, lib = env
    nz, nineq, neq = shape
    ins, o, ct, og = dense_problem(nz, nineq, neq, B, seed)

    def fn(t):
        old = qpmod.FORCE_FLAGS
        qpmod.FORCE_FLAGS = force
        try:
            fwd = qpmod._forward_impl(*t[:6], 1e-12, 20, 3, termination=termination)
            grads = qpmod._backward_impl(fwd[6], *fwd[:4], t[6], (True,) * 6, qpmod.FORCE_FLAGS)
        finally:
            qpmod.FORCE_FLAGS = old
        return fwd[:6] + tuple(grads)

    out, sizes = gb.run_guarded(fn, lambda put: put_qp(put, ins, ct))
    check_forward(out, o, neq)
    check_grads(out[6:], og, neq)
    # the workspaces were intercepted at exactly the sizes include/dqp.h reports
    dims = dense_dims(_lib, B, nz, nineq, neq)
    opts = _lib.dqp_opts(1e-12, qpmod.STALL_TOL, 20, 3, force | (_lib.DQP_FLAG_BATCH_TERMINATION if termination == "batch" else 0), 0)
    wsb = int(lib.dqp_workspace_bytes(ctypes.byref(dims)))
    tb = int(lib.dqp_termination_bytes(ctypes.byref(dims), ctypes.byref(opts)))
    assert (tb > 0) == (termination == "batch") and tb % 8 == 0
    if wsb:
        assert wsb in sizes, (wsb, sizes)
    if tb:
        assert tb in sizes, (tb, sizes)
    assert B * nz * 8 in sizes and B * nz * nz * 8 in sizes          # zhat, dQ
    return out, sizes, wsb


# (nz, nineq, neq), B, seed.  DPP rows: 4 QPs per wavefront (10, 5, 3), (12, 8, 0), (20, 10, 15); the three-slot
# null-space kernel (40, 20, 30)
DPP = [((10, 5, 3), 1, 0), ((10, 5, 3), 3, 0), ((10, 5, 3), 5, 0), ((12, 8, 0), 5, 0), ((20, 10, 15), 5, 0),
       ((40, 20, 30), 2, 0)]
FAMILIES = {"auto": 0, "rows": 4, "generic": 2}      # DQP_FLAG_NO_NULLSPACE, DQP_FLAG_GENERIC_ONLY (asserted below)


def dpp_cases():
    """every DPP shape under the families of test_gpu_parity.py that are a different kernel there: "rows" (the forward
    that keeps the equality rows) exists next to "auto" only where the size has both instantiations"""
    from diff_qp_mpc_amd import _build
    out = []
    for shape, B, seed in DPP:
        for fam in ("auto", "rows", "generic"):
            if fam == "rows" and not (shape in _build.R16_SIZES and shape in _build.R16N_SIZES):
                continue
            out.append(pytest.param(shape, B, seed, fam, id="%d-%d-%d-B%d-%s" % (shape + (B, fam))))
    return out


@pytest.mark.parametrize("termination", ["batch", "per_problem"])
@pytest.mark.parametrize("shape,B,seed,fam", dpp_cases())
def test_dense_dpp_rows(env, shape, B, seed, fam, termination):
    """The size-specialised kernels at their own sizes: automatic dispatch (null-space forward + context backward where
    the size has equalities), the forward that keeps the equality rows, and the generic kernels at the same sizes."""
    _lib, qpmod, lib = env
    assert FAMILIES == {"auto": 0, "rows": _lib.DQP_FLAG_NO_NULLSPACE, "generic": _lib.DQP_FLAG_GENERIC_ONLY}
    from diff_qp_mpc_amd import _build
    out, sizes, wsb = run_dense(env, shape, B, seed, termination, FAMILIES[fam])
    assert (wsb > 0) == (shape in _build.R16N_SIZES)               # the null-space sizes have a workspace


# one shape per width of the generic one-QP-per-wavefront kernels (8, 16, 32, 64 lanes' worth of rows)
GENERIC = [((7, 9, 2), 3, 0), ((17, 7, 3), 3, 0), ((33, 20, 10), 3, 0), ((64, 64, 32), 3, 0)]


@pytest.mark.parametrize("termination", ["batch", "per_problem"])
@pytest.mark.parametrize("shape,B,seed", GENERIC)
def test_dense_generic(env, shape, B, seed, termination):
    _lib, qpmod, lib = env
    run_dense(env, shape, B, seed, termination, _lib.DQP_FLAG_GENERIC_ONLY)


BLOCKED = [((65, 65, 0), 2, 0), ((70, 40, 30), 2, 0), ((64, 100, 0), 2, 0)]


@pytest.mark.parametrize("termination", ["batch", "per_problem"])
@pytest.mark.parametrize("shape,B,seed", BLOCKED)
def test_dense_blocked(env, shape, B, seed, termination):
    """One QP per workgroup, matrices in the workspace (csrc/dqp_big.hip): forward, backward from the forward's context,
    and dqp_qp_backward without DQP_FLAG_BACKWARD_CTX, which rebuilds the factorisations in a workspace of its own."""
    _lib, qpmod, lib = env
    nz, nineq, neq = shape
    out, sizes, wsb = run_dense(env, shape, B, seed, termination, 0)
    assert wsb > 0
    ins, o, ct, og = dense_problem(nz, nineq, neq, B, seed)
    dims = dense_dims(_lib, B, nz, nineq, neq)

    def fn(t):
        Q, p, G, h, A, b, g = t[:7]
        point = t[7:]
        kw = dict(dtype=torch.float64, device="cuda")
        ws = torch.empty(wsb // 8, **kw)
        outs = [torch.empty(B, nz, nz, **kw), torch.empty(B, nz, **kw), torch.empty(B, nineq, nz, **kw),
                torch.empty(B, nineq, **kw)]
        outs += [torch.empty(B, neq, nz, **kw), torch.empty(B, neq, **kw)] if neq else [None, None]
        opts = _lib.dqp_opts(0.0, 0.0, 0, 0, 0, 0)
        _lib.call("dqp_qp_backward", Q.device, dims, opts, Q, G, A, *point, g, *outs, None, ws)
        return tuple(outs)

    def make(put):
        return put_qp(put, ins, ct) + [put(o[k], k) if o[k].size else torch.zeros(o[k].shape, dtype=torch.float64, device="cuda")
                                       for k in ("zhat", "lam", "nu", "slack")]

    grads, sizes = gb.run_guarded(fn, make)
    check_grads(grads, og, neq, "(rebuilt)")
    assert wsb in sizes, (wsb, sizes)


# ------------------------------------------------------------------------------------------ shared-parameter sums
def shared_problem(nz, nineq, neq, B, seed):
    """pattern "all": one Q, p, G, h, A, b for the whole batch (family R, sample 0), the batch differing in nothing but
    the cotangent -- so every per-sample gradient is computed from the same forward point"""
    ins, o, _, _ = dense_problem(nz, nineq, neq, 1, seed)
    ct = np.random.default_rng(seed + 2).standard_normal((B, nz))
    rep = lambda a: np.repeat(a, B, 0)
    og = oracle.qp_backward(rep(ins[0]), rep(ins[2]), rep(ins[4]), rep(o["zhat"]), rep(o["lam"]), rep(o["nu"]),
                            rep(o["slack"]), ct)
    return [a[0] for a in ins], {k: rep(o[k]) for k in ("zhat", "lam", "nu", "slack")}, ct, og


def shared_cases():
    from diff_qp_mpc_amd import _lib
    return [((10, 5, 3), 3, 0), ((10, 5, 3), _lib.SHARED_GRAD_KC + 1, 0), ((70, 65, 3), 3, 0)]


@pytest.mark.parametrize("shape,B,seed", shared_cases())
def test_dense_shared_parameter_sums(env, shape, B, seed):
    """dqp_qp_backward_shared through qp._backward_impl(shared=...), pattern "all" of test_gpu_shared_grads.py: every
    parameter passed once (stride 0), its gradient ONE tensor, the sum over the batch (split-K over chunks of
    SHARED_GRAD_KC samples: B = 3 is one ragged chunk, KC + 1 a full chunk and one sample).  The forward runs on the
    batched copies, as there: its context is per problem."""
    _lib, qpmod, lib = env
    nz, nineq, neq = shape
    ins, o, ct, og = shared_problem(nz, nineq, neq, B, seed)
    dims0 = dense_dims(_lib, B, nz, nineq, neq, shared=(1,) * 6)

    def fn(t):
        fwd = qpmod._forward_impl(*t[:6], 1e-12, 20, 3, termination="per_problem")
        Q, G, A, dims, ctx_ws = fwd[6]
        assert ctx_ws is not None
        grads = qpmod._backward_impl((t[7], t[8], t[9], dims0, ctx_ws), *fwd[:4], t[6], (True,) * 6, 0, shared=(True,) * 6)
        return fwd[:6] + tuple(grads)

    def make(put):
        batched = [np.ascontiguousarray(np.broadcast_to(a, (B,) + a.shape)) for a in ins]
        return put_qp(put, batched, ct) + [put(ins[i], NAMES[i] + " (shared)") for i in (0, 2, 4)]

    out, sizes = gb.run_guarded(fn, make)
    check_forward(out, o, neq)
    for k, t in zip(NAMES, out[6:]):
        assert t.shape == og["d" + k].shape[1:]
        np.testing.assert_allclose(np_(t), og["d" + k].sum(0), err_msg="d" + k, **GT)
    assert nonzero_finite(np_(out[6]))
    rb = int(lib.dqp_qp_backward_shared_bytes(ctypes.byref(dims0)))
    assert rb > 0 and rb in sizes, (rb, sizes)
    wsb = int(lib.dqp_workspace_bytes(ctypes.byref(dense_dims(_lib, B, nz, nineq, neq))))
    assert wsb > 0 and wsb in sizes


# ------------------------------------------------------------------------------------------ DEQ stages (fp32)
def _leaves(ts):
    return [t.requires_grad_() for t in ts]          # the guarded tensors themselves are the autograd leaves


@pytest.mark.parametrize("h,nrows", [(32, 1), (32, 3), (512, 3)])
def test_deq_stages(env, h, nrows):
    """Both fused DEQLayer stages, forward and backward, through deq_fused (fp32; hdim 32 packs two rows into a
    wavefront, so 1 and 3 rows leave half a wavefront idle) under the 4x rule of test_gpu_deq_layer.py."""
    _lib, _, lib = env
    import test_gpu_deq_layer as deq
    from diff_qp_mpc_amd import deq_fused
    d = _lib.dqp_deq_dims(nrows, h)
    part = int(lib.dqp_deq_partial_bytes(ctypes.byref(d)))
    assert part > 0
    for relu in (0, 1):
        a, gamma, beta, dy = deq._stage_a_inputs(h, nrows)

        def fn_a(t):
            a_, g_, b_ = _leaves(t[:3])
            y = deq_fused.LayerNormStage.apply(a_, g_, b_, deq.EPS, relu)
            y.backward(t[3])
            return {"y": y.detach(), "da": a_.grad, "dgamma": g_.grad, "dbeta": b_.grad}

        fused, sizes = gb.run_guarded(fn_a, lambda put: [put(t.cpu(), n) for t, n in zip((a, gamma, beta, dy), ("a", "gamma", "beta", "dy"))])
        deq._check("guarded A h%d n%d relu%d" % (h, nrows, relu), fused, deq._stage_a_torch(a, gamma, beta, dy, relu, torch.float32),
                   deq._stage_a_torch(a, gamma, beta, dy, relu, torch.float64))
        assert part in sizes and nrows * 2 * 4 in sizes and nrows * h * 4 in sizes, (part, sizes)     # partials, stats, y
        assert nonzero_finite(np_(fused["y"])) and nonzero_finite(np_(fused["dgamma"]))
    ins = deq._stage_b_inputs(h, nrows)
    names = ("xi", "a2", "z1", "gamma2", "beta2", "gamma3", "beta3", "dz2")

    def fn_b(t):
        lv = _leaves(t[:7])
        z2 = deq_fused.ResidualStage.apply(*lv, deq.EPS, deq.EPS)
        z2.backward(t[7])
        return dict(zip(("z2", "dxi", "da2", "dz1", "dgamma2", "dbeta2", "dgamma3", "dbeta3"),
                        [z2.detach()] + [v.grad for v in lv]))

    fused, sizes = gb.run_guarded(fn_b, lambda put: [put(t.cpu(), n) for t, n in zip(ins, names)])
    deq._check("guarded B h%d n%d" % (h, nrows), fused, deq._stage_b_torch(*ins, torch.float32), deq._stage_b_torch(*ins, torch.float64))
    assert part in sizes and nrows * 4 * 4 in sizes, (part, sizes)
    assert nonzero_finite(np_(fused["z2"])) and nonzero_finite(np_(fused["dgamma3"]))


# ------------------------------------------------------------------------------------------ dynamics registry
def dyn_models():
    from diff_qp_mpc_amd import dynamics
    return list(dynamics.ALL_NAMES)


@pytest.mark.parametrize("N", [1, 65])
@pytest.mark.parametrize("name", dyn_models())
def test_dynamics_registry(env, name, N):
    """dqp_dyn_step / dqp_dyn_jacobian of every registered model through DeviceDynamics at one point and at 65 (one more
    than a wavefront): the states of tests/golden/DYN_*.npz (the first, or all 48 and the first 17 again) against their
    recorded outputs at test_gpu_dyn.py's tolerances; the integrator, which has no such file, against its closed form
    at the same ones (test_gpu_integrator.py)."""
    import os
    from diff_qp_mpc_amd.dynamics import DeviceDynamics
    if name == "integrator":
        from test_gpu_integrator import step_np
        rng = np.random.default_rng(N)
        dt = 0.1
        x, u = rng.standard_normal((N, 2)), rng.standard_normal((N, 1))
        want = dict(x_next=step_np(x, u, dt), Jx=np.broadcast_to([[1.0, dt], [0.0, 1.0]], (N, 2, 2)),
                    Ju=np.broadcast_to([[dt * dt], [dt]], (N, 2, 1)))
    else:
        g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "DYN_%s.npz" % name))
        idx = np.arange(N) % g["x"].shape[0]
        dt = float(g["dt"])
        x, u = g["x"][idx], g["u"][idx]
        want = {k: g[k][idx] for k in ("x_next", "Jx", "Ju")}
    dyn = DeviceDynamics(name, dt=dt)
    n, m = dyn.n_state, dyn.n_ctrl

    def fn(t):
        with torch.no_grad():
            step = dyn(*t)
        xn, (Jx, Ju) = dyn.jac(*t)
        return step, xn, Jx, Ju

    (step, xn, Jx, Ju), sizes = gb.run_guarded(fn, lambda put: [put(x, "x"), put(u, "u")])
    np.testing.assert_allclose(np_(step), want["x_next"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(np_(xn), want["x_next"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(np_(Jx), want["Jx"], rtol=0, atol=1e-11)
    np.testing.assert_allclose(np_(Ju), want["Ju"], rtol=0, atol=1e-11)
    assert sizes.count(N * n * 8) >= 2 and N * n * m * 8 in sizes and N * n * n * 8 in sizes      # the outputs were guarded
    assert np.isfinite(np_(xn)).all() and nonzero_finite(np_(Jx))      # (the first recorded state of a model may be its rest state)


# ------------------------------------------------------------------------------------------ stage-wise MPC QPs
@functools.lru_cache(maxsize=None)
def stage_problem(n, m, T, B, seed):
    """test_gpu_mpc_bounds.py's problem, (T, B, m) bounds and numpy assembly + oracle.dense_forward / dense_backward,
    once per case.  dense_forward reports no residual, so its convergence is asserted on its solution: the KKT
    residual of the assembled QP below 1e-8, strict complementarity, and bounds both active and inactive."""
    import test_gpu_mpc_bounds as mb
    data = mb.problem(n, m, T, B, seed=seed)
    lo, hi, strides, lo_f, hi_f = mb.bounds("time_major", m, T, B, seed=seed + 1)
    w = mb.weights(B, T, n + m)
    Q, p, G, h, A, b = mb.assemble(*data, lo_f, hi_f)
    o = oracle.dense_forward(Q, p, G, h, A, b)
    z, lam, nu, s = o["zhat"], o["lam"], o["nu"], o["slack"]
    mv = lambda M, x: np.einsum("bij,bj->bi", M, x)
    mtv = lambda M, x: np.einsum("bji,bj->bi", M, x)
    kkt = max(np.abs(mv(Q, z) + p + mtv(G, lam) + mtv(A, nu)).max(), np.abs(mv(A, z) - b).max(),
              np.abs(mv(G, z) + s - h).max(), np.abs(lam * s).max())
    assert kkt < 1e-8, kkt
    assert np.maximum(lam, s).min() > 1e-5
    assert s.min() < 1e-6 and s.max() > 0.02                        # some bounds active, some not
    want = mb.oracle_solve(("guardband", n, m, T, B, seed), data, lo_f, hi_f, w)
    return data, lo, hi, strides, w, want


# n, m, T, B, seed, variant: "lds" / "global" -- the LDS-resident kernels and DQP_FLAG_RIC_GLOBAL_WS, as
# test_stagewise_lds_resident_equals_global_workspace selects them; "wide": two problems per wavefront; "padded": the
# kernels of a larger host pair
STAGE = [(2, 1, 2, 3, 0, "lds"), (3, 1, 4, 5, 0, "lds"), (3, 1, 4, 5, 0, "global"), (12, 4, 3, 5, 0, "lds"),
         (13, 4, 3, 3, 0, "wide"), (5, 3, 3, 5, 0, "padded"), (17, 3, 3, 3, 0, "padded")]


@pytest.mark.parametrize("stepped", [False, True], ids=["fused", "stepped"])
@pytest.mark.parametrize("termination", ["batch", "per_problem"])
@pytest.mark.parametrize("n,m,T,B,seed,variant", STAGE)
def test_stagewise_mpc_qp(env, n, m, T, B, seed, variant, termination, stepped):
    """dqp_mpc_qp_forward_bounds / dqp_mpc_qp_forward_stepped_bounds + dqp_mpc_qp_backward on the stage-wise kernels,
    per-sample per-knot control bounds, both stop rules; outputs, workspace and termination buffer allocated at
    exactly the reported sizes."""
    import test_gpu_mpc_bounds as mb
    _lib, _, lib = env
    data, lo, hi, strides, w, want = stage_problem(n, m, T, B, seed)
    nt = n + m
    flags = _lib.DQP_FLAG_STAGEWISE | (_lib.DQP_FLAG_RIC_GLOBAL_WS if variant == "global" else 0)
    host = 0
    if variant == "padded":
        host = int(lib.dqp_mpc_qp_host_n_state(ctypes.byref(_lib.dqp_mpc_dims(B, n, m, T, 1, 0))))
        assert host > n
    dims = _lib.dqp_mpc_dims(B, n, m, T, 1, 0, host)
    opts = _lib.dqp_opts(1e-12, 1e-10, 20, 3, flags | (_lib.DQP_FLAG_BATCH_TERMINATION if termination == "batch" else 0), 0)
    r = lambda s: ctypes.byref(s)
    if stepped:
        wsb, tb = int(lib.dqp_mpc_qp_stepped_workspace_bytes(r(dims))), int(lib.dqp_mpc_qp_stepped_termination_bytes(r(dims), r(opts)))
    else:
        wsb, tb = int(lib.dqp_mpc_qp_workspace_bytes(r(dims))), int(lib.dqp_mpc_qp_termination_bytes(r(dims), r(opts)))
    assert wsb > 0 and wsb % 8 == 0 and tb % 8 == 0
    kernels = []

    def fn(t):
        C, c, F, f, x0, lo_d, hi_d, w_d = t
        kw = dict(dtype=torch.float64, device="cuda")
        o = [torch.empty(B, T, nt, **kw), torch.empty(B, 2 * T * m, **kw), torch.empty(B, T * n, **kw),
             torch.empty(B, 2 * T * m, **kw), torch.empty(B, 2, dtype=torch.int32, device="cuda"), torch.empty(B, **kw)]
        ws = torch.empty(wsb // 8, **kw)
        term = torch.empty(tb // 8, **kw) if tb else None
        bd = _lib.dqp_al_bounds(lo_d.data_ptr(), hi_d.data_ptr(), *strides)
        with _lib.trace(512) as tr:
            if not stepped:
                _lib.call("dqp_mpc_qp_forward_bounds", C.device, dims, opts, C, c, F, f, x0, bd, *o, ws, term)
            else:
                call = lambda ry, a, b: _lib.call("dqp_mpc_qp_forward_stepped_bounds", C.device, dims, opts, C, c, F, f, x0, bd,
                                                  ry, a, b, *o, ws, term)
                call(None, 0, 0)
                for it in range(20):          # the linear residual of the current iterate, as test_gpu_mpc_bounds.py computes it
                    tau = o[0]
                    pred = torch.matmul(F.transpose(0, 1), tau[:, :-1, :, None])[..., 0] + f.transpose(0, 1)
                    ry = torch.cat(((pred - tau[:, 1:, :n]).reshape(B, -1), tau[:, 0, :n] - x0), 1).contiguous()
                    call(ry, it, it + 1)
            g = [torch.empty(a.shape, **kw) for a in (C, c, F, f, x0)]
            bo = _lib.dqp_opts(0.0, 0.0, 0, 0, _lib.DQP_FLAG_DENSE_BACKWARD | _lib.DQP_FLAG_STAGEWISE, 0)
            _lib.call("dqp_mpc_qp_backward", C.device, dims, bo, C, F, *o[:4], w_d, *g, None, ws)
        kernels.append([k for k, _ in tr.records])
        return dict(zip(("tau", "lam", "nu", "slack", "info", "resid") + mb.GRADS, o + g))

    names = ("C", "c", "F", "f", "x0", "lower", "upper", "dl_dtau")
    out, sizes = gb.run_guarded(fn, lambda put: [put(a, k) for a, k in zip(data + (lo, hi, w), names)])
    mb._check({k: np_(v) for k, v in out.items()}, want, B)
    assert nonzero_finite(np_(out["tau"])) and nonzero_finite(np_(out["dC"]))
    assert wsb in sizes and (tb == 0 or tb in sizes), (wsb, tb, sizes)
    fwd = mb._strided_kernels(kernels[0])                            # the strided-bounds instantiations ran, of this pair
    assert fwd and any("Cfg<%d, %d" % (host if host else n, m) in k for k in fwd), kernels[0]
    if (n, m) == (3, 1) and not stepped:
        assert any("Cfg<3, 1, true>" in k for k in fwd) == (variant == "lds"), fwd


# ------------------------------------------------------------------------------------------ NewtonAL / AL_mpc
@functools.lru_cache(maxsize=None)
def al_case(robot, T, B, box):
    """test_gpu_al_xbounds.py's AL_mpc.MPC problem (a per-sample / per-knot control box; box == "state": its per-sample
    / per-knot state box too) and the numpy oracle's cold and warm call (oracle/al_solve_oracle.py, over the extended
    rows of tests/al_xbounds_oracle.py with the state box) + the oracle's backward of sum(x) + 2 sum(u), once per case"""
    import test_gpu_al_xbounds as xb
    from oracle import al_solve_oracle as aso
    n, m = xb.SIZES[robot]
    p = xb.mpc_problem(robot, T, B)
    xl, xh = (p["xl"], p["xh"]) if box == "state" else (None, None)
    o1, o2 = xb.oracle_two_calls(robot, T, B, p, xl, xh)
    assert not o1["chol_fail"] and not o2["chol_fail"]
    if box == "state":
        assert (o1["lam"][:, T * n + 2 * T * m:] > 0).any()           # the state box is active
    g = np.concatenate((np.ones((B, T, n)), 2.0 * np.ones((B, T, m))), 2)
    dQ, dq = aso.backward(o1["L"], o1["xu"], g)
    return p, xl, xh, o1, o2, dQ, dq


def run_al(env, robot, T, B, box, mode="one_call", group=0):
    """AL_mpc.MPC built and called twice under guards (cold call with gradients, then the warm call) -> (outputs, sizes,
    launches of the cold call).  mode: "one_call" dqp_al_mpc_solve[_xbounds]; "persistent" the single-launch
    dqp_al_mpc_solve_fused; "per_iteration" dqp_al_newton_solve + dqp_al_outer_update per AL iteration; "dense" the same
    on the dense (non-banded) Newton kernels."""
    import test_gpu_al_xbounds as xb
    from diff_qp_mpc_amd import AL_mpc, al_utils
    from diff_qp_mpc_amd.dynamics import DeviceDynamics
    _lib, _, lib = env
    n, m = xb.SIZES[robot]
    p, xl, xh, o1, o2, dQ, dq = al_case(robot, T, B, box)
    dyn = DeviceDynamics(robot, dt=p["dt"])
    launches = []
    switches = {"one_call": {}, "persistent": dict(PERSISTENT_SOLVE=True, PERSISTENT_SOLVE_MAX_BATCH=1 << 20),
                "per_iteration": dict(ONE_CALL_SOLVE=False), "dense": dict(ONE_CALL_SOLVE=False)}[mode]

    def fn(t):
        x0, Qd, c, x_init, u_init, lo, hi = t[:7]
        state = dict(x_lower=t[7], x_upper=t[8]) if box == "state" else {}
        C = torch.diag_embed(Qd).requires_grad_()
        c = c.requires_grad_()
        ctrl = AL_mpc.MPC(n, m, T, u_lower=lo, u_upper=hi, n_batch=B, verbose=0, al_iter=2, solver_type="dense",
                          dtype=torch.float64, eps=1e-5, exit_unconverged=False, backprop=False, **state)
        ctrl.reinitialize(x0, torch.ones(B, T, 1, device="cuda"))
        ctrl.x_init, ctrl.u_init = x_init, u_init
        with _lib.trace(1024) as tr:
            x, u = ctrl(x0, al_utils.QuadCost(C, c), dyn, dyn.jac)
        launches.append([k for k, _ in tr.records])
        o = dict(x1=x.detach(), u1=u.detach(), lam1=ctrl.lamda_prev.clone(), rho1=ctrl.rho_prev.clone())
        (x.double().sum() + 2.0 * u.double().sum()).backward()
        o.update(dC=C.grad.diagonal(dim1=-2, dim2=-1).clone(), dc=c.grad)
        x, u = ctrl(x0, al_utils.QuadCost(C.detach(), c.detach()), dyn, dyn.jac)
        o.update(x2=x, u2=u, lam2=ctrl.lamda_prev.clone(), rho2=ctrl.rho_prev.clone())
        assert not any(bool(f.any()) for f in ctrl.fail_log)
        return o

    def make(put):
        t = [put(p[k], k) for k in ("x0", "Qd", "c", "x_init", "u_init", "lo", "hi")]
        return t + ([put(xl, "x_lower"), put(xh, "x_upper")] if box == "state" else [])

    old = {k: getattr(AL_mpc, k) for k in switches}
    old_banded = al_utils.BANDED_NEWTON_AL
    try:
        for k, v in switches.items():
            setattr(AL_mpc, k, v)
        if mode == "dense":
            al_utils.BANDED_NEWTON_AL = False
        assert lib.dqp_al_lane_group(group) == 0
        out, sizes = gb.run_guarded(fn, make)
    finally:
        for k, v in old.items():
            setattr(AL_mpc, k, v)
        al_utils.BANDED_NEWTON_AL = old_banded
        lib.dqp_al_lane_group(0)
    tol = xb.mpc_tol(robot)
    for call, o, lam_tol in (("1", o1, tol["lam"][0]), ("2", o2, tol["lam"][1])):
        for k in ("x", "u"):
            np.testing.assert_allclose(np_(out[k + call]), o[k], rtol=tol["xu"][0], atol=tol["xu"][1], err_msg=k + call)
        np.testing.assert_allclose(np_(out["lam" + call]), o["lam"], rtol=lam_tol[0], atol=lam_tol[1], err_msg="lam" + call)
        np.testing.assert_array_equal(np_(out["rho" + call]).reshape(-1), o["rho"].reshape(-1), err_msg="rho" + call)
    atol = 1e-6 if robot == "pendulum_euler" else 1e-5            # test_gpu_al.py:253-254, :295-296
    np.testing.assert_allclose(np_(out["dC"]), dQ, rtol=1e-4, atol=atol, err_msg="dC")
    np.testing.assert_allclose(np_(out["dc"]), dq, rtol=1e-4, atol=atol, err_msg="dc")
    assert nonzero_finite(np_(out["x1"])) and nonzero_finite(np_(out["dc"]))
    return out, sizes, launches[0], _lib.dqp_al_mpc_dims(B, n, m, T), dyn


# pendulum_euler at both lane groups (8: eight problems per wavefront, 16: four); cartpole2l on both sides of the
# LDS-resident factor's threshold (T 5 in LDS, T 6 in memory: test_gpu_al_xbounds.py); rexquadrotor: the full 16-lane row
AL_CASES = [("pendulum_euler", 5, 3, 8), ("pendulum_euler", 5, 3, 16), ("cartpole2l", 5, 3, 0), ("cartpole2l", 6, 3, 0),
            ("rexquadrotor", 4, 3, 0)]


@pytest.mark.parametrize("box", ["control", "state"])
@pytest.mark.parametrize("robot,T,B,group", AL_CASES)
def test_al_mpc_one_call_solve(env, robot, T, B, group, box):
    _lib, _, lib = env
    out, sizes, names, dims, dyn = run_al(env, robot, T, B, box, group=group)
    r = ctypes.byref(dims)
    ws = int(lib.dqp_al_mpc_solve_xbounds_bytes(r) if box == "state" else lib.dqp_al_mpc_solve_bytes(r))
    fac = int(lib.dqp_al_banded_factor_bytes(r, dyn.id))
    assert ws > 0 and fac > 0 and ws in sizes and fac in sizes, (ws, fac, sizes)
    newton = [k for k in names if "al_banded_newton_kernel" in k]
    kind = "BoxBounds<" if box == "state" else "StridedBounds<"
    assert len(newton) == 8 and all("al_banded_newton_kernel<dqp::" + kind in k for k in newton), names


@pytest.mark.parametrize("B", [1, 3])
def test_al_mpc_single_launch_solve(env, B):
    _lib, _, lib = env
    out, sizes, names, dims, dyn = run_al(env, "pendulum_euler", 5, B, "control", mode="persistent")
    assert len(names) == 1 and "al_solve_fused_kernel" in names[0], names
    m = dyn.n_ctrl
    bd = _lib.dqp_al_bounds(None, None, 5 * m, m)
    ws = int(lib.dqp_al_mpc_solve_fused_bytes(ctypes.byref(dims)))
    assert ws > 0 and ws == int(lib.dqp_al_mpc_solve_fused_bytes_bounds(ctypes.byref(dims), ctypes.byref(bd))) and ws in sizes


@pytest.mark.parametrize("mode", ["per_iteration", "dense"])
def test_al_mpc_newton_solve_per_iteration(env, mode):
    """dqp_al_newton_solve per AL iteration at pendulum_euler T 5 B 3: on the block-tridiagonal kernels, and on the
    dense (non-banded) Newton kernels with the Jacobian and the Hessian in the workspace"""
    _lib, _, lib = env
    out, sizes, names, dims, dyn = run_al(env, "pendulum_euler", 5, 3, "control", mode=mode)
    ws = int(lib.dqp_al_newton_solve_bytes(ctypes.byref(dims), 0 if mode == "dense" else 1))
    assert ws > 0 and ws in sizes, (ws, sizes)
    assert any("al_banded_newton_kernel" in k for k in names) == (mode != "dense"), names
    assert not any("al_start" in k for k in names)
    if mode == "dense":
        assert 3 * 15 * 15 * 8 in sizes                      # L (B, nz, nz)
    else:
        assert int(lib.dqp_al_banded_factor_bytes(ctypes.byref(dims), dyn.id)) in sizes


# ------------------------------------------------------------------------------------------ caller-linearised banded step
@functools.lru_cache(maxsize=None)
def given_case(n, m, T, B, entry):
    """test_gpu_al_given.py's data of one Newton step with a caller's linearisation (test_gpu_al_given_xbounds.py's with a
    state box) and the dense numpy oracle's update and factor solve, once per case"""
    import test_gpu_al_given as gv
    import test_gpu_al_given_xbounds as gx
    from oracle import al_oracle
    seed = 1000 * n + 10 * m + T + 3
    if entry == "jac_xbounds":
        p = gx.xproblem(n, m, T, B=B, seed=seed)
        upd, L, info = gx.oracle_xstep(p)
    else:
        p = gv.problem(n, m, T, B=B, seed=seed)
        upd, L, info = gv.oracle_step(p)
    assert not info.any()
    return p, upd, al_oracle.chol_solve_neg(L, p["rhs"].reshape(B, -1))


@pytest.mark.parametrize("entry", ["jac", "jac_bounds", "jac_xbounds"])
@pytest.mark.parametrize("n,m,T", [(4, 1, 6), (13, 4, 4), (24, 8, 3)])
def test_al_banded_step_with_the_callers_jacobians(env, n, m, T, entry):
    """dqp_al_banded_newton_step_jac / _jac_bounds / _jac_xbounds, then dqp_al_banded_solve on the factor, B = 3: a
    16-lane pair (four problems per wavefront) and the two wide ones (two per wavefront), against the dense oracle at
    test_gpu_al_given.py's rtol 1e-8 / atol 1e-10.  Bounds: the vector; per knot (the wide pairs read strided control
    bounds only next to a state box: the vector there); per sample and knot for both boxes."""
    import test_gpu_al_given as gv
    from diff_qp_mpc_amd import al_utils
    _lib, _, lib = env
    B, nt = 3, n + m
    p, upd_ref, sol_ref = given_case(n, m, T, B, entry)
    dims = _lib.dqp_al_mpc_dims(B, n, m, T)
    fb = int(lib.dqp_al_banded_jac_factor_bytes(ctypes.byref(dims)))
    assert fb == B * T * nt * (nt + 1 + n) * 8
    if nt <= 16:
        assert fb == int(lib.dqp_al_banded_factor_bytes(ctypes.byref(dims), 0))
    lo, hi = p["lo"], p["hi"]
    if entry == "jac_xbounds":
        lo, hi = [np.ascontiguousarray(np.broadcast_to(a, (B, T, m))) for a in (lo, hi)]
    elif entry == "jac_bounds" and nt <= 16:
        lo, hi = [np.ascontiguousarray(np.broadcast_to(a, (T, m))) for a in (lo, hi)]
    keys = ("xu", "x0", "Qd", "q", "lam", "rho", "xn", "Jx", "Ju", "rhs")

    def fn(t):
        d = dict(zip(keys + ("lo", "hi", "xl", "xh"), t))
        kw = dict(dtype=torch.float64, device="cuda")
        fac, upd, out = torch.empty(fb // 8, **kw), torch.empty(B, T, nt, **kw), torch.empty(B, T, nt, **kw)
        info = torch.empty(B, dtype=torch.int32, device="cuda")
        head = (dims, d["xu"], d["x0"], d["Qd"], d["q"], d["lam"], d["rho"].reshape(B))
        tail = (d["xn"], d["Jx"], d["Ju"], upd, fac, info)
        dev = d["xu"].device
        if entry == "jac":
            _lib.call("dqp_al_banded_newton_step_jac", dev, *head, d["lo"], d["hi"], *tail)
        else:
            bd = al_utils.bounds_layout(d["lo"], d["hi"], B, T, m)
            if entry == "jac_bounds":
                _lib.call("dqp_al_banded_newton_step_jac_bounds", dev, *head, bd.ref(), *tail)
            else:
                xbd = al_utils.bounds_layout(d["xl"], d["xh"], B, T, n)
                _lib.call("dqp_al_banded_newton_step_jac_xbounds", dev, *head, bd.ref(), xbd.ref(), *tail)
        _lib.call("dqp_al_banded_solve", dev, dims, 0, fac, d["rhs"], out)
        return upd, out, info

    def make(put):
        t = [put(p[k], k) for k in keys] + [put(lo, "lower"), put(hi, "upper")]
        return t + ([put(p["xl"], "x_lower"), put(p["xh"], "x_upper")] if entry == "jac_xbounds" else [])

    (upd, out, info), sizes = gb.run_guarded(fn, make)
    assert (np_(info) == 0).all()
    np.testing.assert_allclose(np_(upd).reshape(B, -1), upd_ref, **gv.UT)
    np.testing.assert_allclose(np_(out).reshape(B, -1), sol_ref, **gv.UT)
    assert fb in sizes and nonzero_finite(np_(upd))


# ------------------------------------------------------------------------------------------ device SQP rounds
def test_mpc_sqp_round(env):
    """dqp_mpc_sqp_rounds, one round at pendulum_dx T 4 B 3, against the Python round as
    test_gpu_mpc_sqp.py::test_one_round_equals_the_python_round (rtol 1e-5 / atol 1e-7); the workspace at exactly
    dqp_mpc_sqp_workspace_bytes."""
    import test_gpu_mpc_sqp as sqp
    from diff_qp_mpc_amd import qp_wrapper
    from diff_qp_mpc_amd.al_utils import mpc_bounds_layout
    _lib, _, lib = env
    T, B = 4, 3
    p = sqp.problem("pendulum_dx", T, B)
    n, m, dyn = p["n"], p["m"], p["dyn"]
    mpc = sqp.make_mpc(p)
    with torch.no_grad():
        x_start = mpc.rollout(p["x0"], p["u0"], dyn).clone()
    xn, un, cn = sqp.python_round(p, mpc, x_start, p["u0"])
    dims = _lib.dqp_mpc_dims(B, n, m, T, 1, dyn.id)
    opts = qp_wrapper._mpc_qp_opts(dyn.dt)
    nbytes = int(lib.dqp_mpc_sqp_workspace_bytes(ctypes.byref(dims), ctypes.byref(opts)))
    assert nbytes > 0 and nbytes % 8 == 0

    def fn(t):
        C, c, x0, lo, hi, xs, us = t
        kw = dict(dtype=torch.float64, device="cuda")
        x, u, keep_x, keep_u = torch.empty(T, B, n, **kw), torch.empty(T, B, m, **kw), torch.empty(T, B, n, **kw), torch.empty(T, B, m, **kw)
        x.copy_(xs); u.copy_(us)
        keep_cost = torch.full((B,), -1e300, **kw)                   # round 0 must not compare with it
        state = torch.full((4,), 5, dtype=torch.int32, device="cuda")        # round 0 must clear it
        ws = torch.empty(nbytes // 8, **kw)
        bounds = mpc_bounds_layout(lo, hi, B, T, m)
        _lib.call("dqp_mpc_sqp_rounds", x0.device, dims, opts, C, c, x0, bounds.ref(), float(mpc.linesearch_decay),
                  int(mpc.max_linesearch_iter), float(mpc.best_cost_eps), float(mpc.eps), 0, 1, x, u, keep_x, keep_u, keep_cost,
                  state, ws)
        return x, u, keep_x, keep_u, keep_cost, state

    names = ("C", "c", "x0", "lower", "upper", "x", "u")
    src = (p["C"], p["c"], p["x0"], p["lo"], p["hi"], x_start, p["u0"])
    (x, u, keep_x, keep_u, keep_cost, state), sizes = gb.run_guarded(fn, lambda put: [put(a.cpu(), k) for a, k in zip(src, names)])
    assert state.tolist() == [0, 1, 0, 0]
    tol = dict(rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(np_(x), np_(xn), **tol)
    np.testing.assert_allclose(np_(u), np_(un), **tol)
    np.testing.assert_allclose(np_(keep_cost), np_(cn), **tol)
    assert torch.equal(keep_x, x) and torch.equal(keep_u, u)
    assert nbytes in sizes and nonzero_finite(np_(x))


@pytest.mark.parametrize("termination", ["batch", "per_problem"])
def test_stagewise_mpc_qp_through_the_python_layer(env, termination):
    """qp_wrapper._MPCQP (what qp_wrapper.MPC runs per QP) with (T, B, m) bounds at (3, 1) T 4 B 5 -- no null-space kernel
    has this QP size, so forward and backward take the stage-wise kernels -- allocating its own outputs, workspace and
    termination buffer; as test_gpu_mpc_bounds.py::test_varying_bounds_per_problem_termination_through_the_python_layer."""
    import test_gpu_mpc_bounds as mb
    from diff_qp_mpc_amd import qp_wrapper
    _lib, qpmod, lib = env
    n, m, T, B = 3, 1, 4, 5
    data, lo, hi, strides, w, want = stage_problem(n, m, T, B, 0)
    kernels = []

    def fn(t):
        ins = [a.requires_grad_() for a in t[:5]]
        old = qpmod.TERMINATION
        qpmod.TERMINATION = termination
        try:
            with _lib.trace(64) as tr:
                tau = qp_wrapper._MPCQP.apply(*ins, t[5], t[6], n, m, T)
        finally:
            qpmod.TERMINATION = old
        kernels.append([k for k, _ in tr.records])
        (tau * t[7]).sum().backward()
        return dict(zip(("tau",) + mb.GRADS, [tau.detach()] + [a.grad for a in ins]))

    names = ("C", "c", "F", "f", "x0", "lower", "upper", "dl_dtau")
    out, sizes = gb.run_guarded(fn, lambda put: [put(a, k) for a, k in zip(data + (lo, hi, w), names)])
    assert mb._strided_kernels(kernels[0])
    np.testing.assert_allclose(np_(out["tau"]), want["tau"], **ZT)
    for k in mb.GRADS:
        np.testing.assert_allclose(np_(out[k]), want[k], err_msg=k, **GT)
    dims = _lib.dqp_mpc_dims(B, n, m, T, 1, 0)
    wsb = int(lib.dqp_mpc_qp_workspace_bytes(ctypes.byref(dims)))
    assert wsb > 0 and wsb in sizes, (wsb, sizes)
    assert nonzero_finite(np_(out["tau"])) and nonzero_finite(np_(out["dC"]))


# ------------------------------------------------------------------------------------------ the helper on the device
def test_the_helper_sees_a_store_on_the_device():
    """guardband.py on device memory (tests/test_guardband_cpu.py has the rest): the payload keeps the alignment of a
    fresh allocation, patched_allocations intercepts the device under test, and one element stored past the payload
    -- into the test's own allocation -- fails the check at the right offset."""
    t, h = gb.guarded((3, 5), torch.float64, "cuda", "nan")
    fresh = torch.empty(3, 5, dtype=torch.float64, device="cuda")
    assert t.is_cuda and t.is_contiguous() and t.data_ptr() % 512 == fresh.data_ptr() % 512 == 0
    assert torch.isnan(t).all()
    h.check()
    h.raw.view(torch.float64)[h.guard_bytes // 8 + t.numel()] = 1.0
    with pytest.raises(AssertionError, match="first at payload offset 12[0-7], last at payload offset 127"):
        h.check()
    with gb.patched_allocations("zero", "cuda") as reg:
        a = torch.empty(7, dtype=torch.int32, device=torch.device("cuda", 0))
        b = torch.zeros(2, 2, dtype=torch.float64, device="cuda")
        c = torch.empty(4, dtype=torch.float64)                      # the CPU is not the device under test
        d = torch.empty_like(b)
    assert reg.sizes == [28, 32, 32] and a.is_cuda and not c.is_cuda and (d == 0).all()
    with pytest.raises(AssertionError, match="first at payload offset -8,"):
        with gb.patched_allocations("nan", "cuda") as reg:
            a = torch.empty(3, dtype=torch.float64, device="cuda")
            reg.handles[0].raw.view(torch.float64)[reg.handles[0].guard_bytes // 8 - 1] = 0.0


# ------------------------------------------------------------------------------------------ AL entries through the C ABI
# AL_mpc.MPC copies and recombines its iterate, multipliers and penalty with torch arithmetic (torch.cat, .clone(),
# rho * 10, warm_start_al), which no patch intercepts: in the Python-layer cases above x0, q, the bounds, the
# workspace, the factor and the outputs sit between guards, the in/out iterate, lam and rho of the later calls do not.
# The cases below call the same entry points directly with EVERY array guarded.
@functools.lru_cache(maxsize=None)
def newton_case(robot, T, B, box):
    """test_gpu_al_xbounds.py::step_data (random iterate, multipliers, penalties 1 / 10 / 100, per-sample per-knot control
    box and state box) and oracle/al_solve_oracle.newton_al on it (over the extended rows with the state box) + the
    oracle's factor solve of a random right-hand side, once per case"""
    import contextlib
    import al_xbounds_oracle as xo
    import test_gpu_al_xbounds as xb
    from oracle import al_solve_oracle as aso
    n, m = xb.SIZES[robot]
    d, lo, hi, xl, xh = xb.step_data(robot, T, B, seed=7 * T + B)
    if box == "vector":                     # the n_ctrl-vector form of the control box: sample 0's first knot
        lo, hi = lo[0, 0].copy(), hi[0, 0].copy()
    lam = d["lam"] if box == "state" else np.ascontiguousarray(d["lam"][:, :T * n + 2 * T * m])
    step = xb.host_step(robot, 0.05)
    with (xo.extended(xl, xh) if box == "state" else contextlib.nullcontext()):
        x_est, L, status, chol_fail = aso.newton_al(d["xu"], d["x0"], lam, d["rho"], d["Qd"], d["q"], lo, hi, step)
    assert not chol_fail
    rhs = np.random.default_rng(T + B).standard_normal((B, T, n + m))
    sol = aso.backward(L, x_est, rhs)[1]
    return d, lam, lo, hi, xl, xh, x_est, status, rhs, sol


# T = 33: the line search beyond the lane groups' horizons (al_ls_kernel), with the control box as a vector ("vector"),
# per sample and knot ("control") and with a state box
NEWTON_CASES = [(r, T, B, g, box, 1) for r, T, B, g in AL_CASES for box in ("control", "state")] + \
               [("pendulum_euler", 5, 3, 0, "control", 0), ("pendulum_euler", 5, 3, 0, "vector", 0)] + \
               [("integrator", 33, 3, 0, box, 1) for box in ("vector", "control", "state")]


@pytest.mark.parametrize("robot,T,B,group,box,banded", NEWTON_CASES)
def test_al_newton_solve_through_the_c_abi(env, robot, T, B, group, box, banded):
    """dqp_al_newton_solve_bounds (block-tridiagonal, and banded == 0: the dense Newton kernels with the Jacobian and the
    Hessian in the workspace) and dqp_al_newton_solve_xbounds, then the factor's solve (dqp_al_banded_solve /
    dqp_al_chol_solve), with the in/out iterate, multipliers, penalties, both boxes, status, flag, factor and workspace
    all between guards.  Against al_solve_oracle.newton_al as test_gpu_dyn_registry.py::test_al_newton_solve_vs_oracle:
    iterate rtol 1e-4 / atol 1e-5, acceptance of the last step exactly; the factor solve at the gradients' tolerance
    (test_gpu_al.py:253-254, :295-296: rtol 1e-4, atol 1e-6 pendulum / 1e-5 others)."""
    from diff_qp_mpc_amd import al_utils
    from diff_qp_mpc_amd.dynamics import DeviceDynamics
    _lib, _, lib = env
    dyn = DeviceDynamics(robot, dt=0.05)            # newton_case's step
    n, m = dyn.n_state, dyn.n_ctrl
    nt, nz = n + m, T * (n + m)
    d, lam, lo, hi, xl, xh, x_est, status_ref, rhs, sol = newton_case(robot, T, B, box)
    dims = _lib.dqp_al_mpc_dims(B, n, m, T)
    r = ctypes.byref(dims)
    wsb = int(lib.dqp_al_newton_solve_xbounds_bytes(r) if box == "state" else lib.dqp_al_newton_solve_bytes(r, banded))
    fb = int(lib.dqp_al_banded_factor_bytes(r, dyn.id)) if banded else B * nz * nz * 8
    assert wsb > 0 and fb > 0
    launches = []

    def fn(t):
        xu, x0, Qd, q, lam_d, rho, lo_d, hi_d, rhs_d = t[:9]
        kw = dict(dtype=torch.float64, device="cuda")
        bd = al_utils.bounds_layout(lo_d, hi_d, B, T, m)
        L, ws, status, out = torch.empty(fb // 8, **kw), torch.empty(wsb // 8, **kw), torch.empty(B, **kw), torch.empty(B, T, nt, **kw)
        fail = torch.empty(1, dtype=torch.int32, device="cuda")
        with _lib.trace(256) as tr:
            if box == "state":
                xbd = al_utils.bounds_layout(t[9], t[10], B, T, n)
                _lib.call("dqp_al_newton_solve_xbounds", xu.device, dims, dyn.id, dyn.dt, 4, x0, Qd, q, lam_d, rho, bd.ref(),
                          xbd.ref(), xu, L, status, fail, ws)
            else:
                _lib.call("dqp_al_newton_solve_bounds", xu.device, dims, dyn.id, dyn.dt, 4, banded, x0, Qd, q, lam_d, rho,
                          bd.ref(), xu, L, status, fail, ws)
            if banded:
                _lib.call("dqp_al_banded_solve", xu.device, dims, dyn.id, L, rhs_d, out)
            else:
                _lib.call("dqp_al_chol_solve", xu.device, _lib.dqp_al_dims(B, nz, 0, 0), L, rhs_d, out)
        launches.append([k for k, _ in tr.records])
        return xu, status, fail, out

    def make(put):
        t = [put(d["xu"], "xu (in/out)"), put(d["x0"], "x0"), put(d["Qd"], "Qd"), put(d["q"], "q"), put(lam, "lam"),
             put(d["rho"].reshape(B), "rho"), put(lo, "lower"), put(hi, "upper"), put(rhs, "rhs")]
        return t + ([put(xl, "x_lower"), put(xh, "x_upper")] if box == "state" else [])

    try:
        assert lib.dqp_al_lane_group(group) == 0
        (xu, status, fail, out), sizes = gb.run_guarded(fn, make)
    finally:
        lib.dqp_al_lane_group(0)
    assert not np_(fail).any()
    print(robot, box, "max |xu - oracle| = %.3e, max |solve - oracle| = %.3e"
          % (np.abs(np_(xu) - x_est).max(), np.abs(np_(out) - sol).max()))
    np.testing.assert_allclose(np_(xu), x_est, rtol=1e-4, atol=1e-5)
    np.testing.assert_array_equal(np_(status) != 0.0, status_ref)
    np.testing.assert_allclose(np_(out), sol, rtol=1e-4, atol=1e-6 if robot == "pendulum_euler" else 1e-5)
    assert nonzero_finite(np_(xu)) and nonzero_finite(np_(out))
    newton = [k for k in launches[0] if "al_banded_newton_kernel" in k]
    assert len(newton) == (4 if banded else 0), launches[0]
    family = {"state": "BoxBounds<", "control": "StridedBounds<", "vector": None}[box]
    reads_bounds = newton + [k for k in launches[0] if "al_ls_kernel<" in k or "al_ls_group_kernel<" in k]
    assert all((family in k) if family else ("Bounds<" not in k) for k in reads_bounds), reads_bounds
    assert any("al_ls_kernel<" in k for k in launches[0]) == (T > 32), launches[0]
    assert wsb in sizes and fb in sizes, (wsb, fb, sizes)


@pytest.mark.parametrize("robot,T,B,group,box,fused", [(r, T, B, g, box, False) for r, T, B, g in AL_CASES for box in ("control", "state")] +
                         [("pendulum_euler", 5, 1, 0, "control", True), ("pendulum_euler", 5, 3, 0, "control", True)])
def test_al_mpc_solve_through_the_c_abi(env, robot, T, B, group, box, fused):
    """dqp_al_mpc_solve_bounds / _xbounds / dqp_al_mpc_solve_fused_bounds, cold (n_prev = 0) and then warm from the cold
    call's history, every array between guards: start, x0, cost, both boxes, multipliers and penalties in, iterate,
    the three history arrays, residual norm, factor, status, flags and workspace out.  Against the oracle's two calls
    (al_case) at test_gpu_al_xbounds.py's mpc_tol; the warm call starts from the float32 rounding of the cold solution,
    as AL_mpc.MPC's does (AL_mpc.py:250-251)."""
    import test_gpu_al_xbounds as xb
    from diff_qp_mpc_amd import al_utils
    from diff_qp_mpc_amd.dynamics import DeviceDynamics
    _lib, _, lib = env
    p, xl, xh, o1, o2, _, _ = al_case(robot, T, B, box)
    dyn = DeviceDynamics(robot, dt=p["dt"])
    n, m = dyn.n_state, dyn.n_ctrl
    nt = n + m
    ncon = o1["lam"].shape[1]
    dims = _lib.dqp_al_mpc_dims(B, n, m, T)
    r = ctypes.byref(dims)
    bd0 = _lib.dqp_al_bounds(None, None, T * m, m)
    wsb = int(lib.dqp_al_mpc_solve_xbounds_bytes(r) if box == "state" else
              lib.dqp_al_mpc_solve_fused_bytes_bounds(r, ctypes.byref(bd0)) if fused else lib.dqp_al_mpc_solve_bytes(r))
    fb = int(lib.dqp_al_banded_factor_bytes(r, dyn.id))
    assert wsb > 0 and fb > 0
    K = 3                                      # al_iter + 1 history entries
    launches = []

    def fn(t):
        x_init, u_init, x0, Qd, q, lo_d, hi_d, lam0, rho0 = t[:9]
        kw = dict(dtype=torch.float64, device="cuda")
        bd = al_utils.bounds_layout(lo_d, hi_d, B, T, m)
        xbd = al_utils.bounds_layout(t[9], t[10], B, T, n) if box == "state" else None
        res = {}
        prev, n_prev, lam_in, rho_in = (None, None, None), 0, lam0, rho0
        for call in ("1", "2"):
            xu, hc, hl, hr = torch.empty(B, T, nt, **kw), torch.empty(K, B, **kw), torch.empty(K, B, ncon, **kw), torch.empty(K, B, **kw)
            resn, status, L, ws = torch.empty(B, **kw), torch.empty(B, **kw), torch.empty(fb // 8, **kw), torch.empty(wsb // 8, **kw)
            fail = torch.empty(2, dtype=torch.int32, device="cuda")
            head = (dims, dyn.id, dyn.dt, 2, 4, x_init, u_init, x0, Qd, q, bd.ref())
            tail = (lam_in, rho_in, *prev, n_prev, xu, hc, hl, hr, resn, L, status, fail, ws)
            with _lib.trace(1024) as tr:
                if box == "state":
                    _lib.call("dqp_al_mpc_solve_xbounds", x0.device, *head, xbd.ref(), *tail)
                else:
                    _lib.call("dqp_al_mpc_solve_fused_bounds" if fused else "dqp_al_mpc_solve_bounds", x0.device, *head, *tail)
            launches.append([k for k, _ in tr.records])
            res.update({"xu" + call: xu, "hc" + call: hc, "hl" + call: hl, "hr" + call: hr, "resn" + call: resn, "fail" + call: fail})
            # the warm call: the float32 rounding of this solution as the start, this call's history, its last entry in
            x_init, u_init = torch.empty(B, T, n, **kw), torch.empty(B, T, m, **kw)
            x_init.copy_(xu[:, :, :n].float())
            u_init.copy_(xu[:, :, n:].float())
            prev, n_prev = (hc, hl, hr), K
            lam_in, rho_in = torch.empty(B, ncon, **kw), torch.empty(B, **kw)
            lam_in.copy_(hl[-1])
            rho_in.copy_(hr[-1])
        return res

    def make(put):
        t = [put(p[k], k) for k in ("x_init", "u_init", "x0", "Qd", "c", "lo", "hi")]
        t += [put(np.zeros((B, ncon)), "lam_in"), put(np.ones(B), "rho_in")]
        return t + ([put(xl, "x_lower"), put(xh, "x_upper")] if box == "state" else [])

    try:
        assert lib.dqp_al_lane_group(group) == 0
        out, sizes = gb.run_guarded(fn, make)
    finally:
        lib.dqp_al_lane_group(0)
    tol = xb.mpc_tol(robot)
    for call, o, lam_tol in (("1", o1, tol["lam"][0]), ("2", o2, tol["lam"][1])):
        assert not np_(out["fail" + call]).any()
        # (the oracle's x, u are what AL_mpc.MPC returns: compared, as there, after the float32 rounding of the output)
        got = np_(out["xu" + call].float())
        np.testing.assert_allclose(got, o["xu"], rtol=tol["xu"][0], atol=tol["xu"][1], err_msg="xu" + call)
        np.testing.assert_allclose(np_(out["hl" + call][-1]), o["lam"], rtol=lam_tol[0], atol=lam_tol[1], err_msg="lam" + call)
        np.testing.assert_array_equal(np_(out["hr" + call][-1]), o["rho"].reshape(-1), err_msg="rho" + call)
    assert nonzero_finite(np_(out["xu1"])) and nonzero_finite(np_(out["hl2"]))
    if fused:
        assert all(len(k) == 1 and "al_solve_fused_kernel" in k[0] for k in launches[:2]), launches[:2]
    else:
        newton = [k for k in launches[0] if "al_banded_newton_kernel" in k]
        assert len(newton) == 8 and all(("BoxBounds<" if box == "state" else "StridedBounds<") in k for k in newton), launches[0]
    assert wsb in sizes and fb in sizes, (wsb, fb, sizes)
