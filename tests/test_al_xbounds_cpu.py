"""State bounds (x_lower / x_upper) of AL_mpc.MPC without a GPU: the header, the library and the binding have the
`_xbounds` entry points; dqp_al_ncon_xbounds and the `_bytes` queries answer; the return-code table of every new entry;
the general torch path (residuals, clamped Jacobian, one NewtonAL step + outer update) on CPU tensors against the numpy
oracle over extended rows (tests/al_xbounds_oracle.py); the constructor's shape and finiteness checks."""
import ctypes
import os

import numpy as np
import pytest
import torch

import al_xbounds_oracle as xo
from oracle import al_oracle, al_solve_oracle as aso

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DQP_ERR_BAD_ARG, DQP_ERR_TOO_LARGE = -1, -2
LAUNCHING = ("dqp_al_banded_newton_step_xbounds", "dqp_al_newton_solve_xbounds", "dqp_al_outer_update_xbounds",
             "dqp_al_mpc_solve_xbounds")
QUERIES = ("dqp_al_ncon_xbounds", "dqp_al_newton_solve_xbounds_bytes", "dqp_al_mpc_solve_xbounds_bytes")
# the registered models (include/dqp.h: DQP_DYN_*) and their sizes: every new entry takes a model
SIZES = {"pendulum1l": (2, 1), "cartpole1l": (4, 1), "cartpole2l": (6, 1), "pendulum_euler": (2, 1), "pendulum_dx": (3, 1),
         "integrator": (2, 1), "rexquadrotor": (12, 4)}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from diff_qp_mpc_amd import _lib
    return _lib.load()


def test_declared_exported_and_bound(lib):
    from diff_qp_mpc_amd import _lib
    header = open(os.path.join(ROOT, "include", "dqp.h")).read()
    for s in LAUNCHING + QUERIES:
        assert s + "(" in header, s
        assert s in _lib.SYMBOLS and hasattr(lib, s), s
    for s in LAUNCHING:
        restype, argtypes, names = _lib.PROTOTYPES[s]
        assert names[-1] == "stream" and names[1] == "model", (s, names)          # call() serves it; the model is `model`
        i = names.index("bounds")
        assert names[i + 1] == "xbounds" and argtypes[i] is argtypes[i + 1] is ctypes.POINTER(_lib.dqp_al_bounds), s
        twin = _lib.PROTOTYPES[s.replace("_xbounds", "_bounds")][2]
        assert [a for a in names if a not in ("xbounds", "model")] == [a for a in twin if a not in ("banded", "dyn_id")], s
    assert set(SIZES) == set(_lib.DQP_DYN)
    assert lib.dqp_version() == 303
    assert header.count("#define DQP_VERSION 303") == 1


def test_ncon_and_bytes_queries(lib):
    from diff_qp_mpc_amd import _lib
    r = ctypes.byref
    for (n, m) in set(SIZES.values()):
        for T in (2, 5, 33):
            for B in (1, 3):
                d = _lib.dqp_al_mpc_dims(B, n, m, T)
                assert lib.dqp_al_ncon_xbounds(r(d)) == T * n + 2 * T * m + 2 * T * n == xo.ncon_x(n, m, T)
                assert lib.dqp_al_newton_solve_xbounds_bytes(r(d)) >= lib.dqp_al_newton_solve_bytes(r(d), 1) > 0
                assert lib.dqp_al_mpc_solve_xbounds_bytes(r(d)) >= lib.dqp_al_mpc_solve_bytes(r(d)) > 0
    assert lib.dqp_al_ncon_xbounds(None) == 0


def _call_all(lib, d, rid, bd, xbd, n_steps=4, al_iter=2, newton_steps=4, n_prev=0):
    """every new launching entry with null buffers -> {name: return code}; nothing is launched at nbatch == 0 or with
    null buffers"""
    r = ctypes.byref
    N = None
    return {
        "banded_newton_step": lib.dqp_al_banded_newton_step_xbounds(r(d), rid, 0.05, N, N, N, N, N, N, bd, xbd, N, N, N, N),
        "newton_solve": lib.dqp_al_newton_solve_xbounds(r(d), rid, 0.05, n_steps, N, N, N, N, N, bd, xbd, N, N, N, N, N, N),
        "outer_update": lib.dqp_al_outer_update_xbounds(r(d), rid, 0.05, N, N, N, N, N, N, bd, xbd, N, N, N, N),
        "mpc_solve": lib.dqp_al_mpc_solve_xbounds(r(d), rid, 0.05, al_iter, newton_steps, N, N, N, N, N, bd, xbd, N, N, N, N,
                                                  N, n_prev, N, N, N, N, N, N, N, N, N, N),
    }


# scalar argument faults of the `_xbounds` entries: behind al_xbounds_check (so behind DQP_ERR_TOO_LARGE), in front of the
# nbatch == 0 return.  (scalar arguments, the entries that then return DQP_ERR_BAD_ARG at sizes a model has)
SCALAR_FAULTS = [({"n_steps": 0}, ("newton_solve",)), ({"al_iter": 0}, ("mpc_solve",)), ({"al_iter": 257}, ("mpc_solve",)),
                 ({"newton_steps": 0}, ("mpc_solve",)), ({"n_prev": -1}, ("mpc_solve",)),
                 ({"n_steps": 0, "al_iter": 0}, ("newton_solve", "mpc_solve")), ({"al_iter": 256}, ())]


def test_return_code_table(lib):
    """At nbatch = 0 and, with null buffers, at nbatch = 3: unknown model ids, a registered id with foreign sizes, each
    model's own sizes, a null / bad-stride xbounds (and bounds), n + m > 16 and n > 12."""
    from diff_qp_mpc_amd import _lib
    T = 6
    keep = np.zeros(T * 16)
    ptr = keep.ctypes.data
    r = ctypes.byref
    box = lambda w, sb=0, st=0, p=ptr: _lib.dqp_al_bounds(p, p, sb, st)
    for B in (0, 3):
        for robot, (n, m) in SIZES.items():
            rid = _lib.DQP_DYN[robot]
            d = _lib.dqp_al_mpc_dims(B, n, m, T)
            ok_u = box(m)
            for sb, st in ((0, 0), (0, n), (n, 0), (T * n, 0), (T * n, n)):
                # own sizes: DQP_OK at nbatch == 0, the null buffers at nbatch > 0
                for name, rc in _call_all(lib, d, rid, r(ok_u), r(box(n, sb, st))).items():
                    assert rc == (0 if B == 0 else DQP_ERR_BAD_ARG), (robot, name, B, sb, st, rc)
                # null lower / upper of the state box: behind the nbatch == 0 return
                for name, rc in _call_all(lib, d, rid, r(ok_u), r(box(n, sb, st, None))).items():
                    assert rc == (0 if B == 0 else DQP_ERR_BAD_ARG), (robot, name, B, sb, st, rc)
            for scalars, refused in SCALAR_FAULTS:
                for name, rc in _call_all(lib, d, rid, r(ok_u), r(box(n)), **scalars).items():
                    want = DQP_ERR_BAD_ARG if (name in refused or B > 0) else 0
                    assert rc == want, (robot, name, B, scalars, rc)
            # a null or bad-stride state box, a null or bad-stride control box: in front of it
            for name, rc in _call_all(lib, d, rid, r(ok_u), None).items():
                assert rc == DQP_ERR_BAD_ARG, (robot, name, B, rc)
            for name, rc in _call_all(lib, d, rid, None, r(box(n))).items():
                assert rc == DQP_ERR_BAD_ARG, (robot, name, B, rc)
            for sb, st in ((n + 1, 0), (0, n + 1), (T * n, n + 1), (n, n), (T * n - 1, n), (-T * n, n), (0, -n)):
                for name, rc in _call_all(lib, d, rid, r(ok_u), r(box(n, sb, st))).items():
                    assert rc == DQP_ERR_BAD_ARG, (robot, name, B, sb, st, rc)
            if n != m:      # the control box's strides in the state box's place (and the other way round)
                for name, rc in _call_all(lib, d, rid, r(ok_u), r(box(n, T * m, m))).items():
                    assert rc == DQP_ERR_BAD_ARG, (robot, name, B, rc)
                for name, rc in _call_all(lib, d, rid, r(box(m, T * n, n)), r(box(n))).items():
                    assert rc == DQP_ERR_BAD_ARG, (robot, name, B, rc)
            # unknown ids with these sizes; another model's id
            for bad_id in (0, 8, -1):
                for name, rc in _call_all(lib, d, bad_id, r(ok_u), r(box(n))).items():
                    assert rc == DQP_ERR_BAD_ARG, (robot, name, B, bad_id, rc)
            other = next(k for k, v in SIZES.items() if v != (n, m))
            for name, rc in _call_all(lib, d, _lib.DQP_DYN[other], r(ok_u), r(box(n))).items():
                assert rc == DQP_ERR_BAD_ARG, (robot, name, B, other, rc)
        # beyond the block-tridiagonal kernels: DQP_ERR_TOO_LARGE whatever the model
        for n, m in ((13, 4), (13, 2), (12, 5), (16, 1)):
            d = _lib.dqp_al_mpc_dims(B, n, m, T)
            for rid in (0, _lib.DQP_DYN["rexquadrotor"]):
                for name, rc in _call_all(lib, d, rid, r(box(m)), r(box(n))).items():
                    assert rc == DQP_ERR_TOO_LARGE, (name, B, n, m, rid, rc)
                # two faults at once: illegal strides of either box are reported in front of the sizes' limit, and the
                # limit in front of the model (the rows above: no model has these sizes)
                for name, rc in _call_all(lib, d, rid, r(box(m)), r(box(n, n + 1, 0))).items():
                    assert rc == DQP_ERR_BAD_ARG, (name, B, n, m, rid, rc)
                for name, rc in _call_all(lib, d, rid, r(box(m, 0, m + 1)), r(box(n))).items():
                    assert rc == DQP_ERR_BAD_ARG, (name, B, n, m, rid, rc)
            for name, rc in _call_all(lib, d, 99, r(box(m)), r(box(n))).items():
                assert rc == DQP_ERR_TOO_LARGE, (name, B, n, m, rc)
            for scalars, _ in SCALAR_FAULTS:        # the limit in front of the scalar arguments
                for name, rc in _call_all(lib, d, _lib.DQP_DYN["rexquadrotor"], r(box(m)), r(box(n)), **scalars).items():
                    assert rc == DQP_ERR_TOO_LARGE, (name, B, n, m, scalars, rc)
        # the sizes and horizon checks of the twins
        for n, m, Tb in ((0, 1, T), (2, 0, T), (2, 1, 1)):
            d = _lib.dqp_al_mpc_dims(B, n, m, Tb)
            for name, rc in _call_all(lib, d, 1, r(box(1)), r(box(1))).items():
                assert rc == DQP_ERR_BAD_ARG, (name, n, m, Tb, rc)
    d = _lib.dqp_al_mpc_dims(-1, 2, 1, T)
    for name, rc in _call_all(lib, d, _lib.DQP_DYN["pendulum_euler"], r(box(1)), r(box(2))).items():
        assert rc == DQP_ERR_BAD_ARG, (name, rc)


# ------------------------------------------------------------------ the general torch path on CPU tensors
class ToyPendulum:
    """oracle/al_oracle.pendulum_step as a torch module with its own Jacobians (a caller-supplied dynamics)"""
    n_state, n_ctrl = 2, 1

    def __call__(self, x, u):
        return self.jac(x, u)[0]

    def jac(self, x, u):
        DT, G = al_oracle.DT, al_oracle.G
        th, thd = x[:, 0], x[:, 1]
        nthd = thd + (u[:, 0] + G * torch.sin(th)) * DT
        nth = th + nthd * DT
        c = G * torch.cos(th)
        Jx = torch.zeros(x.shape[0], 2, 2, dtype=x.dtype)
        Jx[:, 1, 0] = c * DT
        Jx[:, 1, 1] = 1.0
        Jx[:, 0, 0] = 1.0 + c * DT * DT
        Jx[:, 0, 1] = DT
        Ju = torch.zeros(x.shape[0], 2, 1, dtype=x.dtype)
        Ju[:, 1, 0] = DT
        Ju[:, 0, 0] = DT * DT
        return torch.stack((nth, nthd), 1), (Jx, Ju)


def toy_problem(B=3, T=5, seed=3):
    r = np.random.default_rng(seed)
    n, m = 2, 1
    xu = 0.5 * r.standard_normal((B, T, n + m))
    p = dict(xu=xu, x0=xu[:, 0, :n] + 0.1 * r.standard_normal((B, n)), Qd=r.random((B, T, n + m)) + 0.1,
             q=r.standard_normal((B, T, n + m)), lam=r.standard_normal((B, xo.ncon_x(n, m, T))),
             rho=10.0 ** r.integers(0, 3, (B, 1)).astype(np.float64),
             lo=np.full(m, -0.3), hi=np.full(m, 0.3))
    # a per-sample, per-knot state box around 0 that cuts through the N(0, 0.5^2) states
    w = 0.4 * np.linspace(0.5, 1.5, B)[:, None, None] * np.linspace(1.0, 0.4, T)[None, :, None] * np.array([1.0, 1.5])
    p["xl"], p["xh"] = -w, w + 0.05
    return p


def tt(a):
    return torch.tensor(np.asarray(a), dtype=torch.float64)


def test_general_path_rows_and_jacobian_vs_extended_oracle(monkeypatch):
    from diff_qp_mpc_amd import al_utils
    p = toy_problem()
    B, T, nt = p["xu"].shape
    n, m = 2, 1
    xo.install(monkeypatch, p["xl"], p["xh"])
    res_o, resc_o, J_o, Jc_o = al_oracle.constraint_jacobian(p["xu"], p["x0"], p["lo"], p["hi"])
    assert res_o.shape == (B, xo.ncon_x(n, m, T))
    sx = res_o[:, T * n + 2 * T * m:].reshape(B, T, 2 * n)
    assert ((sx > 0).any(2).any(1) & (sx.max(2) <= 0).any(1)).sum() >= 2          # active at some knots, none at others
    dyn = ToyPendulum()
    res, resc = al_utils.dyn_res(tt(p["xu"]), dyn, tt(p["x0"]), tt(p["xl"]), tt(p["xh"]), tt(p["lo"]), tt(p["hi"]))
    np.testing.assert_allclose(res.numpy(), res_o, rtol=0, atol=1e-14)
    np.testing.assert_allclose(resc.numpy(), resc_o, rtol=0, atol=1e-14)
    r2, rc2, J, Jc = al_utils.constraint_jacobian(tt(p["xu"]), tt(p["x0"]), dyn.jac, tt(p["lo"]), tt(p["hi"]), tt(p["xl"]),
                                                  tt(p["xh"]))
    np.testing.assert_allclose(r2.numpy(), res_o, rtol=0, atol=1e-14)
    np.testing.assert_allclose(J.numpy(), J_o, rtol=0, atol=1e-14)
    np.testing.assert_allclose(Jc.numpy(), Jc_o, rtol=0, atol=1e-14)
    x, u = tt(p["xu"][..., :n]), tt(p["xu"][..., n:])
    ri, rci, Ji, Jci = al_utils.dyn_res_ineq_jac(x, u, tt(p["x0"]), tt(p["xl"]), tt(p["xh"]), tt(p["lo"]), tt(p["hi"]))
    np.testing.assert_array_equal(Ji.numpy(), J_o[:, T * n:])
    np.testing.assert_array_equal(Jci.numpy(), Jc_o[:, T * n:])
    np.testing.assert_allclose(ri.numpy(), res_o[:, T * n:], rtol=0, atol=1e-14)
    # merit and gradient
    mer = al_utils.merit_function(tt(p["xu"]), tt(p["Qd"]), tt(p["q"]), dyn, tt(p["x0"]), tt(p["lam"]), tt(p["rho"]),
                                  tt(p["xl"]), tt(p["xh"]), tt(p["lo"]), tt(p["hi"]))
    want = aso.merit(p["xu"], p["Qd"], p["q"], p["x0"], p["lam"], p["rho"], p["lo"], p["hi"], al_oracle.pendulum_step)
    np.testing.assert_allclose(mer.numpy(), want, rtol=1e-13, atol=1e-12)
    grad, terms = al_utils.merit_grad_hessian(tt(p["xu"]), tt(p["Qd"]), tt(p["q"]), dyn, dyn.jac, tt(p["x0"]), tt(p["lam"]),
                                              tt(p["rho"]), tt(p["xl"]), tt(p["xh"]), tt(p["lo"]), tt(p["hi"]))
    g_o = al_oracle.merit_grad(p["xu"], p["Qd"], p["q"], p["lam"], p["rho"], resc_o, J_o, Jc_o)
    np.testing.assert_allclose(grad.numpy(), g_o, rtol=1e-13, atol=1e-12)
    np.testing.assert_allclose(terms.dense().numpy(), al_oracle.hessian(Jc_o, p["Qd"], p["rho"]), rtol=1e-13, atol=1e-12)
    # without the state box the rows are the ones they were
    res0, _ = al_utils.dyn_res(tt(p["xu"]), dyn, tt(p["x0"]), None, None, tt(p["lo"]), tt(p["hi"]))
    np.testing.assert_array_equal(res0.numpy(), res.numpy()[:, :T * n + 2 * T * m])


def test_general_path_newton_al_step_and_outer_update_vs_extended_oracle(monkeypatch):
    """AL_mpc.MPC.al_solve on CPU tensors with a toy module: one AL iteration of ONE Newton step (LU solve: the dense
    Newton kernel needs a GPU) with the line search and the multiplier update, against the extended oracle."""
    from diff_qp_mpc_amd import AL_mpc, al_utils
    p = toy_problem()
    B, T, nt = p["xu"].shape
    n, m = 2, 1
    monkeypatch.setattr(al_utils, "MAX_NEWTON_STEPS", 1)
    monkeypatch.setattr(al_utils, "DENSE_NEWTON_MAX_NZ", 0)
    monkeypatch.setattr(aso, "NEWTON_STEPS", 1)
    xo.install(monkeypatch, p["xl"], p["xh"])
    ctrl = AL_mpc.MPC(n, m, T, u_lower=tt(p["lo"]), u_upper=tt(p["hi"]), n_batch=B, al_iter=1, dtype=torch.float64,
                      x_lower=tt(p["xl"]), x_upper=tt(p["xh"]))
    ctrl.reinitialize(tt(p["x0"]), torch.ones(B, T, 1))
    assert ctrl.lamda_prev.shape == (B, xo.ncon_x(n, m, T))
    dyn = ToyPendulum()
    x, u = ctrl.al_solve(tt(p["xu"][..., :n]), tt(p["xu"][..., n:]), dyn, dyn.jac, tt(p["x0"]),
                         al_utils.QuadCost(tt(p["Qd"]), tt(p["q"])), lamda_init=tt(p["lam"]), rho_init=tt(p["rho"]))
    o = aso.al_solve(p["xu"][..., :n], p["xu"][..., n:], p["x0"], p["Qd"], p["q"], p["lo"], p["hi"], al_oracle.pendulum_step,
                     p["lam"], p["rho"], al_iter=1)
    assert np.abs(o["xu"] - p["xu"]).max() > 1e-3                         # a step was taken
    np.testing.assert_allclose(x.numpy(), o["x"], rtol=1e-6, atol=1e-6)      # (the outputs are float32, AL_mpc.py:319-320)
    np.testing.assert_allclose(u.numpy(), o["u"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(ctrl.lamda_prev.numpy(), o["lam"], rtol=1e-9, atol=1e-9)
    np.testing.assert_array_equal(ctrl.rho_prev.numpy(), o["rho"])
    assert (o["lam"][:, T * n + 2 * T * m:] > 0).any() and (o["lam"][:, T * n:] >= 0).all()


# ------------------------------------------------------------------ the constructor
def test_constructor_shapes_and_finiteness():
    from diff_qp_mpc_amd import AL_mpc
    B, T, n, m = 4, 5, 2, 1
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    mk = lambda **kw: AL_mpc.MPC(n, m, T, u_lower=-torch.ones(m), u_upper=torch.ones(m), n_batch=B, **kw)
    base = mk()
    assert base.x_lower is None and base.nineq == 2 * T * m and base.lamda_prev.shape == (B, T * n + 2 * T * m)
    for shape in ((n,), (T, n), (B, 1, n), (B, T, n)):
        c = mk(x_lower=z(*shape) - 1.0, x_upper=z(*shape) + 1.0)
        assert c.nineq == 2 * T * m + 2 * T * n and c.lamda_prev.shape == (B, xo.ncon_x(n, m, T))
        c.reinitialize(z(B, n), torch.ones(B, T, 1))
        assert c.lamda_prev.shape == (B, xo.ncon_x(n, m, T))
        assert c.x_lower.dtype == torch.float64 and c.x_lower.shape == shape
    with pytest.raises(ValueError):
        mk(x_lower=z(n))
    with pytest.raises(ValueError):
        mk(x_upper=z(n))
    for lo, hi in ((z(T, B, n), z(T, B, n)), (z(B, n), z(B, n)), (z(n), z(T, n)), (z(n + 1), z(n + 1)), (z(B, T, m), z(B, T, m))):
        with pytest.raises(ValueError):
            mk(x_lower=lo - 1.0, x_upper=hi + 1.0)
    for bad in (float("inf"), float("-inf"), float("nan")):
        hi = z(n) + 1.0
        hi[1] = bad
        with pytest.raises(ValueError, match="finite"):
            mk(x_lower=z(n) - 1.0, x_upper=hi)
        with pytest.raises(ValueError, match="finite"):
            mk(x_lower=-hi, x_upper=z(n) + 1.0)
    # positional callers are unaffected: the new arguments are the last two
    import inspect
    names = list(inspect.signature(AL_mpc.MPC.__init__).parameters)
    assert names[-2:] == ["x_lower", "x_upper"] and names[-3] == "dtype"
