"""State bounds on the caller-linearised block-tridiagonal Newton step and in the merit kernel, without a GPU:
dqp_al_banded_newton_step_jac_xbounds and dqp_al_merit_xbounds are declared, exported and bound from the header; their
return-code tables (nothing is launched: nbatch 0, or null buffers); policies.Tracking_MPC hands a state box to its
AL_mpc.MPC; al_utils.banded_jac_supported with a state box."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

from test_al_banded_cpu import band_sizes
from test_al_banded_wide_cpu import band_wide_sizes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DQP_OK, DQP_ERR_BAD_ARG, DQP_ERR_TOO_LARGE = 0, -1, -2
NEWTON, MERIT = "dqp_al_banded_newton_step_jac_xbounds", "dqp_al_merit_xbounds"
# a narrow pair, a half-row pair, an LF pair (6 <= n + m <= 8) and the three wide pairs
PAIRS = [(12, 4), (3, 1), (6, 2), (13, 4), (14, 7), (24, 8)]
UNLISTED = [(7, 2), (13, 2), (16, 1)]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from diff_qp_mpc_amd import _lib
    return _lib.load()


def test_pairs_are_what_they_are_called():
    narrow, wide = band_sizes(), band_wide_sizes()
    assert PAIRS[0] in narrow and sum(PAIRS[0]) > 8
    assert PAIRS[1] in narrow and sum(PAIRS[1]) < 6
    assert PAIRS[2] in narrow and 6 <= sum(PAIRS[2]) <= 8
    assert sorted(PAIRS[3:]) == sorted(wide)
    assert not set(UNLISTED) & set(narrow + wide)


def test_declared_exported_and_bound(lib):
    from diff_qp_mpc_amd import _lib
    header = open(os.path.join(ROOT, "include", "dqp.h")).read()
    for s in (NEWTON, MERIT):
        assert s + "(" in header, s
        assert s in _lib.SYMBOLS and hasattr(lib, s), s
        restype, argtypes, names = _lib.PROTOTYPES[s]
        twin = _lib.PROTOTYPES[s.replace("_xbounds", "_bounds")][2]
        i = names.index("bounds")
        assert names[i + 1] == "xbounds" and argtypes[i] is argtypes[i + 1] is ctypes.POINTER(_lib.dqp_al_bounds), s
        assert names[:i + 1] + names[i + 2:] == twin and names[-1] == "stream", (names, twin)
    assert lib.dqp_version() == 303
    assert header.count("#define DQP_VERSION 303") == 1


def _newton(lib, d, bd, xbd):
    N = None
    return lib.dqp_al_banded_newton_step_jac_xbounds(ctypes.byref(d), N, N, N, N, N, N, bd, xbd, N, N, N, N, N, N, N)


def _merit(lib, d, bd, xbd, ncand=20):
    N = None
    return lib.dqp_al_merit_xbounds(ctypes.byref(d), ncand, N, N, N, N, N, N, N, bd, xbd, N, N)


def layouts(w, T):
    return ((0, 0), (0, w), (w, 0), (T * w, 0), (T * w, w))


def bad_strides(w, T):          # those of test_al_xbounds_cpu.test_return_code_table
    return ((w + 1, 0), (0, w + 1), (T * w, w + 1), (w, w), (T * w - 1, w), (-T * w, w), (0, -w))


def test_return_code_table(lib):
    from diff_qp_mpc_amd import _lib
    T = 6
    keep = np.zeros(T * 32)
    ptr = keep.ctypes.data
    r = ctypes.byref
    box = lambda sb=0, st=0, p=ptr: _lib.dqp_al_bounds(p, p, sb, st)
    for B in (0, 3):
        launched = DQP_OK if B == 0 else DQP_ERR_BAD_ARG           # null buffers behind the nbatch == 0 return
        for n, m in PAIRS + UNLISTED:
            d = _lib.dqp_al_mpc_dims(B, n, m, T)
            listed = (n, m) in PAIRS
            for call, want in ((_newton, launched if listed else DQP_ERR_TOO_LARGE), (_merit, launched)):
                where = (call.__name__, B, n, m)
                for usb, ust in layouts(m, T):          # every layout of the control box, at the wide pairs too
                    for xsb, xst in layouts(n, T):
                        assert call(lib, d, r(box(usb, ust)), r(box(xsb, xst))) == want, where + (usb, ust, xsb, xst)
                # null lower / upper of either box: behind the size rule and the nbatch == 0 return
                assert call(lib, d, r(box()), r(box(p=None))) == want, where
                assert call(lib, d, r(box(p=None)), r(box())) == want, where
                # a null box or illegal strides of either: in front of everything else
                assert call(lib, d, r(box()), None) == DQP_ERR_BAD_ARG, where
                assert call(lib, d, None, r(box())) == DQP_ERR_BAD_ARG, where
                for sb, st in bad_strides(n, T):
                    assert call(lib, d, r(box()), r(box(sb, st))) == DQP_ERR_BAD_ARG, where + (sb, st)
                for sb, st in bad_strides(m, T):
                    assert call(lib, d, r(box(sb, st)), r(box())) == DQP_ERR_BAD_ARG, where + (sb, st)
                if n != m and T * m != n and T * n != m:        # one box's strides in the other's place
                    assert call(lib, d, r(box()), r(box(T * m, m))) == DQP_ERR_BAD_ARG, where
                    assert call(lib, d, r(box(T * n, n)), r(box())) == DQP_ERR_BAD_ARG, where
        # sizes and horizon: bad arguments whatever else
        for n, m, Tb in ((0, 1, T), (2, 0, T), (2, 1, 1), (13, 4, 1), (7, 2, 1)):
            d = _lib.dqp_al_mpc_dims(B, n, m, Tb)
            assert _newton(lib, d, r(box()), r(box())) == DQP_ERR_BAD_ARG, (B, n, m, Tb)
            assert _merit(lib, d, r(box()), r(box())) == DQP_ERR_BAD_ARG, (B, n, m, Tb)
    d = _lib.dqp_al_mpc_dims(-1, 3, 1, T)
    assert _newton(lib, d, r(box()), r(box())) == DQP_ERR_BAD_ARG
    assert _merit(lib, d, r(box()), r(box())) == DQP_ERR_BAD_ARG
    N = None
    assert lib.dqp_al_banded_newton_step_jac_xbounds(N, N, N, N, N, N, N, r(box()), r(box()), N, N, N, N, N, N, N) == DQP_ERR_BAD_ARG
    assert lib.dqp_al_merit_xbounds(N, 20, N, N, N, N, N, N, N, r(box()), r(box()), N, N) == DQP_ERR_BAD_ARG
    # the merit entry: no candidates is no launch, a negative count a bad argument
    d = _lib.dqp_al_mpc_dims(3, 7, 2, T)
    assert _merit(lib, d, r(box()), r(box()), ncand=0) == DQP_OK
    assert _merit(lib, d, r(box()), r(box()), ncand=-1) == DQP_ERR_BAD_ARG


def test_twin_still_refuses_strided_control_bounds_at_wide_pairs(lib):
    """dqp_al_banded_newton_step_jac_bounds has no strided wide kernel: unchanged by the state-box entry"""
    from diff_qp_mpc_amd import _lib
    keep = np.zeros(8)
    N = None
    for n, m in band_wide_sizes():
        d = _lib.dqp_al_mpc_dims(0, n, m, 6)
        bd = _lib.dqp_al_bounds(keep.ctypes.data, keep.ctypes.data, 6 * m, m)
        rc = lib.dqp_al_banded_newton_step_jac_bounds(ctypes.byref(d), N, N, N, N, N, N, ctypes.byref(bd), N, N, N, N, N, N, N)
        assert rc == DQP_ERR_TOO_LARGE, (n, m)


def test_banded_jac_supported_with_a_state_box(lib):
    from diff_qp_mpc_amd import al_utils
    assert al_utils.banded_jac_supported(5, 13, 4, 6, strided=True, state_bounds=True)
    assert not al_utils.banded_jac_supported(5, 7, 2, 6, strided=True, state_bounds=True)
    assert not al_utils.banded_jac_supported(5, 7, 2, 6, state_bounds=True)
    assert al_utils.banded_jac_supported(5, 12, 4, 6, strided=True, state_bounds=True)
    # without a state box as before: the wide pairs take the vector form only
    assert al_utils.banded_jac_supported(5, 13, 4, 6) and not al_utils.banded_jac_supported(5, 13, 4, 6, strided=True)
    assert al_utils.banded_jac_supported(5, 13, 4, 6, state_bounds=True)


class _Env:
    """what Tracking_MPC reads of an env; `dynamics` is no registered model and is not evaluated here"""
    nx, nu, nq, dt = 5, 2, 3, 0.05
    action_space = types.SimpleNamespace(low=-np.ones(2), high=np.ones(2))

    @staticmethod
    def dynamics(x, u):
        raise AssertionError("not called")

    dynamics_derivatives = dynamics


def _args(solver):
    return types.SimpleNamespace(T=4, nq=3, device="cpu", dtype="double", qp_iter=1, eps=1e-5, warm_start=True, bsz=3,
                                 Q=None, R=None, solver_type=solver)


def test_tracking_mpc_forwards_the_state_box(monkeypatch):
    from diff_qp_mpc_amd import AL_mpc, policies
    monkeypatch.setattr(policies, "RECOGNISE_ENV_DYNAMICS", False)
    env, T, B = _Env(), 4, 3
    xl, xh = -torch.ones(B, T, env.nx, dtype=torch.float64), torch.ones(env.nx, dtype=torch.float64).expand(B, T, env.nx).clone()
    pol = policies.Tracking_MPC(_args("al"), env, x_lower=xl, x_upper=xh)
    assert isinstance(pol.ctrl, AL_mpc.MPC)
    assert torch.equal(pol.ctrl.x_lower, xl) and torch.equal(pol.ctrl.x_upper, xh)
    assert pol.ctrl.nineq == 2 * T * env.nu + 2 * T * env.nx
    assert pol.ctrl.lamda_prev.shape == (B, T * env.nx + pol.ctrl.nineq)
    free = policies.Tracking_MPC(_args("al"), env)
    assert free.ctrl.x_lower is None and free.ctrl.nineq == 2 * T * env.nu
    with pytest.raises(ValueError):     # both or neither (AL_mpc.MPC's own check)
        policies.Tracking_MPC(_args("al"), env, x_lower=xl)
    for kw in (dict(x_lower=xl, x_upper=xh), dict(x_lower=xl), dict(x_upper=xh)):
        with pytest.raises(ValueError, match="state bounds"):
            policies.Tracking_MPC(_args("ip"), env, **kw)
    import inspect
    assert list(inspect.signature(policies.Tracking_MPC.__init__).parameters) == ["self", "args", "env", "x_lower", "x_upper"]
