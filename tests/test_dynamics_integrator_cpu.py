"""The double integrator of deqmpc/envs.py:182-233 (the reference's `--env integrator`) in the device registry, without a
GPU: the binding and the library's host-side queries know the model, dynamics.NAMES stays the six names the existing
tests parametrise over, and the reference's golden (tests/golden/make_golden_integrator.py) has control bounds active on
some samples and inactive on others."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "INTEGRATOR_AL_b6.npz")
SIX = ("pendulum1l", "cartpole1l", "cartpole2l", "pendulum_euler", "pendulum_dx", "rexquadrotor")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from diff_qp_mpc_amd import _lib
    return _lib.load()


def test_device_dynamics_constructs(lib):
    from diff_qp_mpc_amd import _lib
    from diff_qp_mpc_amd.dynamics import DEFAULT_DT, DeviceDynamics
    dyn = DeviceDynamics("integrator")
    assert (dyn.id, dyn.n_state, dyn.n_ctrl, dyn.nx, dyn.nu, dyn.nq, dyn.dt) == (7, 2, 1, 2, 1, 1, 0.1)
    assert _lib.DQP_DYN["integrator"] == 7 and DEFAULT_DT["integrator"] == 0.1
    assert DeviceDynamics("integrator", dt=0.05).dt == 0.05
    with pytest.raises(ValueError, match="integrator"):          # the error message lists every registered model
        DeviceDynamics("acrobot")


def test_names_frozen_and_all_names():
    from diff_qp_mpc_amd import _lib, dynamics
    assert dynamics.NAMES == SIX
    assert dynamics.ALL_NAMES == SIX + ("integrator",)
    assert set(dynamics.ALL_NAMES) == set(_lib.DQP_DYN) == set(dynamics.DEFAULT_DT)


def test_header_registers_the_model(lib):
    src = open(os.path.join(ROOT, "include", "dqp.h")).read()
    ids = {k: int(v) for k, v in re.findall(r"(DQP_DYN_[A-Z0-9_]+)\s*=\s*(\d+)", src)}
    assert ids["DQP_DYN_INTEGRATOR"] == 7 and len(set(ids.values())) == len(ids) == 7
    assert "deqmpc/envs.py:182-233" in src
    assert lib.dqp_version() == 303
    n, m = ctypes.c_int32(0), ctypes.c_int32(0)
    assert lib.dqp_dyn_sizes(7, ctypes.byref(n), ctypes.byref(m)) == 0 and (n.value, m.value) == (2, 1)
    assert lib.dqp_dyn_sizes(8, None, None) == -1


def test_host_side_queries(lib):
    from diff_qp_mpc_amd import _lib
    for B in (1, 6, 256):
        for T, want in ((2, 1), (5, 1), (32, 1), (1, 0), (33, 0)):
            d = _lib.dqp_al_mpc_dims(B, 2, 1, T)
            assert lib.dqp_al_mpc_solve_fused_supported(ctypes.byref(d), 7) == want, (B, T)
        d = _lib.dqp_al_mpc_dims(B, 2, 1, 5)
        assert lib.dqp_al_banded_factor_bytes(ctypes.byref(d), 7) == B * 5 * 3 * (3 + 1 + 2) * 8
        # the true-dynamics residual of the stage-wise PDIPM
        assert lib.dqp_mpc_qp_supported(ctypes.byref(_lib.dqp_mpc_dims(B, 2, 1, 5, 1, 7))) == 1
    d = _lib.dqp_al_mpc_dims(4, 3, 1, 5)                           # sizes that are not the model's
    assert lib.dqp_al_mpc_solve_fused_supported(ctypes.byref(d), 7) == 0
    # the robots' extension interface stays the robots': the error pendulum_euler gets
    assert lib.dqp_dyn_forward_dynamics(7, 4, *([None] * 7)) == lib.dqp_dyn_forward_dynamics(4, 4, *([None] * 7)) == -1
    assert lib.dqp_dyn_forward_derivatives(7, 4, *([None] * 11)) == lib.dqp_dyn_forward_derivatives(4, 4, *([None] * 11)) == -1


def test_golden_has_active_and_inactive_bounds():
    g = dict(np.load(GOLDEN, allow_pickle=False))
    assert g["in_x0"].shape == (6, 2) and g["in_Qd"].shape == (6, 5, 3) and float(g["dt"]) == 0.1
    assert g["hist_cost1"].shape == (3, 6) and g["hist_lam1"].shape == (3, 6, 5 * 2 + 2 * 5) and g["hist_rho1"].shape == (3, 6)
    lo, hi = g["in_u_lower"], g["in_u_upper"]
    assert lo.tolist() == [-2.0] and hi.tolist() == [2.0]
    assert (np.abs(g["in_x0"]) <= 2.0).all()                      # inside env.reset()'s ranges
    for tag in ("u1", "u2"):
        gap = np.minimum(hi - g[tag].astype(np.float64), g[tag].astype(np.float64) - lo).min(axis=(1, 2))
        assert (gap <= 1e-3).sum() >= 2, (tag, gap)                # a control on (or, mid-solve, past) a bound
        assert (gap >= 0.1).sum() >= 2, (tag, gap)                 # every control well inside
