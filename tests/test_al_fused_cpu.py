"""dqp_al_mpc_solve_fused without a GPU: the symbols are in the built library and in the ctypes binding, the size and
support queries answer on the host, and the Python switch is off by default."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FUSED = ("dqp_al_mpc_solve_fused_supported", "dqp_al_mpc_solve_fused_bytes", "dqp_al_mpc_solve_fused")
SIZES = {"pendulum1l": (2, 1), "cartpole1l": (4, 1), "cartpole2l": (6, 1), "pendulum_euler": (2, 1), "pendulum_dx": (3, 1),
         "rexquadrotor": (12, 4)}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from diff_qp_mpc_amd import _lib
    return _lib.load()


def test_symbols_in_library_and_binding(lib):
    from diff_qp_mpc_amd import _lib
    for s in FUSED:
        assert s in _lib.SYMBOLS
        assert hasattr(lib, s)          # ctypes resolves the name in the shared object
    assert lib.dqp_al_mpc_solve_fused.argtypes == lib.dqp_al_mpc_solve.argtypes
    header = open(os.path.join(ROOT, "include", "dqp.h")).read()
    for s in FUSED:
        assert s + "(" in header


@pytest.mark.parametrize("robot", sorted(SIZES))
def test_supported_and_bytes_answer_on_the_host(robot, lib):
    from diff_qp_mpc_amd import _lib
    n, m = SIZES[robot]
    small = robot != "rexquadrotor"
    for T, want in ((2, small), (5, small), (17, small), (32, small), (33, False), (1, False)):
        for B in (1, 3, 9, 128):
            d = _lib.dqp_al_mpc_dims(B, n, m, T)
            assert lib.dqp_al_mpc_solve_fused_supported(ctypes.byref(d), _lib.DQP_DYN[robot]) == int(want)
            assert lib.dqp_al_mpc_solve_fused_bytes(ctypes.byref(d)) == lib.dqp_al_mpc_solve_bytes(ctypes.byref(d))
            if T >= 2:
                assert lib.dqp_al_mpc_solve_fused_bytes(ctypes.byref(d)) > 0
    # sizes that do not belong to the model, an unknown model, a null dims
    d = _lib.dqp_al_mpc_dims(4, n + 1, m, 5)
    assert lib.dqp_al_mpc_solve_fused_supported(ctypes.byref(d), _lib.DQP_DYN[robot]) == 0
    d = _lib.dqp_al_mpc_dims(4, n, m, 5)
    assert lib.dqp_al_mpc_solve_fused_supported(ctypes.byref(d), 99) == 0
    assert lib.dqp_al_mpc_solve_fused_supported(None, _lib.DQP_DYN[robot]) == 0
    assert lib.dqp_al_mpc_solve_fused_bytes(None) == 0


def test_switch_is_off_by_default():
    from diff_qp_mpc_amd import AL_mpc
    assert AL_mpc.PERSISTENT_SOLVE is False
    assert isinstance(AL_mpc.PERSISTENT_SOLVE_MAX_BATCH, int) and AL_mpc.PERSISTENT_SOLVE_MAX_BATCH >= 0
