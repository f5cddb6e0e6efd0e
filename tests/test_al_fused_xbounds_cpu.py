"""State bounds on the single-launch AL_mpc solve (dqp_al_mpc_solve_fused_xbounds, csrc/dqp_al_fused.hip) without a GPU:
the header, the library and the binding have the four entries; the host-side queries (`_supported_xbounds`,
`_lds_bytes_xbounds`, `_bytes_xbounds`) answer; al_utils.fused_solve_supported takes `state_bounds`."""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = {"pendulum1l": (2, 1), "cartpole1l": (4, 1), "cartpole2l": (6, 1), "pendulum_euler": (2, 1), "pendulum_dx": (3, 1),
         "integrator": (2, 1), "rexquadrotor": (12, 4)}
SMALL = [k for k, (n, m) in SIZES.items() if n + m <= 8]
# name -> number of parameters
ENTRIES = {"dqp_al_mpc_solve_fused_supported_xbounds": 4, "dqp_al_mpc_solve_fused_bytes_xbounds": 1,
           "dqp_al_mpc_solve_fused_lds_bytes_xbounds": 4, "dqp_al_mpc_solve_fused_xbounds": 28}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from diff_qp_mpc_amd import _lib
    return _lib.load()


def boxes(_lib, n, m, T, ctrl=(0, 0), state=(0, 0)):
    return _lib.dqp_al_bounds(None, None, *ctrl), _lib.dqp_al_bounds(None, None, *state)


def test_declared_exported_and_bound(lib):
    from diff_qp_mpc_amd import _lib
    header = open(os.path.join(ROOT, "include", "dqp.h")).read()
    for s, nparam in ENTRIES.items():
        assert s + "(" in header, s
        assert s in _lib.SYMBOLS and hasattr(lib, s), s
        restype, argtypes, names = _lib.PROTOTYPES[s]
        assert len(argtypes) == len(names) == nparam, (s, names)
        assert getattr(lib, s).argtypes == argtypes
    names = _lib.PROTOTYPES["dqp_al_mpc_solve_fused_xbounds"][2]
    assert names == _lib.PROTOTYPES["dqp_al_mpc_solve_xbounds"][2] and names[-1] == "stream"
    for s in ("dqp_al_mpc_solve_fused_supported_xbounds", "dqp_al_mpc_solve_fused_lds_bytes_xbounds"):
        restype, argtypes, names = _lib.PROTOTYPES[s]
        assert names[2:] == ("bounds", "xbounds") and argtypes[2] is argtypes[3] is ctypes.POINTER(_lib.dqp_al_bounds)
    assert _lib.PROTOTYPES["dqp_al_mpc_solve_fused_lds_bytes_xbounds"][0] is ctypes.c_size_t
    assert lib.dqp_version() == 303


def test_supported_answers_on_the_host(lib):
    from diff_qp_mpc_amd import _lib
    r = ctypes.byref
    sup = lib.dqp_al_mpc_solve_fused_supported_xbounds
    for robot, (n, m) in SIZES.items():
        rid = _lib.DQP_DYN[robot]
        for T in (2, 32):
            d = _lib.dqp_al_mpc_dims(3, n, m, T)
            for ctrl in ((0, 0), (T * m, m)):
                for state in ((0, 0), (0, n), (n, 0), (T * n, 0), (T * n, n)):
                    bd, xbd = boxes(_lib, n, m, T, ctrl, state)
                    assert sup(r(d), rid, r(bd), r(xbd)) == (1 if robot in SMALL else 0), (robot, T, ctrl, state)
        for T in (1, 33):
            bd, xbd = boxes(_lib, n, m, T)
            assert sup(r(_lib.dqp_al_mpc_dims(3, n, m, T)), rid, r(bd), r(xbd)) == 0, (robot, T)
        # a state box or a control box whose strides are no layout; a null one; a model whose sizes are not the dims'
        T = 5
        d = _lib.dqp_al_mpc_dims(3, n, m, T)
        ok_u, ok_x = boxes(_lib, n, m, T)
        for sb, st in ((n + 1, 0), (0, n + 1), (T * n, n + 1), (n, n), (T * n - 1, n), (-T * n, n), (0, -n)):
            assert sup(r(d), rid, r(ok_u), r(_lib.dqp_al_bounds(None, None, sb, st))) == 0, (robot, sb, st)
        assert sup(r(d), rid, r(_lib.dqp_al_bounds(None, None, 0, m + 1)), r(ok_x)) == 0
        assert sup(r(d), rid, r(ok_u), None) == 0 and sup(r(d), rid, None, r(ok_x)) == 0
        assert sup(r(d), 0, r(ok_u), r(ok_x)) == 0 and sup(r(d), 99, r(ok_u), r(ok_x)) == 0
        other = next(k for k, v in SIZES.items() if v != (n, m))
        assert sup(r(d), _lib.DQP_DYN[other], r(ok_u), r(ok_x)) == 0
    bd, xbd = boxes(_lib, 2, 1, 5)
    assert sup(None, 1, r(bd), r(xbd)) == 0
    assert sup(r(_lib.dqp_al_mpc_dims(-1, 2, 1, 5)), 1, r(bd), r(xbd)) == 0


def test_lds_and_workspace_bytes(lib):
    """The launch's LDS stays within the 64 KB a launch gets without opt-in, and is that of the call with a strided control
    box plus the 2 T n state rows of lam and the 2 T n staged state bounds; 0 where the entry does not exist."""
    from diff_qp_mpc_amd import _lib
    r = ctypes.byref
    lds_x, lds_u = lib.dqp_al_mpc_solve_fused_lds_bytes_xbounds, lib.dqp_al_mpc_solve_fused_lds_bytes
    for robot, (n, m) in SIZES.items():
        rid = _lib.DQP_DYN[robot]
        for T in (2, 5, 17, 32):
            d = _lib.dqp_al_mpc_dims(3, n, m, T)
            strided = _lib.dqp_al_bounds(None, None, T * m, m)
            for ctrl in ((0, 0), (T * m, m)):
                for state in ((0, 0), (T * n, n)):
                    bd, xbd = boxes(_lib, n, m, T, ctrl, state)
                    got = int(lds_x(r(d), rid, r(bd), r(xbd)))
                    if robot not in SMALL:
                        assert got == 0
                        continue
                    assert 0 < got <= 65536, (robot, T, got)
                    assert got == int(lds_u(r(d), rid, r(strided))) + 4 * T * n * 8, (robot, T, ctrl, state)
            assert int(lib.dqp_al_mpc_solve_fused_bytes_xbounds(r(d))) == int(lib.dqp_al_mpc_solve_xbounds_bytes(r(d))) > 0
        d = _lib.dqp_al_mpc_dims(3, n, m, 33)
        bd, xbd = boxes(_lib, n, m, 33)
        assert int(lds_x(r(d), rid, r(bd), r(xbd))) == 0
    # the largest carve: cartpole-2 at T = 32
    d = _lib.dqp_al_mpc_dims(3, 6, 1, 32)
    bd, xbd = boxes(_lib, 6, 1, 32)
    assert int(lds_x(r(d), _lib.DQP_DYN["cartpole2l"], r(bd), r(xbd))) == 6912 * 8 + 5120


def test_entry_return_codes_without_a_launch(lib):
    """with null buffers nothing is launched: the order of the checks of the `_xbounds` entries, then the kernel's limits"""
    from diff_qp_mpc_amd import _lib
    r = ctypes.byref
    keep = np.zeros(64)

    def call(robot, T, B, bd, xbd, al_iter=2, newton_steps=4, n_prev=0, rid=None, N=None):
        n, m = SIZES[robot]
        d = _lib.dqp_al_mpc_dims(B, n, m, T)
        return lib.dqp_al_mpc_solve_fused_xbounds(r(d), _lib.DQP_DYN[robot] if rid is None else rid, 0.05, al_iter, newton_steps,
                                                  N, N, N, N, N, bd, xbd, N, N, N, N, N, n_prev, N, N, N, N, N, N, N, N, N, None)

    for robot in SIZES:
        n, m = SIZES[robot]
        bd, xbd = boxes(_lib, n, m, 5)
        small = robot in SMALL
        assert call(robot, 5, 0, r(bd), r(xbd)) == 0                      # nbatch == 0: DQP_OK in front of the limits
        assert call(robot, 33, 0, r(bd), r(xbd)) == 0
        assert call(robot, 5, 3, r(bd), r(xbd)) == -1                     # null buffers
        assert call(robot, 5, -1, r(bd), r(xbd)) == -1
        assert call(robot, 1, 0, r(bd), r(xbd)) == -1
        assert call(robot, 5, 0, r(bd), None) == -1 and call(robot, 5, 0, None, r(xbd)) == -1
        assert call(robot, 5, 0, r(bd), r(_lib.dqp_al_bounds(None, None, n + 1, 0))) == -1
        for kw in (dict(al_iter=257), dict(al_iter=0), dict(newton_steps=0), dict(n_prev=-1)):
            assert call(robot, 5, 0, r(bd), r(xbd), **kw) == -1, (robot, kw)
        assert call(robot, 5, 0, r(bd), r(xbd), rid=99) == -1
        # every buffer set (host memory: the limits are checked in front of the launch): the kernel's limits
        ptr = keep.ctypes.data
        full_u, full_x = _lib.dqp_al_bounds(ptr, ptr, 0, 0), _lib.dqp_al_bounds(ptr, ptr, 0, 0)
        assert call(robot, 33, 3, r(full_u), r(full_x), N=ptr) == -2
        if not small:
            assert call(robot, 5, 3, r(full_u), r(full_x), N=ptr) == -2
        assert call(robot, 5, 3, r(full_u), r(xbd), N=ptr) == -1          # null lower / upper of the state box


def test_fused_solve_supported_with_state_bounds(lib):
    from diff_qp_mpc_amd import al_utils

    class Dyn:
        def __init__(self, robot):
            from diff_qp_mpc_amd import _lib
            self.id, (self.n_state, self.n_ctrl) = _lib.DQP_DYN[robot], SIZES[robot]

    assert al_utils.fused_solve_supported(128, Dyn("cartpole2l"), 5, False, True) is True
    for robot in SIZES:
        for strided in (False, True):
            for T in (2, 32, 33):
                want = robot in SMALL and T <= 32
                assert al_utils.fused_solve_supported(4, Dyn(robot), T, strided, state_bounds=True) is want, (robot, T)
                assert al_utils.fused_solve_supported(4, Dyn(robot), T, strided) is want
