"""Host side of the wide stage-wise MPC kernels (csrc/dqp_mpc_qp.hip, 16 < n_state + n_ctrl <= 32): which shapes
the library serves and the exact workspace sizes include/dqp.h documents.  Needs only the built library."""
import ctypes

import pytest

WIDE = [(13, 4), (14, 7), (24, 8)]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from diff_qp_mpc_amd import _lib
    return _lib.load()


def dims(B, n, m, T, dyn=0):
    from diff_qp_mpc_amd import _lib
    return ctypes.byref(_lib.dqp_mpc_dims(B, n, m, T, 1, dyn))


def per_qp_doubles(n, m, T):
    """W of include/dqp.h: ev(ev(ev(T (3 nt + 4 n + 14 m)) + T n^2) + T nt m + T (n + m))"""
    ev = lambda x: x + (x & 1)
    nt = n + m
    return ev(ev(ev(T * (3 * nt + 4 * n + 14 * m)) + T * n * n) + T * nt * m + T * (n + m))


@pytest.mark.parametrize("n,m,T", [(13, 4, 40), (14, 7, 30), (24, 8, 30)])
@pytest.mark.parametrize("B", [1, 3, 5, 8192])
def test_wide_pairs_supported_with_documented_workspace(lib, n, m, T, B):
    """Two QPs per wavefront: the batch is rounded up to even."""
    assert lib.dqp_mpc_qp_supported(dims(B, n, m, T)) == 1
    Bp = (B + 1) // 2 * 2
    assert lib.dqp_mpc_qp_workspace_bytes(dims(B, n, m, T)) == 8 * Bp * per_qp_doubles(n, m, T)
    assert lib.dqp_mpc_qp_stepped_workspace_bytes(dims(B, n, m, T)) == 8 * Bp * (per_qp_doubles(n, m, T) + 8)


def test_wide_termination_buffer_sized(lib):
    from diff_qp_mpc_amd import _lib
    opts = _lib.dqp_opts(1e-12, 1e-10, 20, 3, _lib.DQP_FLAG_BATCH_TERMINATION, 0)
    for n, m in WIDE:
        assert lib.dqp_mpc_qp_termination_bytes(dims(5, n, m, 30), ctypes.byref(opts)) > 0
        assert lib.dqp_mpc_qp_stepped_termination_bytes(dims(5, n, m, 30), ctypes.byref(opts)) > 0


@pytest.mark.parametrize("n,m,dyn", [(15, 4, 0), (13, 5, 0), (30, 4, 0), (28, 8, 0), (13, 4, 6), (24, 8, 1)])
def test_other_shapes_stay_unsupported(lib, n, m, dyn):
    """Uncompiled wide pairs, knots above 32 and a device model (dyn_id) on a wide pair (no registered model is that
    wide) are refused, workspace 0."""
    for T in (6, 30):
        assert lib.dqp_mpc_qp_supported(dims(4, n, m, T, dyn)) == 0
        assert lib.dqp_mpc_qp_workspace_bytes(dims(4, n, m, T, dyn)) == 0
        if dyn == 0:
            assert lib.dqp_mpc_qp_stepped_workspace_bytes(dims(4, n, m, T)) == 0


def test_wide_horizon_limit(lib):
    """The 32-bit byte-offset guard of the stage-wise kernels applies to the wide pairs unchanged."""
    W = per_qp_doubles(24, 8, 1)
    T_bad = 0x7fffffff // (8 * 4 * W) + 10
    assert lib.dqp_mpc_qp_supported(dims(8, 24, 8, T_bad)) == 0
    assert lib.dqp_mpc_qp_stepped_workspace_bytes(dims(8, 24, 8, T_bad)) == 0
    assert lib.dqp_mpc_qp_supported(dims(8, 24, 8, 2000)) == 1


@pytest.mark.parametrize("n,m,T,B", [(12, 4, 30, 8192), (12, 4, 30, 5), (8, 4, 40, 3), (6, 1, 40, 9), (3, 1, 30, 1)])
def test_sixteen_lane_pairs_keep_their_sizes(lib, n, m, T, B):
    """Pairs with n + m <= 16 keep four QPs per wavefront (batch rounded to a multiple of four)."""
    Bp = (B + 3) // 4 * 4
    assert lib.dqp_mpc_qp_workspace_bytes(dims(B, n, m, T)) == 8 * Bp * per_qp_doubles(n, m, T)
    assert lib.dqp_mpc_qp_stepped_workspace_bytes(dims(B, n, m, T)) == 8 * Bp * (per_qp_doubles(n, m, T) + 8)
    # BASELINE config 4, recorded before the wide kernels existed
    if (n, m, T, B) == (12, 4, 30, 8192):
        assert lib.dqp_mpc_qp_workspace_bytes(dims(B, n, m, T)) == 739246080
