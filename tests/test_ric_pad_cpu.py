"""Host side of padded stage-wise MPC QPs (dqp_mpc_dims.n_state_host, csrc/dqp_ric_pad.hip): which host pair the
library names for every (n_state, n_ctrl), that n_state_host = 0 keeps every existing answer, the padded workspace
formula of include/dqp.h and the argument errors.  Needs only the built library."""
import ctypes

import pytest

from test_ric_wide_cpu import per_qp_doubles

NATIVE16 = [(12, 4), (3, 3), (3, 1), (4, 1), (6, 1), (2, 1), (4, 2), (5, 1), (8, 1), (2, 2), (3, 2), (6, 2), (8, 2),
            (6, 3), (4, 4), (8, 4), (10, 4), (12, 2)]
NATIVE_WIDE = [(13, 4), (14, 7), (24, 8)]
HOST16 = [(15, 1), (14, 2), (13, 3), (11, 5), (10, 6), (9, 7), (8, 8)]
HOST_WIDE = [(31, 1), (30, 2), (29, 3), (28, 4), (27, 5), (26, 6), (25, 7)]
COMPILED = set(NATIVE16 + NATIVE_WIDE + HOST16 + HOST_WIDE)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from diff_qp_mpc_amd import _lib
    return _lib.load()


def dims(B, n, m, T, dyn=0, host=0, bounds=1):
    from diff_qp_mpc_amd import _lib
    return ctypes.byref(_lib.dqp_mpc_dims(B, n, m, T, bounds, dyn, host))


def ev(x):
    return x + (x & 1)


def region_doubles(nh, m, T, B):
    """R of include/dqp.h: 2 (ev(T B nt'^2) + ev((T-1) B n' nt') + 2 ev(T B nt') + ev(T B n') + ev((T-1) B n') + ev(B n'))"""
    ntp = nh + m
    return 2 * (ev(T * B * ntp * ntp) + ev((T - 1) * B * nh * ntp) + 2 * ev(T * B * ntp) + ev(T * B * nh) +
                ev((T - 1) * B * nh) + ev(B * nh))


def batch_rounded(nh, m, B):
    q = 4 if nh + m <= 16 else 2
    return (B + q - 1) // q * q


def test_every_shape_up_to_32_has_the_minimal_host(lib):
    """Every n >= 1, 1 <= m <= 8, n + m <= 32 has a host, the smallest compiled n' >= n; none beyond."""
    for m in range(1, 11):
        for n in range(1, 34 - m):
            want = min([a for a, b in COMPILED if b == m and a >= n], default=0)
            got = lib.dqp_mpc_qp_host_n_state(dims(4, n, m, 10))
            assert got == want, (n, m, got, want)
            if m <= 8 and n + m <= 32:
                assert got >= n, (n, m)
    assert lib.dqp_mpc_qp_host_n_state(dims(4, 7, 1, 10)) == 8
    assert lib.dqp_mpc_qp_host_n_state(dims(4, 5, 3, 10)) == 6
    assert lib.dqp_mpc_qp_host_n_state(dims(4, 17, 3, 10)) == 29
    assert lib.dqp_mpc_qp_host_n_state(dims(4, 15, 8, 10)) == 24


def test_host_query_needs_bounds_and_no_model(lib):
    assert lib.dqp_mpc_qp_host_n_state(dims(4, 7, 1, 10, bounds=0)) == 0
    assert lib.dqp_mpc_qp_host_n_state(dims(4, 3, 1, 10, dyn=1)) == 0
    assert lib.dqp_mpc_qp_host_n_state(None) == 0


def test_build_parts_cover_the_host_list():
    from diff_qp_mpc_amd import _build
    parts = [p for part in _build.RIC_HOST_PARTS for p in part]
    assert sorted(parts) == sorted(HOST16 + HOST_WIDE) and len(parts) == len(set(parts))


@pytest.mark.parametrize("n,m,T,B", [(13, 4, 40, 5), (14, 7, 30, 1), (24, 8, 30, 8192), (12, 4, 30, 8192), (12, 4, 30, 5),
                                     (8, 4, 40, 3), (6, 1, 40, 9), (3, 1, 30, 1), (3, 3, 5, 7), (3, 3, 30, 7), (12, 4, 6, 6)])
def test_field_zero_keeps_every_answer(lib, n, m, T, B):
    """n_state_host = 0 at the pairs test_ric_wide_cpu and test_capi_cpu pin: the same supported / workspace answers."""
    from diff_qp_mpc_amd import _lib
    old = ctypes.byref(_lib.dqp_mpc_dims(B, n, m, T, 1, 0))
    new = dims(B, n, m, T, host=0)
    assert lib.dqp_mpc_qp_supported(new) == lib.dqp_mpc_qp_supported(old) == 1
    assert lib.dqp_mpc_qp_workspace_bytes(new) == lib.dqp_mpc_qp_workspace_bytes(old)
    assert lib.dqp_mpc_qp_stepped_workspace_bytes(new) == lib.dqp_mpc_qp_stepped_workspace_bytes(old)
    if T > 5:      # the stage-wise kernels (T 5 at (3, 3) is a null-space size)
        Bp = batch_rounded(n, m, B)
        assert lib.dqp_mpc_qp_workspace_bytes(new) == 8 * Bp * per_qp_doubles(n, m, T)
        assert lib.dqp_mpc_qp_stepped_workspace_bytes(new) == 8 * Bp * (per_qp_doubles(n, m, T) + 8)


@pytest.mark.parametrize("n,m", [(15, 4), (13, 5), (7, 1), (5, 3), (9, 8)])
def test_field_zero_keeps_unserved_shapes_unserved(lib, n, m):
    for T in (6, 30):
        assert lib.dqp_mpc_qp_supported(dims(4, n, m, T)) == 0
        assert lib.dqp_mpc_qp_workspace_bytes(dims(4, n, m, T)) == 0
        assert lib.dqp_mpc_qp_stepped_workspace_bytes(dims(4, n, m, T)) == 0


@pytest.mark.parametrize("n,nh,m,T,B", [(7, 8, 1, 30, 8192), (5, 6, 3, 70, 256), (17, 29, 3, 30, 1024), (3, 8, 1, 4, 37),
                                        (12, 28, 4, 6, 5), (13, 28, 4, 5, 1), (15, 15, 1, 12, 3), (8, 8, 8, 7, 2),
                                        (3, 3, 3, 5, 7)])
def test_padded_sizes_follow_the_formula(lib, n, nh, m, T, B):
    """Workspace 8 (Bp' W' + R) (stepped: Bp' (W' + 8)); the termination buffers are those of the host pair's snapshot.
    (3, 3) on itself at T 5 shows that the field bypasses the null-space route."""
    from diff_qp_mpc_amd import _lib
    d = dims(B, n, m, T, host=nh)
    assert lib.dqp_mpc_qp_supported(d) == 1
    Bp, W, R = batch_rounded(nh, m, B), per_qp_doubles(nh, m, T), region_doubles(nh, m, T, B)
    assert lib.dqp_mpc_qp_workspace_bytes(d) == 8 * (Bp * W + R)
    assert lib.dqp_mpc_qp_stepped_workspace_bytes(d) == 8 * (Bp * (W + 8) + R)
    opts = _lib.dqp_opts(1e-12, 1e-10, 20, 3, _lib.DQP_FLAG_BATCH_TERMINATION, 0)
    tb = lib.dqp_mpc_qp_termination_bytes(d, ctypes.byref(opts))
    assert tb > 0 and tb == lib.dqp_mpc_qp_stepped_termination_bytes(d, ctypes.byref(opts))
    if (nh, m) in NATIVE16 + NATIVE_WIDE and T > 5:
        assert tb == lib.dqp_mpc_qp_termination_bytes(dims(B, nh, m, T), ctypes.byref(opts))
    per = _lib.dqp_opts(1e-12, 1e-10, 20, 3, 0, 0)
    assert lib.dqp_mpc_qp_termination_bytes(d, ctypes.byref(per)) == 0


def test_padded_horizon_limit(lib):
    """The 32-bit byte-offset guard applies to the host pair's per-QP workspace."""
    T_bad = 0x7fffffff // (8 * 4 * per_qp_doubles(31, 1, 1)) + 1000
    assert per_qp_doubles(31, 1, T_bad) * 8 * 4 > 0x7fffffff
    assert lib.dqp_mpc_qp_supported(dims(2, 20, 1, T_bad, host=31)) == 0
    assert lib.dqp_mpc_qp_stepped_workspace_bytes(dims(2, 20, 1, T_bad, host=31)) == 0
    assert lib.dqp_mpc_qp_supported(dims(2, 20, 1, 200, host=31)) == 1


@pytest.mark.parametrize("n,m,nh,dyn", [(5, 3, 4, 0), (5, 3, 7, 0), (7, 1, 9, 0), (3, 1, 4, 5), (4, 1, 4, 2),
                                        (9, 8, 33, 0), (3, 1, -1, 0)])
def test_argument_errors(lib, n, m, nh, dyn):
    """n_state_host < n_state, an uncompiled (n_state_host, n_ctrl), a registered model with a host: size 0 from the
    queries, DQP_ERR_BAD_ARG from the entry points (an empty batch reaches no pointer and no GPU)."""
    from diff_qp_mpc_amd import _lib
    d = dims(4, n, m, 12, dyn=dyn, host=nh)
    assert lib.dqp_mpc_qp_supported(d) == 0
    assert lib.dqp_mpc_qp_workspace_bytes(d) == 0
    assert lib.dqp_mpc_qp_stepped_workspace_bytes(d) == 0
    opts = _lib.dqp_opts(1e-12, 1e-10, 20, 3, _lib.DQP_FLAG_BATCH_TERMINATION, 0)
    assert lib.dqp_mpc_qp_termination_bytes(d, ctypes.byref(opts)) == 0
    assert lib.dqp_mpc_qp_stepped_termination_bytes(d, ctypes.byref(opts)) == 0
    e = dims(0, n, m, 12, dyn=dyn, host=nh)
    z = [None] * 16
    assert lib.dqp_mpc_qp_forward(e, ctypes.byref(opts), *z) == -1
    assert lib.dqp_mpc_qp_backward(e, ctypes.byref(opts), *[None] * 15) == -1
    assert lib.dqp_mpc_qp_forward_stepped(e, ctypes.byref(opts), *[None] * 8, 0, 0, *[None] * 9) == -1
    # the same shape on its proper host, empty batch: accepted
    good = lib.dqp_mpc_qp_host_n_state(dims(4, n, m, 12))
    if dyn == 0 and good:
        ok = dims(0, n, m, 12, host=good)
        assert lib.dqp_mpc_qp_forward(ok, ctypes.byref(opts), *z) == 0
        assert lib.dqp_mpc_qp_forward_stepped(ok, ctypes.byref(opts), *[None] * 8, 0, 0, *[None] * 9) == 0
