"""Host-side checks of the block-tridiagonal NewtonAL entry points for caller-linearised dynamics
(csrc/dqp_al_banded.hip: dqp_al_banded_factor_bytes, dqp_al_banded_newton_step_jac) without a GPU.

The (n_state, n_ctrl) pairs with a Given<n, m> instantiation are read out of DQP_BAND_SIZES in the kernel source,
so that tests/test_gpu_al_given.py runs every pair the library is compiled for, a pair added later included."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BANDED_SRC = os.path.join(ROOT, "diff-qp-mpc_amd", "csrc", "dqp_al_banded.hip")
DQP_OK, DQP_ERR_BAD_ARG, DQP_ERR_TOO_LARGE = 0, -1, -2


def band_sizes():
    """[(n_state, n_ctrl)] of the DQP_BAND_SIZES X-macro, in source order"""
    src = open(BANDED_SRC).read()
    body = re.search(r"#define\s+DQP_BAND_SIZES((?:[^\n]*\\\n)*[^\n]*)", src).group(1)
    return [(int(a), int(b)) for a, b in re.findall(r"X\(\s*(\d+)\s*,\s*(\d+)\s*\)", body)]


def knot_doubles(n, m):
    """per knot: nt factor rows of (L row, 1 / diag, M row) = nt (nt + 1 + n) doubles"""
    nt = n + m
    return nt * (nt + 1 + n)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from diff_qp_mpc_amd import _lib
    return _lib.load()


def test_band_sizes_parsed():
    pairs = band_sizes()
    assert len(pairs) == 24, pairs
    assert len(set(pairs)) == len(pairs)
    assert all(1 <= n and 1 <= m and n + m <= 16 for n, m in pairs), pairs


def test_factor_bytes_for_exactly_the_listed_pairs(lib):
    from diff_qp_mpc_amd import _lib
    listed = set(band_sizes())
    for n in range(1, 17):
        for m in range(1, 17):
            for B, T in [(37, 11), (1, 2)]:
                d = _lib.dqp_al_mpc_dims(B, n, m, T)
                want = B * T * knot_doubles(n, m) * 8 if (n, m) in listed else 0
                assert lib.dqp_al_banded_factor_bytes(ctypes.byref(d), 0) == want, (n, m, B, T)


def test_factor_bytes_zero_below_two_knots_and_for_empty_batches(lib):
    from diff_qp_mpc_amd import _lib
    for n, m in band_sizes():
        for B, T in [(5, 1), (5, 0), (5, -3), (0, 6), (-1, 6)]:
            d = _lib.dqp_al_mpc_dims(B, n, m, T)
            assert lib.dqp_al_banded_factor_bytes(ctypes.byref(d), 0) == 0, (n, m, B, T)
    assert lib.dqp_al_banded_factor_bytes(None, 0) == 0


def _step_jac(lib, dims):
    z = ctypes.c_void_p(0)
    return lib.dqp_al_banded_newton_step_jac(ctypes.byref(dims), *([z] * 15))


def test_newton_step_jac_argument_validation(lib):
    """Unlisted pairs are refused as too large before any pointer is looked at; a horizon below two knots and
    empty state or control vectors are bad arguments; an empty batch is no launch."""
    from diff_qp_mpc_amd import _lib
    listed = set(band_sizes())
    for n, m in [(7, 2), (13, 3), (2, 3), (16, 1)]:
        assert (n, m) not in listed
        assert _step_jac(lib, _lib.dqp_al_mpc_dims(4, n, m, 6)) == DQP_ERR_TOO_LARGE, (n, m)
    for n, m, T in [(4, 1, 1), (0, 1, 6), (4, 0, 6), (12, 4, 1)]:
        assert _step_jac(lib, _lib.dqp_al_mpc_dims(4, n, m, T)) == DQP_ERR_BAD_ARG, (n, m, T)
    assert _step_jac(lib, _lib.dqp_al_mpc_dims(-1, 4, 1, 6)) == DQP_ERR_BAD_ARG
    for n, m in band_sizes():
        assert _step_jac(lib, _lib.dqp_al_mpc_dims(0, n, m, 6)) == DQP_OK, (n, m)
        assert _step_jac(lib, _lib.dqp_al_mpc_dims(4, n, m, 6)) == DQP_ERR_BAD_ARG, (n, m)    # null pointers
    assert lib.dqp_al_banded_newton_step_jac(None, *([ctypes.c_void_p(0)] * 15)) == DQP_ERR_BAD_ARG


def test_banded_solve_argument_validation(lib):
    """dqp_al_banded_solve(dims, 0, ...) reads the factor layout by sizes: unlisted pairs are refused."""
    from diff_qp_mpc_amd import _lib
    z = ctypes.c_void_p(0)
    d = _lib.dqp_al_mpc_dims(4, 4, 1, 1)
    assert lib.dqp_al_banded_solve(ctypes.byref(d), 0, z, z, z, None) == DQP_ERR_BAD_ARG
    d = _lib.dqp_al_mpc_dims(0, 7, 2, 6)
    assert lib.dqp_al_banded_solve(ctypes.byref(d), 0, z, z, z, None) == DQP_OK
    d = _lib.dqp_al_mpc_dims(4, 4, 1, 6)
    assert lib.dqp_al_banded_solve(ctypes.byref(d), 0, z, z, z, None) == DQP_ERR_BAD_ARG
