"""Host-side checks of the wide block-tridiagonal NewtonAL pairs (16 < n_state + n_ctrl <= 32: DQP_BAND_WIDE_SIZES in
csrc/dqp_al_banded.hip, instantiated in csrc/dqp_al_banded_wide.hip) and of dqp_al_banded_jac_factor_bytes, without a
GPU.  The narrow table (DQP_BAND_SIZES) and dqp_al_banded_factor_bytes(dims, 0) keep their meaning: the wide pairs are
in neither."""
import ctypes
import os
import re

import pytest

from test_al_banded_cpu import BANDED_SRC, ROOT, band_sizes, knot_doubles

DQP_OK, DQP_ERR_BAD_ARG, DQP_ERR_TOO_LARGE = 0, -1, -2
NARROW = [(1, 1), (2, 1), (3, 1), (4, 1), (5, 1), (6, 1), (7, 1), (8, 1), (2, 2), (3, 2), (4, 2), (5, 2), (6, 2), (8, 2),
          (10, 2), (12, 2), (3, 3), (6, 3), (9, 3), (4, 4), (6, 4), (8, 4), (10, 4), (12, 4)]
WIDE = [(13, 4), (14, 7), (24, 8)]
REFUSED = [(15, 4), (13, 5), (25, 8), (30, 4)]


def band_wide_sizes():
    """[(n_state, n_ctrl)] of the DQP_BAND_WIDE_SIZES X-macro, in source order"""
    src = open(BANDED_SRC).read()
    body = re.search(r"#define\s+DQP_BAND_WIDE_SIZES((?:[^\n]*\\\n)*[^\n]*)", src).group(1)
    return [(int(a), int(b)) for a, b in re.findall(r"X\(\s*(\d+)\s*,\s*(\d+)\s*\)", body)]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from diff_qp_mpc_amd import _lib
    return _lib.load()


def test_size_tables():
    wide = band_wide_sizes()
    assert sorted(wide) == WIDE, wide
    assert all(16 < n + m <= 32 for n, m in wide)
    assert band_sizes() == NARROW
    assert not set(wide) & set(band_sizes())


def test_jac_factor_bytes(lib):
    """narrow pairs: the value of dqp_al_banded_factor_bytes(dims, 0); wide pairs: 8 B T nt (nt + 1 + n); zero at every
    other pair of 1..32 x 1..16, below two knots, for empty batches and for null dims"""
    from diff_qp_mpc_amd import _lib
    f = lib.dqp_al_banded_jac_factor_bytes
    for n in range(1, 33):
        for m in range(1, 17):
            for B, T in [(37, 11), (1, 2)]:
                d = _lib.dqp_al_mpc_dims(B, n, m, T)
                got = f(ctypes.byref(d))
                if (n, m) in NARROW:
                    assert got == lib.dqp_al_banded_factor_bytes(ctypes.byref(d), 0) == 8 * B * T * knot_doubles(n, m), (n, m)
                elif (n, m) in WIDE:
                    assert got == 8 * B * T * (n + m) * (n + m + 1 + n), (n, m, B, T)
                else:
                    assert got == 0, (n, m, B, T)
    for n, m in NARROW + WIDE:
        for B, T in [(5, 1), (5, 0), (5, -3), (0, 6), (-1, 6)]:
            d = _lib.dqp_al_mpc_dims(B, n, m, T)
            assert f(ctypes.byref(d)) == 0, (n, m, B, T)
    assert f(None) == 0


def test_narrow_factor_bytes_stay_zero_at_the_wide_pairs(lib):
    from diff_qp_mpc_amd import _lib
    for n, m in WIDE:
        d = _lib.dqp_al_mpc_dims(37, n, m, 11)
        assert lib.dqp_al_banded_factor_bytes(ctypes.byref(d), 0) == 0, (n, m)


def _step_jac(lib, dims):
    z = ctypes.c_void_p(0)
    return lib.dqp_al_banded_newton_step_jac(ctypes.byref(dims), *([z] * 15))


def test_newton_step_jac_accepts_the_wide_pairs(lib):
    from diff_qp_mpc_amd import _lib
    for n, m in WIDE:
        assert _step_jac(lib, _lib.dqp_al_mpc_dims(0, n, m, 6)) == DQP_OK, (n, m)
        assert _step_jac(lib, _lib.dqp_al_mpc_dims(4, n, m, 6)) == DQP_ERR_BAD_ARG, (n, m)      # null pointers
        assert _step_jac(lib, _lib.dqp_al_mpc_dims(4, n, m, 1)) == DQP_ERR_BAD_ARG, (n, m)
    for n, m in REFUSED:
        assert _step_jac(lib, _lib.dqp_al_mpc_dims(4, n, m, 6)) == DQP_ERR_TOO_LARGE, (n, m)
        assert _step_jac(lib, _lib.dqp_al_mpc_dims(0, n, m, 6)) == DQP_ERR_TOO_LARGE, (n, m)


def test_banded_solve_accepts_the_wide_pairs(lib):
    from diff_qp_mpc_amd import _lib
    z = ctypes.c_void_p(0)
    solve = lambda d: lib.dqp_al_banded_solve(ctypes.byref(d), 0, z, z, z, None)
    for n, m in WIDE:
        assert solve(_lib.dqp_al_mpc_dims(0, n, m, 6)) == DQP_OK, (n, m)
        assert solve(_lib.dqp_al_mpc_dims(4, n, m, 6)) == DQP_ERR_BAD_ARG, (n, m)               # null pointers
        assert solve(_lib.dqp_al_mpc_dims(4, n, m, 1)) == DQP_ERR_BAD_ARG, (n, m)
    one = ctypes.c_void_p(8)        # non-null: an unlisted pair is refused before any pointer is used
    for n, m in REFUSED:
        d = _lib.dqp_al_mpc_dims(4, n, m, 6)
        assert lib.dqp_al_banded_solve(ctypes.byref(d), 0, one, one, one, None) == DQP_ERR_TOO_LARGE, (n, m)


def test_version_matches_header(lib):
    src = open(os.path.join(ROOT, "include", "dqp.h")).read()
    version = int(re.search(r"#define\s+DQP_VERSION\s+(\d+)", src).group(1))
    assert version == 303
    assert lib.dqp_version() == version
