"""Host side of dqp_qp_backward_shared / dqp_qp_backward_shared_bytes (include/dqp.h): exported, bound, and the
argument rules that are decided before anything touches a device."""
import ctypes
import itertools
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHED = (900, 30, 900, 30, 450, 15)          # strides of (Q, p, G, h, A, b) at (nz, nineq, neq) = (30, 30, 15)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from diff_qp_mpc_amd import _lib
    return _lib.load()


def dims(B, strides=BATCHED, shape=(30, 30, 15)):
    from diff_qp_mpc_amd import _lib
    return _lib.dqp_dims(B, *shape, *strides)


def scratch(lib, d):
    return int(lib.dqp_qp_backward_shared_bytes(ctypes.byref(d)))


def test_symbols_exported_bound_and_declared(lib):
    from diff_qp_mpc_amd import _lib
    src = open(os.path.join(ROOT, "include", "dqp.h")).read()
    for s in ("dqp_qp_backward_shared_bytes", "dqp_qp_backward_shared"):
        assert s in _lib.SYMBOLS
        assert hasattr(lib, s)
        assert re.search(r"\b%s\s*\(" % s, re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    assert lib.dqp_qp_backward_shared_bytes.restype is ctypes.c_size_t
    assert len(lib.dqp_qp_backward_shared.argtypes) == len(lib.dqp_qp_backward.argtypes) + 1
    assert lib.dqp_version() == 303                      # additive: no version bump


def test_scratch_bytes_is_a_host_function(lib):
    """0 with every stride non-zero, > 0 with any stride 0, non-decreasing in B, the formula of include/dqp.h."""
    from diff_qp_mpc_amd import _lib
    assert scratch(lib, dims(7)) == 0
    assert lib.dqp_qp_backward_shared_bytes(None) == 0
    for i in range(6):
        st = list(BATCHED)
        st[i] = 0
        assert scratch(lib, dims(7, st)) > 0, i
        prev = 0
        for B in (1, 2, 63, 64, 65, 128, 129, 4096):
            cur = scratch(lib, dims(B, st))
            assert cur >= prev and cur % 8 == 0, (i, B)
            prev = cur
    # neq == 0: A and b do not exist, their strides say nothing
    assert scratch(lib, dims(7, (144, 12, 96, 8, 0, 0), (12, 8, 0))) == 0
    K = _lib.SHARED_GRAD_KC
    t = lambda n: -(-n // 16)
    for (nz, nineq, neq), B in itertools.product([(30, 30, 15), (50, 37, 11), (500, 500, 0), (7, 5, 2)], (1, K, K + 1, 1000)):
        tiles = t(nz) * t(nz) + t(nz) + t(nineq) * t(nz) + t(nineq) + ((t(neq) * t(nz) + t(neq)) if neq else 0)
        want = 8 * (B * (nz + nineq + neq) + -(-B // K) * tiles * 256)
        assert scratch(lib, dims(B, (0,) * 6, (nz, nineq, neq))) == want, (nz, nineq, neq, B)


def test_argument_rules_without_gpu(lib):
    z = ctypes.c_void_p(0)
    one = ctypes.c_void_p(8)                              # never dereferenced on the host
    assert lib.dqp_qp_backward_shared(None, None, *([z] * 18)) == -1                      # NULL dims
    shared = dims(4, (0, 30, 0, 30, 0, 15))
    inputs = [one] * 8
    outs = [one] * 6
    # a shared parameter and no scratch
    assert lib.dqp_qp_backward_shared(ctypes.byref(shared), None, *inputs, *outs, z, z, z, z) == -1
    # empty batch: nothing to do, with or without scratch
    empty = dims(0, (0, 30, 0, 30, 0, 15))
    assert lib.dqp_qp_backward_shared(ctypes.byref(empty), None, *([z] * 18)) == 0
    assert lib.dqp_qp_backward_shared(ctypes.byref(dims(0)), None, *([z] * 18)) == 0
    # nothing shared: dqp_qp_backward's own rules (NULL inputs -> bad argument), scratch not needed
    assert lib.dqp_qp_backward_shared(ctypes.byref(dims(4)), None, *([z] * 18)) == -1
    bad = dims(4, (0,) * 6, (30, 0, 0))
    assert lib.dqp_qp_backward_shared(ctypes.byref(bad), None, *([z] * 18)) == -1         # nineq == 0
