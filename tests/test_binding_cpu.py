"""The ctypes binding is read from include/dqp.h (_lib.prototypes), and qp_wrapper.MPC decides its solver route in one
host-side function (MPC._route).  Needs only the built library: no test here touches a GPU."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from diff_qp_mpc_amd import _lib
    return _lib.load()


def declared():
    """{name: parameter text} by this file's own reading of the header"""
    src = open(os.path.join(ROOT, "include", "dqp.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return dict(re.findall(r"\b(dqp_[a-z_0-9]+)\s*\(([^)]*)\)", src))


def test_every_prototype_is_bound_with_its_parameter_count(lib):
    protos = declared()
    assert len(protos) >= 61
    for name, params in protos.items():
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is not None, name
        want = 0 if params.strip() == "void" else len(params.split(","))
        assert len(fn.argtypes) == want, (name, len(fn.argtypes), want)


def test_binding_types_follow_the_header(lib):
    from diff_qp_mpc_amd import _lib
    assert lib.dqp_error_string.restype is ctypes.c_char_p
    assert lib.dqp_workspace_bytes.restype is ctypes.c_size_t
    assert lib.dqp_mpc_qp_host_n_state.restype is ctypes.c_int32
    assert lib.dqp_qp_forward.argtypes[:3] == [ctypes.POINTER(_lib.dqp_dims), ctypes.POINTER(_lib.dqp_opts), ctypes.c_void_p]
    assert lib.dqp_mpc_assemble_bounds.argtypes[6] is ctypes.POINTER(_lib.dqp_al_bounds)      # a dqp_mpc_bounds *
    assert lib.dqp_mpc_line_search.argtypes[1:3] == [ctypes.c_int, ctypes.c_double]
    assert lib.dqp_trace_end.argtypes == [ctypes.POINTER(_lib.dqp_trace_record), ctypes.c_int32, ctypes.c_void_p]
    n, m = ctypes.c_int32(0), ctypes.c_int32(0)
    assert lib.dqp_dyn_sizes(6, ctypes.byref(n), ctypes.byref(m)) == 0 and (n.value, m.value) == (12, 4)


def test_a_miscounted_call_is_a_type_error(lib):
    from diff_qp_mpc_amd import _lib
    d = _lib.dqp_mpc_dims(0, 3, 3, 5, 1, 0)
    z = ctypes.c_void_p(0)
    assert lib.dqp_mpc_assemble(ctypes.byref(d), *([z] * 14)) == 0
    with pytest.raises(TypeError):
        lib.dqp_mpc_assemble(ctypes.byref(d), *([z] * 13))


def test_unknown_types_are_refused_by_name():
    from diff_qp_mpc_amd import _lib
    ok = "int dqp_fine(const dqp_dims *dims, double *x, int32_t n, void *stream);\n"
    p = _lib.prototypes(ok)
    assert p["dqp_fine"] == (ctypes.c_int, [ctypes.POINTER(_lib.dqp_dims), ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p],
                             ("dims", "x", "n", "stream"))
    for bad in ("int dqp_odd(const dqp_dims *dims, float scale, void *stream);\n",
                "int dqp_odd(uint64_t mask);\n", "float dqp_odd(int code);\n", "double *dqp_odd(int code);\n"):
        with pytest.raises(RuntimeError, match="dqp_odd"):
            _lib.prototypes(ok + bad)


def test_call_serves_only_entries_that_take_a_stream(lib):
    from diff_qp_mpc_amd import _lib
    with pytest.raises(RuntimeError, match="dqp_workspace_bytes"):
        _lib.call("dqp_workspace_bytes", "cuda:0", _lib.dqp_dims(1, 3, 2, 0, 0, 0, 0, 0, 0, 0))
    import torch
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.call("dqp_dyn_step", torch.device("cpu"), 2, 1, torch.zeros(1, 4, dtype=torch.float64), None, 0.05, None)


# ---------------------------------------------------------------------------------------------- MPC._route
class _Module:
    """a caller's dynamics module, as far as the route is concerned: anything that is not a LinDx or DeviceDynamics"""


def _mpc(n, m, T, B=4, dx="lin", bounds=True, **kw):
    from diff_qp_mpc_amd import qp_wrapper as qw
    from diff_qp_mpc_amd.dynamics import DeviceDynamics
    mpc = qw.MPC(n, m, T, u_lower=-1.0 if bounds else None, u_upper=1.0 if bounds else None, n_batch=B, **kw)
    dx = {"lin": qw.LinDx(None, None), "module": _Module()}.get(dx) or DeviceDynamics(dx)
    mpc.dx_true = dx
    return mpc, dx


@pytest.mark.parametrize("n,m,T,dx,kw,want", [
    (3, 3, 5, "lin", {}, ("fused", 0, False, False)),
    (3, 1, 14, "lin", {}, ("fused", 0, False, False)),            # the stage-wise kernels answer `supported`
    (7, 1, 10, "lin", {}, ("dense", 0, False, False)),
    (7, 1, 80, "lin", {}, ("padded", 8, False, False)),
    (5, 3, 6, "module", {}, ("stepped", 6, False, False)),
    (3, 1, 5, "pendulum_dx", {}, ("fused", 0, True, False)),
    (3, 1, 5, "lin", dict(add_goal_constraint=True), ("dense", 0, False, True)),
    (3, 1, 5, "lin", dict(add_goal_constraint=True, x_goal=[0.0, 0.0, 0.0]), ("dense", 0, False, True)),
    (3, 1, 5, "pendulum_dx", dict(add_goal_constraint=True), ("dense", 0, True, True)),
    (5, 3, 6, "module", dict(linearised_residual=True), ("dense", 0, False, False)),
    (3, 3, 5, "module", dict(linearised_residual=True), ("fused", 0, False, False)),
    (7, 1, 80, "module", dict(linearised_residual=True), ("padded", 8, False, False)),
    (3, 3, 5, "module", {}, ("stepped", 0, False, False)),
])
def test_route_table(lib, n, m, T, dx, kw, want):
    mpc, dx = _mpc(n, m, T, dx=dx, **kw)
    r = mpc._route(dx)
    assert (r.kind, r.n_state_host, r.model is not None, r.goal_rows) == want
    if r.model is not None:
        assert r.model is dx


@pytest.mark.parametrize("n,m,T,dx,bounds,kw,text", [
    (5, 3, 6, "module", False, {}, "caller-supplied dynamics module"),
    (5, 3, 6, "module", True, dict(add_goal_constraint=True), "caller-supplied dynamics module"),
    (30, 9, 6, "module", True, {}, "caller-supplied dynamics module"),          # n_ctrl > 8: no host pair
    (3, 1, 5, "lin", True, dict(add_goal_constraint=True, x_goal=[0.0, 1.0, 0.0]), "nonzero x_goal"),
])
def test_route_refusals(lib, n, m, T, dx, bounds, kw, text):
    mpc, dx = _mpc(n, m, T, dx=dx, bounds=bounds, **kw)
    with pytest.raises(NotImplementedError, match=text):
        mpc._route(dx)


def test_route_without_the_fused_entry_points(lib, monkeypatch):
    """FUSED_MPC_QP = False takes the shapes' own kernels out, nothing else: the padded route stays"""
    from diff_qp_mpc_amd import qp_wrapper as qw
    monkeypatch.setattr(qw, "FUSED_MPC_QP", False)
    mpc, dx = _mpc(3, 3, 5)
    assert mpc._route(dx).kind == "dense"
    mpc, dx = _mpc(7, 1, 80)
    assert mpc._route(dx) == qw.Route("padded", 8)
    mpc, dx = _mpc(3, 3, 5, bounds=False)
    assert mpc._route(dx).kind == "dense"
    mpc.dx_true = _Module()
    with pytest.raises(NotImplementedError, match="dx_true must be the LinDx"):
        mpc._route(dx)
