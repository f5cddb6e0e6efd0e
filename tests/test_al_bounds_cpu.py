"""Per-sample, per-knot control bounds (dqp_al_bounds) without a GPU: the header and the library have the struct and the
`_bounds` twins, the Python layout helper maps each accepted shape to its strides without expanding it, the host-side
queries answer, bad layouts are refused by every twin, and the numpy oracle -- the reference of the GPU tests in
test_gpu_al_bounds.py -- takes (B, T, m) bounds as it stands."""
import ctypes
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "BOUNDS_AL_pendulum_T5_b6.npz")

TWINS = ("dqp_al_merit", "dqp_al_banded_newton_step", "dqp_al_banded_newton_step_jac", "dqp_al_newton_solve",
         "dqp_al_outer_update", "dqp_al_mpc_solve", "dqp_al_mpc_solve_fused", "dqp_al_mpc_solve_fused_supported",
         "dqp_al_mpc_solve_fused_bytes")
DQP_ERR_BAD_ARG, DQP_ERR_TOO_LARGE = -1, -2


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from diff_qp_mpc_amd import _lib
    return _lib.load()


def test_header_library_and_binding(lib):
    from diff_qp_mpc_amd import _lib
    header = open(os.path.join(ROOT, "include", "dqp.h")).read()
    assert "typedef struct dqp_al_bounds {" in header and "} dqp_al_bounds;" in header
    for field in ("const double *lower, *upper;", "int64_t stride_b, stride_t;"):
        assert field in header
    for s in TWINS:
        assert s + "_bounds(" in header, s
        assert s + "(" in header                    # the old entry point stays declared
        assert s + "_bounds" in _lib.SYMBOLS
        assert hasattr(lib, s + "_bounds") and hasattr(lib, s)
    assert lib.dqp_version() == 303
    assert header.count("#define DQP_VERSION 303") == 1
    assert lib.dqp_error_string(DQP_ERR_BAD_ARG) is not None
    b = _lib.dqp_al_bounds(None, None, 10, 2)
    assert ctypes.sizeof(b) == 32 and (b.stride_b, b.stride_t) == (10, 2)


# ------------------------------------------------------------------ the Python layout helper
def test_layout_helper_strides_and_buffers():
    from diff_qp_mpc_amd import al_utils
    B, T, m = 6, 5, 2
    lo_v = -torch.arange(1.0, m + 1, dtype=torch.float64)
    cases = {"vector": (lo_v, (0, 0), m),
             "per_knot": (lo_v.expand(T, m).clone(), (0, m), T * m),
             "per_sample": (lo_v.expand(B, 1, m).clone(), (m, 0), B * m),
             "full": (lo_v.expand(B, T, m).clone(), (T * m, m), B * T * m)}
    for name, (lo, strides, numel) in cases.items():
        bd = al_utils.bounds_layout(lo, -lo, B, T, m)
        assert (bd.stride_b, bd.stride_t) == strides, name
        assert (bd.c.stride_b, bd.c.stride_t) == strides, name
        assert bd.lower.numel() == numel and bd.upper.numel() == numel, name       # nothing expanded
        assert bd.lower.dtype == torch.float64 and bd.lower.is_contiguous() and bd.upper.is_contiguous()
        assert bd.c.lower == bd.lower.data_ptr() and bd.c.upper == bd.upper.data_ptr()
        assert bd.lower.data_ptr() == lo.data_ptr()            # fp64 contiguous input: passed through, no copy
        assert al_utils.bounds_supported(lo, -lo, B, T, m)
        assert al_utils.bounds_strided(lo, m) == (name != "vector")
        # the index formula of include/dqp.h reproduces the broadcast the torch path does
        want = lo.expand(B, T, m) if name != "per_knot" else lo[None].expand(B, T, m)
        flat = bd.lower.reshape(-1)
        for b_, t_, k_ in ((0, 0, 0), (B - 1, T - 1, m - 1), (2, 3, 1)):
            assert flat[b_ * bd.stride_b + t_ * bd.stride_t + k_] == want[b_, t_, k_]
    # float32 and non-contiguous inputs are converted, still without expanding
    lo32 = cases["per_sample"][0].float()
    bd = al_utils.bounds_layout(lo32, -lo32, B, T, m)
    assert bd.lower.dtype == torch.float64 and bd.lower.numel() == B * m
    view = cases["full"][0].transpose(0, 1).contiguous().transpose(0, 1)              # (B, T, m), strides of (T, B, m)
    bd = al_utils.bounds_layout(view, -view, B, T, m)
    assert bd.lower.is_contiguous() and (bd.stride_b, bd.stride_t) == (T * m, m)
    # a requires-grad bound stays detached
    lo_g = cases["full"][0].clone().requires_grad_()
    assert not al_utils.bounds_layout(lo_g, -lo_g, B, T, m).lower.requires_grad


def test_layout_helper_rejects():
    from diff_qp_mpc_amd import al_utils
    B, T, m = 6, 5, 2
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    bad = [(z(B, T, m), z(T, m)),                 # lower / upper of different shapes
           (z(m), z(B, 1, m)),
           (z(T, B, m), z(T, B, m)),              # time-major
           (z(1, B, m), z(1, B, m)),
           (z(B, m), z(B, m)),                    # per-sample without its knot axis: ambiguous with (T, m) when B == T
           (z(B, T, m + 1), z(B, T, m + 1)),
           (z(B, T + 1, m), z(B, T + 1, m))]
    for lo, hi in bad:
        with pytest.raises(ValueError):
            al_utils.bounds_layout(lo, hi, B, T, m)
        assert not al_utils.bounds_supported(lo, hi, B, T, m)
    with pytest.raises(ValueError):
        al_utils.bounds_layout(None, None, B, T, m)


# ------------------------------------------------------------------ host-side queries
SIZES = {"pendulum1l": (2, 1), "cartpole1l": (4, 1), "cartpole2l": (6, 1), "pendulum_euler": (2, 1), "pendulum_dx": (3, 1),
         "integrator": (2, 1), "rexquadrotor": (12, 4)}


def layouts(T, m):
    return {"vector": (0, 0), "per_knot": (0, m), "per_sample": (m, 0), "per_sample_rows": (T * m, 0), "full": (T * m, m)}


@pytest.mark.parametrize("robot", sorted(SIZES))
def test_fused_queries_account_for_the_staged_bounds(robot, lib):
    """_supported_bounds / _bytes_bounds at every layout, and the launch's LDS: the strided instantiation stages the
    problem's 2 T n_ctrl bounds next to the problem (16 T n_ctrl bytes on top of the vector one's)."""
    from diff_qp_mpc_amd import _lib
    n, m = SIZES[robot]
    rid = _lib.DQP_DYN[robot]
    small = robot != "rexquadrotor"
    for T in (2, 5, 32, 33):
        d = _lib.dqp_al_mpc_dims(3, n, m, T)
        want = int(small and T <= 32)
        assert lib.dqp_al_mpc_solve_fused_supported(ctypes.byref(d), rid) == want
        vec = _lib.dqp_al_bounds(None, None, 0, 0)
        lds_vec = lib.dqp_al_mpc_solve_fused_lds_bytes(ctypes.byref(d), rid, ctypes.byref(vec))
        assert (lds_vec > 0) == bool(want) and lds_vec <= 64 * 1024
        for name, (sb, st) in layouts(T, m).items():
            bd = _lib.dqp_al_bounds(None, None, sb, st)
            assert lib.dqp_al_mpc_solve_fused_supported_bounds(ctypes.byref(d), rid, ctypes.byref(bd)) == want, name
            assert lib.dqp_al_mpc_solve_fused_bytes_bounds(ctypes.byref(d), ctypes.byref(bd)) == \
                lib.dqp_al_mpc_solve_fused_bytes(ctypes.byref(d)), name
            lds = lib.dqp_al_mpc_solve_fused_lds_bytes(ctypes.byref(d), rid, ctypes.byref(bd))
            if want:
                assert lds == lds_vec + (0 if name == "vector" else 2 * T * m * 8), name
                assert lds <= 64 * 1024
            else:
                assert lds == 0
        for sb, st in ((T * m + 1, 0), (0, m + 1), (T * m, m + 1), (m, m), (T * m + 1, m), (-m, 0)):
            bd = _lib.dqp_al_bounds(None, None, sb, st)
            assert lib.dqp_al_mpc_solve_fused_supported_bounds(ctypes.byref(d), rid, ctypes.byref(bd)) == 0
            assert lib.dqp_al_mpc_solve_fused_bytes_bounds(ctypes.byref(d), ctypes.byref(bd)) == 0
            assert lib.dqp_al_mpc_solve_fused_lds_bytes(ctypes.byref(d), rid, ctypes.byref(bd)) == 0
        assert lib.dqp_al_mpc_solve_fused_supported_bounds(ctypes.byref(d), rid, None) == 0


def _call_twins(lib, d, rid, bd, given=False, n_steps=4, banded=1, al_iter=2, newton_steps=4, n_prev=0, ncand=20):
    """every launching twin with null buffers -> {name: return code}; nothing is launched at nbatch == 0 or null buffers"""
    r = ctypes.byref
    N = None
    out = {
        "merit": lib.dqp_al_merit_bounds(r(d), ncand, N, N, N, N, N, N, N, bd, N, N),
        "newton_solve": lib.dqp_al_newton_solve_bounds(r(d), rid, 0.05, n_steps, banded, N, N, N, N, N, bd, N, N, N, N, N, N),
        "outer_update": lib.dqp_al_outer_update_bounds(r(d), rid, 0.05, N, N, N, N, N, N, bd, N, N, N, N),
        "mpc_solve": lib.dqp_al_mpc_solve_bounds(r(d), rid, 0.05, al_iter, newton_steps, N, N, N, N, N, bd, N, N, N, N, N,
                                                 n_prev, N, N, N, N, N, N, N, N, N, N),
        "mpc_solve_fused": lib.dqp_al_mpc_solve_fused_bounds(r(d), rid, 0.05, al_iter, newton_steps, N, N, N, N, N, bd, N, N,
                                                             N, N, N, n_prev, N, N, N, N, N, N, N, N, N, N),
        "banded_newton_step": lib.dqp_al_banded_newton_step_bounds(r(d), rid, 0.05, N, N, N, N, N, N, bd, N, N, N, N),
    }
    if given:
        out["banded_newton_step_jac"] = lib.dqp_al_banded_newton_step_jac_bounds(r(d), N, N, N, N, N, N, bd, N, N, N, N, N,
                                                                                 N, N)
    return out


def _call_legacy(lib, d, rid, n_steps=4, banded=1, al_iter=2, newton_steps=4, n_prev=0, ncand=20):
    """the same through the vector entry points (u_lower / u_upper null as every other buffer)"""
    r = ctypes.byref
    N = None
    return {
        "merit": lib.dqp_al_merit(r(d), ncand, N, N, N, N, N, N, N, N, N, N, N),
        "newton_solve": lib.dqp_al_newton_solve(r(d), rid, 0.05, n_steps, banded, N, N, N, N, N, N, N, N, N, N, N, N, N),
        "outer_update": lib.dqp_al_outer_update(r(d), rid, 0.05, N, N, N, N, N, N, N, N, N, N, N, N),
        "mpc_solve": lib.dqp_al_mpc_solve(r(d), rid, 0.05, al_iter, newton_steps, N, N, N, N, N, N, N, N, N, N, N, N, n_prev,
                                          N, N, N, N, N, N, N, N, N, N),
        "mpc_solve_fused": lib.dqp_al_mpc_solve_fused(r(d), rid, 0.05, al_iter, newton_steps, N, N, N, N, N, N, N, N, N, N, N,
                                                      N, n_prev, N, N, N, N, N, N, N, N, N, N),
        "banded_newton_step": lib.dqp_al_banded_newton_step(r(d), rid, 0.05, N, N, N, N, N, N, N, N, N, N, N, N),
        "banded_newton_step_jac": lib.dqp_al_banded_newton_step_jac(r(d), N, N, N, N, N, N, N, N, N, N, N, N, N, N, N),
    }


# Two faults at once, at the vector layout (0, 0) with every buffer null: which one an entry reports.  A row is
# (nbatch, (n_state, n_ctrl, T), model, scalar arguments, {entry: return code where it is not the row's default}); the
# default is DQP_OK at nbatch == 0 -- an empty batch returns in front of the model, the kernels' limits and the pointers --
# and DQP_ERR_BAD_ARG at nbatch == 3 (the null buffers, or the model in front of them).  The exceptions: the banded step
# checks its model in front of the nbatch == 0 return, the caller-linearised step its pair (DQP_ERR_TOO_LARGE); the scalar
# arguments are checked with the sizes, in front of everything.
UNREGISTERED, CARTPOLE1L, REXQUADROTOR = 99, 2, 6
PRECEDENCE_ROWS = [
    # an unregistered model id, at a compiled pair
    (0, (4, 1, 6), UNREGISTERED, {}, {"banded_newton_step": DQP_ERR_BAD_ARG}),
    (0, (4, 1, 6), 0, {}, {"banded_newton_step": DQP_ERR_BAD_ARG}),
    (3, (4, 1, 6), UNREGISTERED, {}, {}),
    (3, (4, 1, 6), 0, {}, {}),
    # sizes beyond the block-tridiagonal kernels (no registered model has them: the model check meets them first)
    (0, (13, 4, 6), REXQUADROTOR, {}, {"banded_newton_step": DQP_ERR_BAD_ARG}),
    (0, (16, 1, 6), REXQUADROTOR, {}, {"banded_newton_step": DQP_ERR_BAD_ARG, "banded_newton_step_jac": DQP_ERR_TOO_LARGE}),
    (0, (13, 4, 6), UNREGISTERED, {}, {"banded_newton_step": DQP_ERR_BAD_ARG}),
    (0, (16, 1, 6), UNREGISTERED, {}, {"banded_newton_step": DQP_ERR_BAD_ARG, "banded_newton_step_jac": DQP_ERR_TOO_LARGE}),
    (3, (13, 4, 6), REXQUADROTOR, {}, {}),
    (3, (16, 1, 6), REXQUADROTOR, {}, {"banded_newton_step_jac": DQP_ERR_TOO_LARGE}),
    (3, (13, 4, 6), UNREGISTERED, {}, {}),
    (3, (16, 1, 6), UNREGISTERED, {}, {"banded_newton_step_jac": DQP_ERR_TOO_LARGE}),
    # dqp_al_newton_solve_bounds with banded = 0: sizes beyond the dense kernel, T (n + m) > 128
    (0, (9, 1, 6), REXQUADROTOR, {"banded": 0}, {"banded_newton_step": DQP_ERR_BAD_ARG, "banded_newton_step_jac": DQP_ERR_TOO_LARGE}),
    (0, (4, 3, 6), CARTPOLE1L, {"banded": 0}, {"banded_newton_step": DQP_ERR_BAD_ARG, "banded_newton_step_jac": DQP_ERR_TOO_LARGE}),
    (0, (12, 4, 6), REXQUADROTOR, {"banded": 0}, {}),
    (0, (4, 1, 26), CARTPOLE1L, {"banded": 0}, {}),
    (3, (9, 1, 6), REXQUADROTOR, {"banded": 0}, {"banded_newton_step_jac": DQP_ERR_TOO_LARGE}),
    (3, (4, 3, 6), CARTPOLE1L, {"banded": 0}, {"banded_newton_step_jac": DQP_ERR_TOO_LARGE}),
    (3, (12, 4, 6), REXQUADROTOR, {"banded": 0}, {}),
    (3, (4, 1, 26), CARTPOLE1L, {"banded": 0}, {}),
    # scalar arguments: in front of the nbatch == 0 return
    (0, (4, 1, 6), CARTPOLE1L, {"n_steps": 0}, {"newton_solve": DQP_ERR_BAD_ARG}),
    (0, (4, 1, 6), CARTPOLE1L, {"n_steps": 0, "banded": 0}, {"newton_solve": DQP_ERR_BAD_ARG}),
    (0, (4, 1, 6), CARTPOLE1L, {"al_iter": 0}, {"mpc_solve": DQP_ERR_BAD_ARG, "mpc_solve_fused": DQP_ERR_BAD_ARG}),
    (0, (4, 1, 6), CARTPOLE1L, {"al_iter": 257}, {"mpc_solve": DQP_ERR_BAD_ARG, "mpc_solve_fused": DQP_ERR_BAD_ARG}),
    (0, (4, 1, 6), CARTPOLE1L, {"al_iter": 256}, {}),
    (0, (4, 1, 6), CARTPOLE1L, {"newton_steps": 0}, {"mpc_solve": DQP_ERR_BAD_ARG, "mpc_solve_fused": DQP_ERR_BAD_ARG}),
    (0, (4, 1, 6), CARTPOLE1L, {"n_prev": -1}, {"mpc_solve": DQP_ERR_BAD_ARG, "mpc_solve_fused": DQP_ERR_BAD_ARG}),
    (0, (4, 1, 6), CARTPOLE1L, {"ncand": -1}, {"merit": DQP_ERR_BAD_ARG}),
    # ... and in front of an unregistered model and of sizes beyond the kernels
    (0, (13, 4, 6), UNREGISTERED, {"n_steps": 0, "al_iter": 257, "ncand": -1},
     {"newton_solve": DQP_ERR_BAD_ARG, "mpc_solve": DQP_ERR_BAD_ARG, "mpc_solve_fused": DQP_ERR_BAD_ARG,
      "merit": DQP_ERR_BAD_ARG, "banded_newton_step": DQP_ERR_BAD_ARG}),
    (3, (4, 1, 6), CARTPOLE1L, {"n_steps": 0, "al_iter": 0, "n_prev": -1, "ncand": -1}, {}),
]


def _precedence_rows():
    """-> (row, dims, scalar arguments, {entry: expected code}) of PRECEDENCE_ROWS"""
    from diff_qp_mpc_amd import _lib
    names = ("merit", "newton_solve", "outer_update", "mpc_solve", "mpc_solve_fused", "banded_newton_step",
             "banded_newton_step_jac")
    for row in PRECEDENCE_ROWS:
        B, (n, m, T), rid, scalars, exceptions = row
        want = dict.fromkeys(names, 0 if B == 0 else DQP_ERR_BAD_ARG)
        want.update(exceptions)
        yield row, _lib.dqp_al_mpc_dims(B, n, m, T), rid, scalars, want


def test_every_twin_checks_the_layout(lib):
    """Strides outside the allowed set and a null struct are DQP_ERR_BAD_ARG in front of the nbatch == 0 return; a valid
    layout passes at nbatch == 0 (DQP_OK, nothing touched) and is refused with null buffers at nbatch > 0 -- the lower /
    upper pointers included -- as the existing CPU tests probe the other arguments."""
    from diff_qp_mpc_amd import _lib
    n, m, T = 4, 1, 6                         # cartpole1l; (4, 1) is a DQP_BAND_SIZES pair as well
    rid = _lib.DQP_DYN["cartpole1l"]
    keep = np.zeros(T * m)
    ptr = keep.ctypes.data
    for B in (0, 3):
        d = _lib.dqp_al_mpc_dims(B, n, m, T)
        for sb, st in ((m + 1, 0), (0, m + 1), (T * m, m + 1), (m, m), (T * m - 1, m), (-T * m, m), (0, -m)):
            bad = _lib.dqp_al_bounds(ptr, ptr, sb, st)
            for name, rc in _call_twins(lib, d, rid, ctypes.byref(bad), given=True).items():
                assert rc == DQP_ERR_BAD_ARG, (name, B, sb, st, rc)
        for name, rc in _call_twins(lib, d, rid, None, given=True).items():
            assert rc == DQP_ERR_BAD_ARG, (name, B, "null struct", rc)
        for sb, st in layouts(T, m).values():
            ok = _lib.dqp_al_bounds(ptr, ptr, sb, st)
            for name, rc in _call_twins(lib, d, rid, ctypes.byref(ok), given=True).items():
                assert rc == (0 if B == 0 else DQP_ERR_BAD_ARG), (name, B, sb, st, rc)     # B > 0: the null buffers
            nul = _lib.dqp_al_bounds(None, None, sb, st)
            for name, rc in _call_twins(lib, d, rid, ctypes.byref(nul), given=True).items():
                assert rc == (0 if B == 0 else DQP_ERR_BAD_ARG), (name, B, sb, st, rc)
    # two faults at once (PRECEDENCE_ROWS), at the vector layout with null lower / upper
    assert (_lib.DQP_DYN["cartpole1l"], _lib.DQP_DYN["rexquadrotor"]) == (CARTPOLE1L, REXQUADROTOR)
    assert UNREGISTERED not in _lib.DQP_DYN.values() and 0 not in _lib.DQP_DYN.values()
    vec = _lib.dqp_al_bounds(None, None, 0, 0)
    for row, d, rid, scalars, want in _precedence_rows():
        assert _call_twins(lib, d, rid, ctypes.byref(vec), given=True, **scalars) == want, row
    # the wide pairs (DQP_BAND_WIDE_SIZES) have the vector instantiation only: DQP_ERR_TOO_LARGE at non-zero strides
    d = _lib.dqp_al_mpc_dims(0, 13, 4, 6)
    N = None
    for (sb, st), want in (((0, 0), 0), ((6 * 4, 4), DQP_ERR_TOO_LARGE), ((0, 4), DQP_ERR_TOO_LARGE)):
        bd = _lib.dqp_al_bounds(ptr, ptr, sb, st)
        rc = lib.dqp_al_banded_newton_step_jac_bounds(ctypes.byref(d), N, N, N, N, N, N, ctypes.byref(bd), N, N, N, N, N, N, N)
        assert rc == want, (sb, st, rc)


def test_old_entry_points_keep_their_answers(lib):
    """The wrappers: what tests/test_capi_cpu.py-style probes of the vector entry points returned before."""
    from diff_qp_mpc_amd import _lib
    rid = _lib.DQP_DYN["cartpole1l"]
    N = None
    for B, want in ((0, 0), (3, DQP_ERR_BAD_ARG)):
        d = ctypes.byref(_lib.dqp_al_mpc_dims(B, 4, 1, 6))
        assert lib.dqp_al_merit(d, 20, N, N, N, N, N, N, N, N, N, N, N) == want
        assert lib.dqp_al_newton_solve(d, rid, 0.05, 4, 1, N, N, N, N, N, N, N, N, N, N, N, N, N) == want
        assert lib.dqp_al_outer_update(d, rid, 0.05, N, N, N, N, N, N, N, N, N, N, N, N) == want
        assert lib.dqp_al_banded_newton_step(d, rid, 0.05, N, N, N, N, N, N, N, N, N, N, N, N) == want
        assert lib.dqp_al_banded_newton_step_jac(d, N, N, N, N, N, N, N, N, N, N, N, N, N, N, N) == want
        assert lib.dqp_al_mpc_solve(d, rid, 0.05, 2, 4, N, N, N, N, N, N, N, N, N, N, N, N, 0, N, N, N, N, N, N, N, N, N,
                                    N) == want
        assert lib.dqp_al_mpc_solve_fused(d, rid, 0.05, 2, 4, N, N, N, N, N, N, N, N, N, N, N, N, 0, N, N, N, N, N, N, N, N,
                                          N, N) == want
    # every row of PRECEDENCE_ROWS: the answer of the `_bounds` twin at strides (0, 0)
    for row, d, rid, scalars, want in _precedence_rows():
        assert _call_legacy(lib, d, rid, **scalars) == want, row


# ------------------------------------------------------------------ the oracle under (B, T, m) bounds
def _pendulum_case(B=6, T=5, seed=3):
    rng = np.random.default_rng(seed)
    n, m = 2, 1
    x0 = np.stack([3.0 * (rng.random(B) - 0.5), rng.random(B) - 0.5], 1)
    Qd = np.broadcast_to(np.array([10.0, 1.0, 0.01]), (B, T, n + m)).copy()
    q = 0.1 * rng.standard_normal((B, T, n + m))
    u = 0.1 * rng.standard_normal((B, T, m))
    x = np.broadcast_to(x0[:, None], (B, T, n)).copy()
    return n, m, x, u, x0, Qd, q


def test_oracle_takes_expanded_bounds_bit_for_bit():
    """oracle/al_solve_oracle.al_solve and oracle/al_oracle.constraint_jacobian broadcast the bounds with numpy
    (al_solve_oracle.py:40, al_oracle.py:45): a vector expanded to (T, m), (B, 1, m) and (B, T, m) gives the vector's
    results to the last bit, so the GPU tests can hand them varying bounds unchanged."""
    from oracle import al_oracle, al_solve_oracle as aso
    n, m, x, u, x0, Qd, q = _pendulum_case()
    B, T = x.shape[:2]
    lo, hi = np.array([-0.6]), np.array([0.6])
    lam0, rho0 = np.zeros((B, T * n + 2 * T * m)), np.ones((B, 1))
    ref = aso.al_solve(x, u, x0, Qd, q, lo, hi, al_oracle.pendulum_step, lam0, rho0)
    assert (np.abs(ref["u"]) > 0.6 - 1e-3).any() and (np.abs(ref["u"]) < 0.5).any()        # bounds active and inactive
    jref = al_oracle.constraint_jacobian(ref["xu"], x0, lo, hi)
    for shape in ((T, m), (B, 1, m), (B, T, m)):
        lo_e, hi_e = np.broadcast_to(lo, shape).copy(), np.broadcast_to(hi, shape).copy()
        got = aso.al_solve(x, u, x0, Qd, q, lo_e, hi_e, al_oracle.pendulum_step, lam0, rho0)
        for k in ("xu", "lam", "rho", "L"):
            np.testing.assert_array_equal(got[k], ref[k], err_msg="%s %s" % (k, shape))
        for a, b in zip(got["history"], ref["history"]):
            for ai, bi in zip(a, b):
                np.testing.assert_array_equal(ai, bi)
        for a, b in zip(al_oracle.constraint_jacobian(ref["xu"], x0, lo_e, hi_e), jref):
            np.testing.assert_array_equal(a, b)


def test_oracle_reproduces_the_reference_golden():
    """BOUNDS_AL_pendulum_T5_b6.npz (tests/golden/make_golden_al_bounds.py: the reference's AL_mpc.MPC under (B, T, m)
    bounds, cold and warm call) against the oracle, at the tolerances of
    tests/test_oracle_golden.py::test_al_solve_oracle_matches_reference (:189-204): x, u rtol 1e-4 / atol 1e-5 (float32
    in the reference), multipliers rtol 1e-5 / atol 1e-5, rho exact, gradients rtol 1e-4 / atol 1e-6.  The golden meets
    the condition its generator asserts: two samples with a bound active at some knots and inactive at others, one
    sample with none active."""
    from oracle import al_oracle, al_solve_oracle as aso
    g = dict(np.load(GOLDEN, allow_pickle=False))
    B, T, nt = g["in_Qd"].shape
    n, m = 2, 1
    assert g["in_u_lower"].shape == (B, T, m) and g["in_u_upper"].shape == (B, T, m)
    assert float(g["dt"]) == al_oracle.DT
    gap = np.minimum(g["in_u_upper"] - g["u1"], g["u1"] - g["in_u_lower"]).min(axis=2)
    act, inact = gap <= 1e-3, gap >= 0.02
    assert (act.any(1) & inact.any(1)).sum() >= 2 and inact.all(1).sum() >= 1
    lam0, rho0 = np.zeros((B, T * n + 2 * T * m)), np.ones((B, 1))
    from oracle.al_solve_oracle import residuals  # noqa: F401  (the broadcasting line the docstring names)
    x_init = np.empty((B, T, n))
    x_init[:, 0] = g["in_x0"]
    for t in range(T - 1):                                     # AL_mpc.MPC.forward: the rollout of u_init
        x_init[:, t + 1] = al_oracle.pendulum_step(x_init[:, t], g["in_u_init"][:, t])[0]
    o1 = aso.al_solve(x_init, g["in_u_init"], g["in_x0"], g["in_Qd"], g["in_c"], g["in_u_lower"], g["in_u_upper"],
                      al_oracle.pendulum_step, lam0, rho0)
    np.testing.assert_allclose(o1["x"], g["x1"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(o1["u"], g["u1"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(o1["lam"], g["lam1"], rtol=1e-5, atol=1e-5)
    np.testing.assert_array_equal(o1["rho"], g["rho1"])
    gxu = np.concatenate((np.ones((B, T, n)), 2.0 * np.ones((B, T, m))), 2)
    dQ, dq = aso.backward(o1["L"], o1["xu"], gxu)
    np.testing.assert_allclose(dQ, g["dC1"], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(dq, g["dc1"], rtol=1e-4, atol=1e-6)
    o2 = aso.al_solve(g["x1"].astype(np.float64), g["u1"].astype(np.float64), g["in_x0"], g["in_Qd"], g["in_c"],
                      g["in_u_lower"], g["in_u_upper"], al_oracle.pendulum_step, o1["lam"], o1["rho"], history=o1["history"])
    np.testing.assert_allclose(o2["x"], g["x2"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(o2["u"], g["u2"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(o2["lam"], g["lam2"], rtol=1e-5, atol=1e-5)
    np.testing.assert_array_equal(o2["rho"], g["rho2"])
