"""The device model registry (csrc/dqp_dyn_models.h: one list, dqp::dyn::visit, dqp::dyn::model_matches) seen from the
C ABI, without a GPU: every DQP_DYN_* of include/dqp.h is registered and bound, and every entry point that takes a model
id answers an unknown id, a registered id with sizes that are not its own, and each model's own sizes with the code it
always returned.  The calls pass nbatch = 0, or null pointers at nbatch = 3, so none of them launches.

The expected values are those of the library as it was before the registry was dispatched through one list (the commit
"qp_wrapper.MPC: run the SQP rounds of a registered model on the device"), recorded by running this file as a script
against that build: `python tests/test_dyn_registry_cpu.py` prints the two tables below for the library in use."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 5
UNKNOWN = (0, 8, -1)


def _lib_and_module():
    import __graft_entry__ as ge
    ge.build()
    from diff_qp_mpc_amd import _lib
    return _lib.load(), _lib


@pytest.fixture(scope="module")
def lib():
    return _lib_and_module()[0]


def header_ids():
    src = open(os.path.join(ROOT, "include", "dqp.h")).read()
    return {k: int(v) for k, v in re.findall(r"DQP_DYN_([A-Z0-9_]+)\s*=\s*(\d+)", src)}


# every entry point of include/dqp.h that takes a model: as an argument, in dqp_mpc_dims.dyn_id, or in dqp_opts.dyn_id
BY_ARGUMENT = ("dqp_dyn_sizes", "dqp_dyn_step", "dqp_dyn_jacobian", "dqp_dyn_forward_dynamics", "dqp_dyn_forward_derivatives",
               "dqp_mpc_line_search", "dqp_mpc_rollout_backward", "dqp_al_newton_solve", "dqp_al_newton_solve_bounds",
               "dqp_al_outer_update", "dqp_al_outer_update_bounds", "dqp_al_mpc_solve", "dqp_al_mpc_solve_bounds",
               "dqp_al_mpc_solve_fused_supported", "dqp_al_mpc_solve_fused_supported_bounds",
               "dqp_al_mpc_solve_fused_lds_bytes", "dqp_al_mpc_solve_fused", "dqp_al_mpc_solve_fused_bounds",
               "dqp_al_banded_factor_bytes", "dqp_al_banded_newton_step", "dqp_al_banded_newton_step_bounds",
               "dqp_al_banded_solve")
BY_MPC_DIMS = ("dqp_mpc_qp_supported", "dqp_mpc_qp_workspace_bytes", "dqp_mpc_qp_termination_bytes", "dqp_mpc_qp_forward",
               "dqp_mpc_qp_forward_bounds", "dqp_mpc_qp_backward", "dqp_mpc_qp_stepped_workspace_bytes",
               "dqp_mpc_qp_forward_stepped", "dqp_mpc_qp_forward_stepped_bounds", "dqp_mpc_linearize",
               "dqp_mpc_sqp_supported", "dqp_mpc_sqp_workspace_bytes", "dqp_mpc_sqp_rounds")
BY_OPTS = ("dqp_qp_forward", "dqp_qp_backward")
ENTRIES = BY_ARGUMENT + BY_MPC_DIMS + BY_OPTS
INTS = {"al_iter": 2, "newton_steps": 2, "n_steps": 2, "banded": 1, "max_iter": 3, "n_prev": 0, "it_begin": 0, "it_end": 2,
        "max_linesearch_iter": 3, "round_begin": 0, "round_end": 2}


def call(lib, mod, name, dyn, n, m, B):
    """the entry `name` for the model id `dyn` at sizes (n, m), horizon T and batch B, every pointer null"""
    _, argtypes, params = mod.PROTOTYPES[name]
    opts = mod.dqp_opts(1e-8, 1e-3, 10, 3, 0, 0, dyn if name in BY_OPTS else 0, T, 0.05, None)
    bounds = mod.dqp_al_bounds(None, None, 0, 0)
    args = []
    for p, t in zip(params, argtypes):
        if p == "dims":
            d = {mod.dqp_al_mpc_dims: lambda: mod.dqp_al_mpc_dims(B, n, m, T),
                 mod.dqp_mpc_dims: lambda: mod.dqp_mpc_dims(B, n, m, T, 1, dyn if name in BY_MPC_DIMS else 0),
                 mod.dqp_dims: lambda: mod.dqp_dims(B, T * (n + m), 2 * T * m, T * n, 0, 0, 0, 0, 0, 0)}[t._type_]()
            args.append(ctypes.byref(d))
        elif p == "opts":
            args.append(ctypes.byref(opts))
        elif p == "bounds":
            args.append(ctypes.byref(bounds))
        elif p in ("dyn_id", "id"):
            args.append(dyn)
        elif p == "n" and name.startswith("dqp_dyn_"):
            args.append(B)
        elif t is ctypes.c_double:
            args.append(0.5)
        elif t in (ctypes.c_int, ctypes.c_int32):
            args.append(INTS[p])
        else:
            assert t is ctypes.c_void_p, (name, p, t)
            args.append(None)
    return int(getattr(lib, name)(*args))


def sizes(lib):
    out = {}
    for k in sorted(header_ids().values()):
        n, m = ctypes.c_int32(0), ctypes.c_int32(0)
        assert lib.dqp_dyn_sizes(k, ctypes.byref(n), ctypes.byref(m)) == 0, k
        out[k] = (n.value, m.value)
    return out


def cases(lib):
    """(model id, n_state, n_ctrl): the unknown ids at a pendulum's sizes, then every registered id with a state more than
    its own, then every registered id at its own sizes"""
    own = sizes(lib)
    return ([(k, 2, 1) for k in UNKNOWN] + [(k, n + 1, m) for k, (n, m) in own.items()] +
            [(k, n, m) for k, (n, m) in own.items()])


def codes(lib, mod, name):
    return tuple(call(lib, mod, name, k, n, m, B) for B in (0, 3) for k, n, m in cases(lib))


QUERY_B, QUERY_T = (1, 6, 256), (1, 2, 5, 32, 33)


def queries(lib, mod, k, n, m):
    """the host-side queries of test_dynamics_integrator_cpu.py::test_host_side_queries for one model"""
    out = []
    for B in QUERY_B:
        for Tq in QUERY_T:
            d = mod.dqp_al_mpc_dims(B, n, m, Tq)
            out.append((lib.dqp_al_mpc_solve_fused_supported(ctypes.byref(d), k),
                        lib.dqp_al_banded_factor_bytes(ctypes.byref(d), k),
                        lib.dqp_mpc_qp_supported(ctypes.byref(mod.dqp_mpc_dims(B, n, m, Tq, 1, k)))))
    d = mod.dqp_al_mpc_dims(4, n + 1, m, 5)                        # sizes that are not the model's
    out.append((lib.dqp_al_mpc_solve_fused_supported(ctypes.byref(d), k), lib.dqp_al_banded_factor_bytes(ctypes.byref(d), k),
                lib.dqp_mpc_qp_supported(ctypes.byref(mod.dqp_mpc_dims(4, n + 1, m, 5, 1, k)))))
    return tuple(out)


# recorded (see the module docstring).  EXPECTED_CODES[entry]: one code per case of cases(), at nbatch = 0, then at nbatch = 3;
# EXPECTED_QUERIES[id]: (fused_supported, banded_factor_bytes, mpc_qp_supported) per (B, T) of QUERY_B x QUERY_T, then at
# sizes that are not the model's
EXPECTED_CODES = {
    'dqp_dyn_sizes': (-1, -1, -1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
        -1, -1, -1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0),
    'dqp_dyn_step': (-1, -1, -1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
        -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    'dqp_dyn_jacobian': (-1, -1, -1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
        -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    'dqp_dyn_forward_dynamics': (-1, -1, -1, 0, 0, 0, -1, -1, -1, -1, 0, 0, 0, -1, -1, -1, -1,
        -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    'dqp_dyn_forward_derivatives': (-1, -1, -1, 0, 0, 0, -1, -1, -1, -1, 0, 0, 0, -1, -1, -1, -1,
        -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    'dqp_mpc_line_search': (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
        -1, -1, -1, -1, -1, -1, -1, -1, -2, -1, -1, -1, -1, -1, -1, -1, -1),
    'dqp_mpc_rollout_backward': (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
        -1, -1, -1, -1, -1, -1, -1, -1, -2, -1, -1, -1, -1, -1, -1, -1, -1),
    'dqp_al_newton_solve': (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
        -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    'dqp_al_newton_solve_bounds': (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
        -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    'dqp_al_outer_update': (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
        -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    'dqp_al_outer_update_bounds': (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
        -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    'dqp_al_mpc_solve': (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
        -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    'dqp_al_mpc_solve_bounds': (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
        -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    'dqp_al_mpc_solve_fused_supported': (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 0, 1,
        0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 0, 1),
    'dqp_al_mpc_solve_fused_supported_bounds': (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 0, 1,
        0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 0, 1),
    'dqp_al_mpc_solve_fused_lds_bytes': (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 7176, 9576, 12936, 7176, 8256, 0, 7176,
        0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 7176, 9576, 12936, 7176, 8256, 0, 7176),
    'dqp_al_mpc_solve_fused': (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
        -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    'dqp_al_mpc_solve_fused_bounds': (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
        -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    'dqp_al_banded_factor_bytes': (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
        2160, 0, 0, 2160, 6000, 11760, 2160, 3840, 55680, 2160, 2160, 6000, 11760, 2160, 3840, 55680, 2160),
    'dqp_al_banded_newton_step': (-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, 0, 0, 0, 0, 0, 0, 0,
        -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    'dqp_al_banded_newton_step_bounds': (-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, 0, 0, 0, 0, 0, 0, 0,
        -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    'dqp_al_banded_solve': (0, -1, -1, -1, -1, -1, -1, -1, -1, -1, 0, 0, 0, 0, 0, 0, 0,
        -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    'dqp_mpc_qp_supported': (1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1,
        1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1),
    'dqp_mpc_qp_workspace_bytes': (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
        12744, 0, 0, 0, 0, 0, 0, 0, 0, 0, 6592, 11392, 17472, 6592, 8832, 60160, 6592),
    'dqp_mpc_qp_termination_bytes': (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
        0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0),
    'dqp_mpc_qp_forward': (0, -1, -1, -1, -1, -1, -1, -1, -1, -1, 0, 0, 0, 0, 0, 0, 0,
        -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    'dqp_mpc_qp_forward_bounds': (0, -1, -1, -1, -1, -1, -1, -1, -1, -1, 0, 0, 0, 0, 0, 0, 0,
        -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    'dqp_mpc_qp_backward': (0, -1, -1, -1, -1, -1, -1, -1, -1, -1, 0, 0, 0, 0, 0, 0, 0,
        -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    'dqp_mpc_qp_stepped_workspace_bytes': (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
        6848, 6848, 6848, 9088, 14528, 0, 9088, 11648, 66432, 9088, 6848, 11648, 17728, 6848, 9088, 60416, 6848),
    'dqp_mpc_qp_forward_stepped': (0, 0, 0, 0, 0, -2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
        -1, -1, -1, -1, -1, -2, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    'dqp_mpc_qp_forward_stepped_bounds': (0, 0, 0, 0, 0, -2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
        -1, -1, -1, -1, -1, -2, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    'dqp_mpc_linearize': (-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, 0, 0, 0, 0, 0, 0, 0,
        -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    'dqp_mpc_sqp_supported': (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1,
        0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1),
    'dqp_mpc_sqp_workspace_bytes': (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
        0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 9088, 16144, 25248, 9088, 12368, 87568, 9088),
    'dqp_mpc_sqp_rounds': (-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, 0, 0, 0, 0, 0, 0, 0,
        -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    'dqp_qp_forward': (0, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
        -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
    'dqp_qp_backward': (0, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
        -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1),
}
EXPECTED_QUERIES = {
    1: ((0, 0, 0), (1, 288, 1), (1, 720, 1), (1, 4608, 1), (0, 4752, 1), (0, 0, 0), (1, 1728, 1), (1, 4320, 1), (1,
        27648, 1), (0, 28512, 1), (0, 0, 0), (1, 73728, 1), (1, 184320, 1), (1, 1179648, 1), (0, 1216512, 1), (0, 2880,
        0)),
    2: ((0, 0, 0), (1, 800, 1), (1, 2000, 1), (1, 12800, 1), (0, 13200, 1), (0, 0, 0), (1, 4800, 1), (1, 12000, 1), (1,
        76800, 1), (0, 79200, 1), (0, 0, 0), (1, 204800, 1), (1, 512000, 1), (1, 3276800, 1), (0, 3379200, 1), (0, 8000,
        0)),
    3: ((0, 0, 0), (1, 1568, 1), (1, 3920, 1), (1, 25088, 1), (0, 25872, 1), (0, 0, 0), (1, 9408, 1), (1, 23520, 1), (1,
        150528, 1), (0, 155232, 1), (0, 0, 0), (1, 401408, 1), (1, 1003520, 1), (1, 6422528, 1), (0, 6623232, 1), (0,
        15680, 0)),
    4: ((0, 0, 0), (1, 288, 1), (1, 720, 1), (1, 4608, 1), (0, 4752, 1), (0, 0, 0), (1, 1728, 1), (1, 4320, 1), (1,
        27648, 1), (0, 28512, 1), (0, 0, 0), (1, 73728, 1), (1, 184320, 1), (1, 1179648, 1), (0, 1216512, 1), (0, 2880,
        0)),
    5: ((0, 0, 0), (1, 512, 1), (1, 1280, 1), (1, 8192, 1), (0, 8448, 1), (0, 0, 0), (1, 3072, 1), (1, 7680, 1), (1,
        49152, 1), (0, 50688, 1), (0, 0, 0), (1, 131072, 1), (1, 327680, 1), (1, 2097152, 1), (0, 2162688, 1), (0, 5120,
        0)),
    6: ((0, 0, 0), (0, 7424, 1), (0, 18560, 1), (0, 118784, 1), (0, 122496, 1), (0, 0, 0), (0, 44544, 1), (0, 111360,
        1), (0, 712704, 1), (0, 734976, 1), (0, 0, 0), (0, 1900544, 1), (0, 4751360, 1), (0, 30408704, 1), (0, 31358976,
        1), (0, 74240, 0)),
    7: ((0, 0, 0), (1, 288, 1), (1, 720, 1), (1, 4608, 1), (0, 4752, 1), (0, 0, 0), (1, 1728, 1), (1, 4320, 1), (1,
        27648, 1), (0, 28512, 1), (0, 0, 0), (1, 73728, 1), (1, 184320, 1), (1, 1179648, 1), (0, 1216512, 1), (0, 2880,
        0)),
}


def test_every_enum_entry_is_registered_and_bound(lib):
    from diff_qp_mpc_amd import _lib
    ids = header_ids()
    assert len(ids) == 7 and sorted(ids.values()) == list(range(1, 8))
    assert _lib.DQP_DYN == {k.lower(): v for k, v in ids.items()}
    assert sizes(lib) == {1: (2, 1), 2: (4, 1), 3: (6, 1), 4: (2, 1), 5: (3, 1), 6: (12, 4), 7: (2, 1)}
    for k in UNKNOWN:
        assert lib.dqp_dyn_sizes(k, None, None) == -1


def test_the_table_covers_every_entry_that_takes_a_model():
    from diff_qp_mpc_amd import _lib
    takes = {name for name, (_, _, params) in _lib.PROTOTYPES.items() if "dyn_id" in params or "id" in params}
    assert takes == set(BY_ARGUMENT)
    assert set(EXPECTED_CODES) == set(ENTRIES)


def test_an_enum_entry_the_library_rejects_fails_the_load(lib, monkeypatch):
    from diff_qp_mpc_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setitem(_lib.DQP_DYN, "acrobot", 8)
    with pytest.raises(RuntimeError, match="DQP_DYN_ACROBOT = 8"):
        _lib.load()


@pytest.mark.parametrize("name", ENTRIES)
def test_return_codes_are_the_recorded_ones(lib, name):
    from diff_qp_mpc_amd import _lib
    got = codes(lib, _lib, name)
    assert got == EXPECTED_CODES[name], list(zip(cases(lib) * 2, got, EXPECTED_CODES[name]))
    if _lib.PROTOTYPES[name][1][-1:] == [ctypes.c_void_p] and _lib.PROTOTYPES[name][2][-1] == "stream":
        half = len(got) // 2
        assert all(c < 0 and c != -3 for c in got[half:]), got[half:]       # null pointers at nbatch = 3: refused, not launched


@pytest.mark.parametrize("k", range(1, 8))
def test_host_side_queries_of_every_model(lib, k):
    from diff_qp_mpc_amd import _lib
    n, m = sizes(lib)[k]
    assert queries(lib, _lib, k, n, m) == EXPECTED_QUERIES[k]
    # the robots' extension interface stays the robots'
    want = 0 if k <= 3 else -1
    assert lib.dqp_dyn_forward_dynamics(k, 0, *([None] * 7)) == want
    assert lib.dqp_dyn_forward_derivatives(k, 0, *([None] * 11)) == want
    assert lib.dqp_dyn_forward_dynamics(k, 4, *([None] * 7)) == -1


if __name__ == "__main__":
    import sys
    sys.path.insert(0, ROOT)
    lib_, mod_ = _lib_and_module()
    print("EXPECTED_CODES = {")
    for name_ in ENTRIES:
        print("    %r: %r," % (name_, codes(lib_, mod_, name_)))
    print("}\nEXPECTED_QUERIES = {")
    for k_, (n_, m_) in sizes(lib_).items():
        print("    %d: %r," % (k_, queries(lib_, mod_, k_, n_, m_)))
    print("}")
