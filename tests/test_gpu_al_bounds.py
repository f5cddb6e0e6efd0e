"""Per-sample, per-knot control bounds (include/dqp.h: dqp_al_bounds) on the device AL_mpc paths.

 1. layout equivalence, bit for bit: a vector bound expanded to (T, m), (B, 1, m) and (B, T, m) through every `_bounds`
    twin and through AL_mpc.MPC gives the bytes of the vector entry point, on the same launch list
 2. truly varying bounds against the numpy oracle (oracle/al_solve_oracle.py, oracle/al_oracle.py): AL_mpc.MPC cold and
    warm, one Newton step, the merit, the outer update -- on inputs for which ignoring the strides cannot pass
 3. backward under varying bounds against the project's general torch path
 4. the reference's golden (tests/golden/make_golden_al_bounds.py) through AL_mpc.MPC, PERSISTENT_SOLVE off and on
 5. hipGraph capture and replay of one call with (B, T, m) bounds

Shapes: pendulum_euler (2, 1) T 5 B 6; cartpole1l (4, 1) T 6 B 3; rexquadrotor (12, 4) T 4 B 3 (the full 16-lane row,
n_ctrl > 1: the `+ k` term of the index); Given<3, 2> T 5 B 5 (the ragged last lane group); the single-launch solve at
pendulum_euler T 5 and cartpole1l T 32, B 3.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from oracle import al_oracle, al_solve_oracle as aso, dyn_host

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "BOUNDS_AL_pendulum_T5_b6.npz")

MODELS = [("pendulum_euler", 5, 6), ("cartpole1l", 6, 3), ("rexquadrotor", 4, 3)]
FUSED = [("pendulum_euler", 5, 3), ("cartpole1l", 32, 3)]
LAYOUTS = ["per_knot", "per_sample", "full"]
SIZES = {"pendulum_euler": (2, 1), "cartpole1l": (4, 1), "rexquadrotor": (12, 4)}
WIDTH = {"pendulum_euler": 5.0, "cartpole1l": 6.0, "rexquadrotor": 6.0}      # half-width of the widest control box
HOVER = 14.5            # the quadrotor's motor command around which the tests put its bounds (test_gpu_al.py:400,409)


@pytest.fixture(autouse=True)
def _auto_lane_group():
    yield
    from diff_qp_mpc_amd import _lib
    _lib.load().dqp_al_lane_group(0)


def dev(a, grad=False):
    t = torch.tensor(np.asarray(a), dtype=torch.float64, device="cuda")
    return t.requires_grad_() if grad else t


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


# ------------------------------------------------------------------ bounds
def expand(vec, layout, B, T):
    """a (m,) numpy vector in one of the layouts, as a contiguous array of that shape"""
    m = vec.shape[0]
    shape = {"vector": (m,), "per_knot": (T, m), "per_sample": (B, 1, m), "full": (B, T, m)}[layout]
    return np.ascontiguousarray(np.broadcast_to(vec, shape))


def varying(mid, width, B, T, m, freeze=None):
    """(lo, hi) of shape (B, T, m): mid -+ width * scale[b] * fade[b, t] * (1 + 0.1 k), scale from 30 % to 100 % over the
    samples; the limit fades linearly to 20 % along the horizon on the even samples and grows from 20 % on the odd ones
    (tight while the control is large, loose later).  freeze = (b, t): lo == hi there."""
    scale = np.linspace(0.3, 1.0, B)[:, None, None]
    fade = np.tile(np.linspace(1.0, 0.2, T)[None, :, None], (B, 1, 1))
    fade[1::2] = fade[1::2, ::-1]
    w = width * scale * fade * (1.0 + 0.1 * np.arange(m))[None, None, :]
    lo, hi = mid - w, mid + w
    if freeze is not None:
        b, t = freeze
        lo[b, t] = hi[b, t] = mid + 0.25 * w[b, t]
    return np.ascontiguousarray(lo), np.ascontiguousarray(hi)


def strip_layout(name):
    """a kernel's traced name without what tells the bound layout: the StridedBounds<> wrapper of the model, the
    <true> / <false> of the kernels templated on the layout alone, and the parameter list (the strided kernels' argument
    struct carries the strides)"""
    i = name.find("_kernel")
    if i >= 0:
        i += len("_kernel")
        if name[i:i + 1] == "<":
            depth = 0
            while i < len(name):
                depth += {"<": 1, ">": -1}.get(name[i], 0)
                i += 1
                if depth == 0:
                    break
        name = name[:i]
    key = "dqp::StridedBounds<"
    while key in name:
        i = name.index(key)
        j, depth = i + len(key), 1
        while depth:
            depth += {"<": 1, ">": -1}.get(name[j], 0)
            j += 1
        name = name[:i] + name[i + len(key):j - 1].rstrip() + name[j:]
    return re.sub(r"_kernel<(true|false)>$", "_kernel", name).replace(" >", ">")


def same_bytes(a, b, what):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), "%s: %s differs" % (what, k)


def same_launches(vec, strided, what):
    """the launch list of the vector call, on the strided instantiations"""
    assert [strip_layout(k) for k in strided] == [strip_layout(k) for k in vec], (what, vec, strided)
    reads_bounds = [k for k in strided if re.search(r"al_(banded_newton|ls|ls_group|outer|merit|linearize|solve_fused)_kernel", k)]
    assert reads_bounds and all("StridedBounds<" in k or "_kernel<true>" in k for k in reads_bounds), (what, strided)
    assert not any("StridedBounds<" in k or "_kernel<true>" in k for k in vec), (what, vec)


# ------------------------------------------------------------------ one Newton step's data (C ABI level)
def step_data(robot, T, B, seed):
    """the inputs of test_gpu_al.py::test_banded_newton_step_vs_dense_oracle at this shape (numpy); bounds mid -+ 0.3"""
    n, m = SIZES[robot]
    nt = n + m
    rng = np.random.default_rng(seed)
    xu = 0.5 * rng.standard_normal((B, T, nt))
    mid = HOVER if robot == "rexquadrotor" else 0.0
    if robot == "rexquadrotor":
        xu[..., n:] = HOVER + 0.3 * rng.standard_normal((B, T, m))
    d = dict(xu=xu, x0=xu[:, 0, :n] + 0.1 * rng.standard_normal((B, n)), Qd=rng.random((B, T, nt)) + 0.1,
             q=rng.standard_normal((B, T, nt)), lam=rng.standard_normal((B, T * n + 2 * T * m)),
             rho=10.0 ** rng.integers(0, 3, (B, 1)).astype(np.float64))
    return d, np.full(m, mid - 0.3), np.full(m, mid + 0.3), mid


class Call:
    """The C-ABI entry points of one problem, each through its vector form (bounds = None) or its `_bounds` twin."""

    def __init__(self, robot, T, B, d, lo, hi, layout):
        from diff_qp_mpc_amd import _lib, al_utils
        from diff_qp_mpc_amd.dynamics import DeviceDynamics
        self.lib, self._lib = _lib.load(), _lib
        self.dyn = DeviceDynamics(robot)
        self.n, self.m, self.T, self.B = self.dyn.n_state, self.dyn.n_ctrl, T, B
        self.nt, self.ncon = self.n + self.m, T * self.n + 2 * T * self.m
        self.dims = _lib.dqp_al_mpc_dims(B, self.n, self.m, T)
        self.t = {k: dev(v).contiguous() for k, v in d.items()}
        self.t["rho"] = self.t["rho"].reshape(B).contiguous()
        self.lo, self.hi = dev(lo), dev(hi)
        self.bd = None if layout is None else al_utils.bounds_layout(self.lo, self.hi, B, T, self.m)
        if layout is not None:
            want = {"vector": (0, 0), "per_knot": (0, self.m), "per_sample": (self.m, 0), "full": (T * self.m, self.m)}
            assert (self.bd.stride_b, self.bd.stride_t) == want[layout]
        self.kw = dict(dtype=torch.float64, device="cuda")

    def _run(self, fn, outs):
        with self._lib.trace(256) as tr:
            rc = fn()
            torch.cuda.synchronize()
        assert rc == 0, rc
        return {k: v.cpu().numpy() for k, v in outs.items()}, [k for k, _ in tr.records]

    def _bounds(self):
        return (self.bd.ref(),) if self.bd is not None else (P(self.lo), P(self.hi))

    def _entry(self, name):
        return getattr(self.lib, name + ("_bounds" if self.bd is not None else ""))

    def factor(self):
        return torch.full((int(self.lib.dqp_al_banded_factor_bytes(ctypes.byref(self.dims), self.dyn.id)) // 8,), np.nan, **self.kw)

    def newton_step(self):
        t, B, T, nt = self.t, self.B, self.T, self.nt
        o = dict(upd=torch.full((B, T, nt), np.nan, **self.kw), fac=self.factor(),
                 info=torch.full((B,), -7, dtype=torch.int32, device="cuda"))
        return self._run(lambda: self._entry("dqp_al_banded_newton_step")(
            ctypes.byref(self.dims), self.dyn.id, self.dyn.dt, P(t["xu"]), P(t["x0"]), P(t["Qd"]), P(t["q"]), P(t["lam"]),
            P(t["rho"]), *self._bounds(), P(o["upd"]), P(o["fac"]), P(o["info"]), None), o)

    def merit(self, ncand=20):
        t, B, T, n, m = self.t, self.B, self.T, self.n, self.m
        steps = (2.0 ** -torch.arange(ncand, **self.kw))[:, None, None, None]
        cand = (t["xu"][None] * (1.0 + steps)).contiguous()
        xn = self.dyn(cand[:, :, :-1, :n].reshape(-1, n).contiguous(), cand[:, :, :-1, n:].reshape(-1, m).contiguous())
        self.cand, self.xn = cand, xn.reshape(ncand, B, T - 1, n).contiguous()
        o = dict(merit=torch.full((ncand, B), np.nan, **self.kw))
        return self._run(lambda: self._entry("dqp_al_merit")(
            ctypes.byref(self.dims), ncand, P(self.cand), P(self.xn), P(t["x0"]), P(t["Qd"]), P(t["q"]), P(t["lam"]),
            P(t["rho"]), *self._bounds(), P(o["merit"]), None), o)

    def outer_update(self):
        t, B = self.t, self.B
        o = dict(lam_new=torch.full((B, self.ncon), np.nan, **self.kw), cost=torch.full((B,), np.nan, **self.kw),
                 resn=torch.full((B,), np.nan, **self.kw))
        return self._run(lambda: self._entry("dqp_al_outer_update")(
            ctypes.byref(self.dims), self.dyn.id, self.dyn.dt, P(t["xu"]), P(t["x0"]), P(t["lam"]), P(t["rho"]), P(t["Qd"]),
            P(t["q"]), *self._bounds(), P(o["lam_new"]), P(o["cost"]), P(o["resn"]), None), o)

    def newton_solve(self):
        t, B = self.t, self.B
        ws = torch.zeros(int(self.lib.dqp_al_newton_solve_bytes(ctypes.byref(self.dims), 1)) // 8 + 1, **self.kw)
        o = dict(xu=t["xu"].clone(), L=self.factor(), status=torch.full((B,), np.nan, **self.kw),
                 fail=torch.full((1,), -7, dtype=torch.int32, device="cuda"))
        return self._run(lambda: self._entry("dqp_al_newton_solve")(
            ctypes.byref(self.dims), self.dyn.id, self.dyn.dt, 4, 1, P(t["x0"]), P(t["Qd"]), P(t["q"]), P(t["lam"]), P(t["rho"]),
            *self._bounds(), P(o["xu"]), P(o["L"]), P(o["status"]), P(o["fail"]), P(ws), None), o)

    def mpc_solve(self, fused=False, al_iter=2):
        t, B, T, n, m = self.t, self.B, self.T, self.n, self.m
        ws = torch.zeros(int(self.lib.dqp_al_mpc_solve_bytes(ctypes.byref(self.dims))) // 8 + 1, **self.kw)
        x_init, u_init = t["xu"][..., :n].contiguous(), t["xu"][..., n:].contiguous()
        lam0, rho0 = torch.zeros(B, self.ncon, **self.kw), torch.ones(B, **self.kw)
        full = lambda *s: torch.full(s, np.nan, **self.kw)
        o = dict(xu=full(B, T, self.nt), hc=full(al_iter + 1, B), hl=full(al_iter + 1, B, self.ncon), hr=full(al_iter + 1, B),
                 resn=full(B), fac=self.factor(), status=full(B), fail=torch.full((al_iter,), -7, dtype=torch.int32, device="cuda"))
        name = "dqp_al_mpc_solve_fused" if fused else "dqp_al_mpc_solve"
        return self._run(lambda: self._entry(name)(
            ctypes.byref(self.dims), self.dyn.id, self.dyn.dt, al_iter, 4, P(x_init), P(u_init), P(t["x0"]), P(t["Qd"]), P(t["q"]),
            *self._bounds(), P(lam0), P(rho0), None, None, None, 0, P(o["xu"]), P(o["hc"]), P(o["hl"]), P(o["hr"]), P(o["resn"]),
            P(o["fac"]), P(o["status"]), P(o["fail"]), P(ws), None), o)


ENTRIES = ["newton_step", "merit", "outer_update", "newton_solve", "mpc_solve"]


# ------------------------------------------------------------------ 1
@pytest.mark.parametrize("robot,T,B", MODELS)
def test_layout_equivalence_c_abi(robot, T, B):
    """Every twin at every layout of an expanded vector: the bytes of the vector entry point (update, factor, info,
    merit, multipliers, cost, residual norm, iterate, status, flags, history), from the same launches on the strided
    instantiations.  Both lane groups of the half-row models."""
    from diff_qp_mpc_amd import _lib
    d, lo, hi, _ = step_data(robot, T, B, seed=11 * T + B)
    groups = (16, 8) if sum(SIZES[robot]) <= 8 else (16,)
    for group in groups:
        assert _lib.load().dqp_al_lane_group(group) == 0
        old = Call(robot, T, B, d, lo, hi, None)
        ref = {e: getattr(old, e)() for e in ENTRIES}
        vec = Call(robot, T, B, d, lo, hi, "vector")               # the twin at (0, 0): the vector kernels themselves
        for e in ENTRIES:
            out, names = getattr(vec, e)()
            same_bytes(out, ref[e][0], "%s vector twin" % e)
            assert names == ref[e][1], (e, names, ref[e][1])
        for layout in LAYOUTS:
            c = Call(robot, T, B, d, expand(lo, layout, B, T), expand(hi, layout, B, T), layout)
            for e in ENTRIES:
                out, names = getattr(c, e)()
                same_bytes(out, ref[e][0], "%s %s group %d" % (e, layout, group))
                same_launches(ref[e][1], names, "%s %s group %d" % (e, layout, group))
        assert np.isfinite(ref["newton_step"][0]["upd"]).all() and not ref["newton_step"][0]["info"].any()


@pytest.mark.parametrize("robot,T,B", FUSED)
def test_layout_equivalence_fused_solve(robot, T, B):
    """dqp_al_mpc_solve_fused_bounds: one launch of the strided instantiation, the bytes of the vector launch -- at
    T = 32 with the staged bounds in the carve's last 2 T n_ctrl doubles."""
    d, lo, hi, _ = step_data(robot, T, B, seed=5 * T + B)
    d["xu"] *= 0.2                                       # a milder start: 32 knots of random states are far from a trajectory
    d["x0"] = d["xu"][:, 0, :SIZES[robot][0]].copy()
    ref, names = Call(robot, T, B, d, lo, hi, None).mpc_solve(fused=True)
    assert len(names) == 1 and "al_solve_fused_kernel" in names[0], names
    for layout in ["vector"] + LAYOUTS:
        out, got = Call(robot, T, B, d, expand(lo, layout, B, T), expand(hi, layout, B, T), layout).mpc_solve(fused=True)
        same_bytes(out, ref, "fused %s" % layout)
        if layout == "vector":
            assert got == names
        else:
            same_launches(names, got, "fused %s" % layout)


def test_layout_equivalence_caller_jacobians():
    """dqp_al_banded_newton_step_jac_bounds at Given<3, 2>, T = 5, B = 5 (an odd batch: the last lane group is ragged in
    both widths), then dqp_al_banded_solve on the factor."""
    from diff_qp_mpc_amd import _lib, al_utils
    from test_gpu_al_given import problem
    lib = _lib.load()
    n, m, T, B = 3, 2, 5, 5
    p = problem(n, m, T, B=B, seed=17)
    t = {k: dev(v).contiguous() for k, v in p.items()}
    dims = _lib.dqp_al_mpc_dims(B, n, m, T)
    nt = n + m

    def run(layout):
        lo, hi = dev(expand(p["lo"], layout or "vector", B, T)), dev(expand(p["hi"], layout or "vector", B, T))
        fac = torch.full((int(lib.dqp_al_banded_jac_factor_bytes(ctypes.byref(dims))) // 8,), np.nan, dtype=torch.float64, device="cuda")
        o = dict(upd=torch.full((B, T, nt), np.nan, dtype=torch.float64, device="cuda"), fac=fac,
                 out=torch.full((B, T, nt), np.nan, dtype=torch.float64, device="cuda"),
                 info=torch.full((B,), -7, dtype=torch.int32, device="cuda"))
        head = (ctypes.byref(dims), P(t["xu"]), P(t["x0"]), P(t["Qd"]), P(t["q"]), P(t["lam"]), P(t["rho"].reshape(B).contiguous()))
        tail = (P(t["xn"]), P(t["Jx"]), P(t["Ju"]), P(o["upd"]), P(fac), P(o["info"]), None)
        with _lib.trace(16) as tr:
            if layout is None:
                rc = lib.dqp_al_banded_newton_step_jac(*head, P(lo), P(hi), *tail)
            else:
                bd = al_utils.bounds_layout(lo, hi, B, T, m)
                rc = lib.dqp_al_banded_newton_step_jac_bounds(*head, bd.ref(), *tail)
            assert rc == 0
            assert lib.dqp_al_banded_solve(ctypes.byref(dims), 0, P(fac), P(t["rhs"]), P(o["out"]), None) == 0
            torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in o.items()}, [k for k, _ in tr.records]

    for group in (16, 8):
        assert lib.dqp_al_lane_group(group) == 0
        ref, names = run(None)
        assert not ref["info"].any() and np.isfinite(ref["upd"]).all()
        out, got = run("vector")
        same_bytes(out, ref, "vector twin")
        assert got == names
        for layout in LAYOUTS:
            out, got = run(layout)
            same_bytes(out, ref, "%s group %d" % (layout, group))
            assert [strip_layout(k) for k in got] == [strip_layout(k) for k in names]
            assert "StridedBounds<" in got[0] and "Given<3, 2>" in got[0] and "StridedBounds<" not in names[0], (got, names)


# ------------------------------------------------------------------ AL_mpc.MPC problems (numpy)
def mpc_problem(robot, T, B, seed=0):
    """x0, Qd, c, the initial guess and a (mid, width) of the control box for which the solution saturates on some
    samples and knots only.  Pendulum: the golden's cost; cartpole / quadrotor: the fixtures' (make_golden_cfg3 / cfg4)."""
    n, m = SIZES[robot]
    r = np.random.default_rng(seed)
    if robot == "pendulum_euler":
        x0 = np.stack([3.0 * (r.random(B) - 0.5), r.random(B) - 0.5], 1)
        Qd = np.broadcast_to(np.array([10.0, 1.0, 0.01]), (B, T, 3)).copy()
        mid, width, dt = 0.0, WIDTH[robot], 0.05
    elif robot == "cartpole1l":
        x0 = r.uniform(-0.5, 0.5, (B, n))
        Qd = np.broadcast_to(np.concatenate([np.ones(n), 1e-3 * np.ones(m)]), (B, T, n + m)).copy()
        mid, width, dt = 0.0, WIDTH[robot], 0.05
    else:
        x0 = r.uniform(-0.5, 0.5, (B, n))
        Qd = np.broadcast_to(np.concatenate([np.ones(n), 1e-3 * np.ones(m)]), (B, T, n + m)).copy()
        mid, width, dt = HOVER, WIDTH[robot], 0.05
    x0[-1] *= 0.01                              # one sample next to the target: no bound becomes active
    x_ref = x0[:, None, :] * np.linspace(1.0, 0.0, T)[None, :, None]
    u_ref = np.full((B, T, m), mid)
    c = -(Qd * np.concatenate([x_ref, u_ref], -1))
    return dict(x0=x0, Qd=Qd, c=c, x_init=x_ref, u_init=u_ref, mid=mid, width=width, dt=dt)


def oracle_step_fn(robot, dt):
    if robot == "pendulum_euler":
        assert dt == al_oracle.DT
        return al_oracle.pendulum_step
    step = dyn_host.stepper(robot, dt)
    assert step is not None, "the host build of the dynamics needs hipcc"
    return step


# x, u, multipliers of AL_mpc.MPC against the reference / the oracle: test_gpu_al.py:248-260 (pendulum: x, u rtol 1e-4 /
# atol 1e-5, multipliers rtol 1e-5 / atol 1e-7 cold and 1e-6 warm) and test_gpu_al.py:290-301 (cartpole, quadrotor: x, u
# rtol 1e-4 / atol 1e-4, multipliers rtol 1e-5 / atol 1e-5); rho exact (:251, :293)
def mpc_tol(robot):
    if robot == "pendulum_euler":
        return dict(xu=(1e-4, 1e-5), lam=((1e-5, 1e-7), (1e-5, 1e-6)))
    return dict(xu=(1e-4, 1e-4), lam=((1e-5, 1e-5), (1e-5, 1e-5)))


def oracle_two_calls(robot, T, B, p, lo, hi):
    n, m = SIZES[robot]
    step = oracle_step_fn(robot, p["dt"])
    lam0, rho0 = np.zeros((B, T * n + 2 * T * m)), np.ones((B, 1))
    o1 = aso.al_solve(p["x_init"], p["u_init"], p["x0"], p["Qd"], p["c"], lo, hi, step, lam0, rho0)
    # AL_mpc.py:250-251: the warm call starts from the float32 solution of the first
    o2 = aso.al_solve(o1["x"].astype(np.float32).astype(np.float64), o1["u"].astype(np.float32).astype(np.float64), p["x0"],
                      p["Qd"], p["c"], lo, hi, step, o1["lam"], o1["rho"], history=o1["history"])
    return o1, o2


_ORACLE = {}


def varying_case(robot, T, B, freeze=None):
    """problem, varying bounds and the oracle's two calls, computed once per case and left unchanged"""
    key = (robot, T, B, freeze)
    if key not in _ORACLE:
        n, m = SIZES[robot]
        p = mpc_problem(robot, T, B)
        lo, hi = varying(p["mid"], p["width"], B, T, m, freeze)
        _ORACLE[key] = (p, lo, hi) + oracle_two_calls(robot, T, B, p, lo, hi)
    return _ORACLE[key]


def assert_strides_matter(robot, T, B, p, lo, hi, o1):
    """The condition on the inputs, on the oracle alone: bounds active at some knots and inactive at others on at least
    two samples, none active on at least one; and the solution under every uniform bound built from the per-control min
    or max of the varying one is at least 100 x the tolerance away from the solution under the varying one."""
    n, m = SIZES[robot]
    gap = np.minimum(hi - o1["u"], o1["u"] - lo).min(axis=2)[:, :-1]          # (the last knot's control is free)
    act, inact = gap <= 1e-3 * p["width"], gap >= 1e-2 * p["width"]
    assert (act.any(1) & inact.any(1)).sum() >= 2 and inact.all(1).sum() >= 1, (act, inact)
    rtol, atol = mpc_tol(robot)["xu"]
    step = oracle_step_fn(robot, p["dt"])
    lam0, rho0 = np.zeros((B, T * n + 2 * T * m)), np.ones((B, 1))
    for pick_lo, pick_hi in ((np.min, np.max), (np.max, np.min), (np.min, np.min), (np.max, np.max)):
        ul, uh = pick_lo(lo, axis=(0, 1)), pick_hi(hi, axis=(0, 1))
        if (ul > uh).any():
            continue                                           # (max of the lower above min of the upper: the frozen knot)
        o = aso.al_solve(p["x_init"], p["u_init"], p["x0"], p["Qd"], p["c"], ul, uh, step, lam0, rho0)
        diff = np.abs(o["xu"] - o1["xu"])
        assert (diff >= 100.0 * (atol + rtol * np.abs(o1["xu"]))).any(), (pick_lo.__name__, pick_hi.__name__, diff.max())


def run_mpc(robot, T, B, p, lo, hi, grads=False, calls=2):
    """AL_mpc.MPC on the device, `calls` calls -> list of dicts (numpy)"""
    from diff_qp_mpc_amd import AL_mpc, _lib, al_utils
    from diff_qp_mpc_amd.dynamics import DeviceDynamics
    n, m = SIZES[robot]
    dyn = DeviceDynamics(robot, dt=p["dt"])
    x0 = dev(p["x0"])
    C = torch.diag_embed(dev(p["Qd"])).requires_grad_(grads)
    c = dev(p["c"], grad=grads)
    ctrl = AL_mpc.MPC(n, m, T, u_lower=dev(lo), u_upper=dev(hi), n_batch=B, verbose=0, al_iter=2, solver_type="dense",
                      dtype=torch.float64, eps=1e-5, exit_unconverged=False, backprop=False)
    ctrl.reinitialize(x0, torch.ones(B, T, 1, device="cuda"))
    ctrl.x_init, ctrl.u_init = dev(p["x_init"]), dev(p["u_init"])
    outs = []
    for k in range(calls):
        with _lib.trace(512) as tr:
            x, u = ctrl(x0, al_utils.QuadCost(C if k == 0 else C.detach(), c if k == 0 else c.detach()), dyn, dyn.jac)
        o = dict(x=x.detach().cpu().numpy(), u=u.detach().cpu().numpy(), lam=ctrl.lamda_prev.cpu().numpy(),
                 rho=ctrl.rho_prev.cpu().numpy(),
                 hist_cost=torch.stack([t.reshape(B) for t in ctrl.cost_lam_hist[0]]).cpu().numpy(),
                 hist_lam=torch.stack(list(ctrl.cost_lam_hist[1])).cpu().numpy(),
                 hist_rho=torch.stack([t.reshape(B) for t in ctrl.cost_lam_hist[2]]).cpu().numpy())
        assert not any(bool(f.any()) for f in ctrl.fail_log)
        if k == 0 and grads:
            (x.double().sum() + 2.0 * u.double().sum()).backward()
            o.update(dC=C.grad.diagonal(dim1=-2, dim2=-1).cpu().numpy().copy(), dc=c.grad.cpu().numpy().copy())
        outs.append((o, [kn for kn, _ in tr.records]))
    return outs


@pytest.mark.parametrize("robot,T,B", MODELS)
def test_layout_equivalence_al_mpc(robot, T, B):
    """AL_mpc.MPC with the vector expanded to each layout: x, u, cost_lam_hist and the gradients of C's diagonal and c to
    the last bit, cold and warm call, on the launch list of the vector call (on the parent the expanded bounds took the
    general path: another list)."""
    p = mpc_problem(robot, T, B)
    m = SIZES[robot][1]
    lo, hi = np.full(m, p["mid"] - 0.5 * p["width"]), np.full(m, p["mid"] + 0.5 * p["width"])
    ref = run_mpc(robot, T, B, p, lo, hi, grads=True)
    assert any("al_banded_newton_kernel" in k for k in ref[0][1])
    for layout in LAYOUTS:
        got = run_mpc(robot, T, B, p, expand(lo, layout, B, T), expand(hi, layout, B, T), grads=True)
        for (a, an), (b, bn), call in zip(got, ref, ("cold", "warm")):
            same_bytes(a, b, "%s %s" % (layout, call))
            same_launches(bn, an, "%s %s" % (layout, call))


# ------------------------------------------------------------------ 2
@pytest.mark.parametrize("freeze", [None, (1, 2)])
@pytest.mark.parametrize("robot,T,B", MODELS)
def test_varying_bounds_al_mpc_vs_oracle(robot, T, B, freeze):
    """x, u, multipliers and rho after al_iter = 2, cold and warm call, under bounds that shrink to 20 % along the horizon,
    differently per sample (freeze: lo == hi at one knot of one sample), against oracle/al_solve_oracle.al_solve."""
    p, lo, hi, o1, o2 = varying_case(robot, T, B, freeze)
    assert_strides_matter(robot, T, B, p, lo, hi, o1)
    if freeze is not None:
        b, t = freeze
        assert (lo[b, t] == hi[b, t]).all()
    tol = mpc_tol(robot)
    got = run_mpc(robot, T, B, p, lo, hi)
    assert any("al_banded_newton_kernel<dqp::StridedBounds<" in k for k in got[0][1]), got[0][1]
    for (g, _), o, lam_tol, call in zip(got, (o1, o2), tol["lam"], ("cold", "warm")):
        for k in ("x", "u"):
            print(call, k, "max |gpu - oracle| = %.3e" % float(np.abs(g[k] - o[k]).max()))
        for k in ("x", "u"):
            np.testing.assert_allclose(g[k], o[k], rtol=tol["xu"][0], atol=tol["xu"][1], err_msg=call + " " + k)
        np.testing.assert_allclose(g["lam"], o["lam"], rtol=lam_tol[0], atol=lam_tol[1], err_msg=call)
        np.testing.assert_array_equal(g["rho"], o["rho"], err_msg=call)
        if freeze is not None and call == "cold":
            b, t = freeze
            assert np.abs(g["u"][b, t] - hi[b, t]).max() < 1e-2 * p["width"]       # the frozen control sits at its value


@pytest.mark.parametrize("robot,T,B", MODELS)
def test_varying_bounds_kernels_vs_oracle(robot, T, B):
    """One Newton step's update (rtol 1e-8 / atol 1e-10: test_gpu_al.py:433), the merit of 20 candidates (rtol 1e-12 /
    atol 1e-10: test_gpu_al.py:211) and the outer update (multipliers, cost and residual norm at the multipliers'
    tolerance rtol 1e-5 / atol 1e-7: test_gpu_al.py:250, as test_gpu_integrator.py:227 treats the history rows) under
    varying bounds with a frozen knot, against oracle/al_oracle.py and oracle/al_solve_oracle.py on the device model's
    own Jacobians (as test_gpu_al.py:412-421)."""
    n, m = SIZES[robot]
    d, _, _, mid = step_data(robot, T, B, seed=3 * T + B)
    # (the controls are N(mid, 0.5^2), the quadrotor's four N(mid, 0.3^2): a box in which some knots of a sample have an
    # active row and some have none -- checked below)
    lo, hi = varying(mid, 1.5 if robot == "rexquadrotor" else 0.45, B, T, m, freeze=(1, 2))
    c = Call(robot, T, B, d, lo, hi, "full")
    dyn = c.dyn

    def step_np(x, u):
        xn, (Jx, Ju) = dyn.jac(dev(x), dev(u))
        return xn.cpu().numpy(), Jx.cpu().numpy(), Ju.cpu().numpy()

    res, resc, J, Jc = al_oracle.constraint_jacobian(d["xu"], d["x0"], lo, hi, step=step_np)
    iq = res[:, T * n:].reshape(B, T, 2 * m)
    mixed = ((iq > 0).any(2).any(1) & (iq.max(2) <= 0).any(1))
    assert mixed.sum() >= 2, iq                                     # active at some knots, inactive at others
    grad = al_oracle.merit_grad(d["xu"], d["Qd"], d["q"], d["lam"], d["rho"], resc, J, Jc)
    upd_ref, _, info_ref = al_oracle.newton_update(Jc, d["Qd"].reshape(B, -1), d["rho"], grad)
    assert not info_ref.any()
    out, names = c.newton_step()
    assert "StridedBounds<" in names[0]
    assert not out["info"].any()
    np.testing.assert_allclose(out["upd"].reshape(B, -1), upd_ref, rtol=1e-8, atol=1e-10)
    # ignoring the strides would not pass: the update under the first sample's first-knot bounds for everybody differs
    res_u, resc_u, J_u, Jc_u = al_oracle.constraint_jacobian(d["xu"], d["x0"], lo[0, 0], hi[0, 0], step=step_np)
    grad_u = al_oracle.merit_grad(d["xu"], d["Qd"], d["q"], d["lam"], d["rho"], resc_u, J_u, Jc_u)
    upd_u = al_oracle.newton_update(Jc_u, d["Qd"].reshape(B, -1), d["rho"], grad_u)[0]
    assert (np.abs(upd_u - upd_ref) >= 100.0 * (1e-10 + 1e-8 * np.abs(upd_ref))).any()
    # merit
    out, names = c.merit()
    assert len(names) == 1 and "al_merit_kernel<true>" in names[0], names
    cand = c.cand.cpu().numpy()
    want = np.stack([aso.merit(cand[k], d["Qd"], d["q"], d["x0"], d["lam"], d["rho"], lo, hi, step_np) for k in range(cand.shape[0])])
    np.testing.assert_allclose(out["merit"], want, rtol=1e-12, atol=1e-10)
    # outer update
    out, names = c.outer_update()
    assert "al_outer_kernel<dqp::StridedBounds<" in names[0]
    res, resc = aso.residuals(d["xu"], d["x0"], lo, hi, step_np)
    lam_new = d["lam"] + d["rho"] * res
    lam_new[:, T * n:] = np.maximum(lam_new[:, T * n:], 0.0)
    np.testing.assert_allclose(out["lam_new"], lam_new, rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(out["cost"], aso.compute_cost(d["xu"], d["Qd"], d["q"]), rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(out["resn"], np.linalg.norm(resc, axis=1), rtol=1e-5, atol=1e-7)


# ------------------------------------------------------------------ 3
@pytest.mark.parametrize("robot,T,B", MODELS)
def test_backward_vs_general_path(robot, T, B, monkeypatch):
    """Gradients of sum(x) + 2 sum(u) wrt C's diagonal and c under varying bounds: the one-call device solve against the
    project's general torch path (ONE_CALL_SOLVE = False, FUSED_NEWTON_AL = False) on the same inputs, at the tolerance
    of the AL gradient tests (test_gpu_al.py:253-254, :295-296: rtol 1e-4, atol 1e-6 pendulum / 1e-5 others)."""
    from diff_qp_mpc_amd import AL_mpc
    p, lo, hi, o1, _ = varying_case(robot, T, B)
    dev_out = run_mpc(robot, T, B, p, lo, hi, grads=True, calls=1)[0]
    monkeypatch.setattr(AL_mpc, "ONE_CALL_SOLVE", False)
    monkeypatch.setattr(AL_mpc, "FUSED_NEWTON_AL", False)
    monkeypatch.setattr(AL_mpc, "BANDED_USER_DYNAMICS", False)      # (else the module's Jacobians take the banded step)
    gen_out = run_mpc(robot, T, B, p, lo, hi, grads=True, calls=1)[0]
    assert any("al_banded_newton_kernel" in k for k in dev_out[1]) and not any("al_banded_newton_kernel" in k for k in gen_out[1])
    atol = 1e-6 if robot == "pendulum_euler" else 1e-5
    for k in ("dC", "dc"):
        print(k, "max |device - general| = %.3e" % float(np.abs(dev_out[0][k] - gen_out[0][k]).max()))
    assert np.abs(dev_out[0]["dc"]).max() > 1e-3
    for k in ("dC", "dc"):
        np.testing.assert_allclose(dev_out[0][k], gen_out[0][k], rtol=1e-4, atol=atol, err_msg=k)


# ------------------------------------------------------------------ 4
@pytest.mark.parametrize("persistent", [False, True])
def test_reference_golden(persistent, monkeypatch):
    """BOUNDS_AL_pendulum_T5_b6.npz -- the reference's AL_mpc.MPC under (B, T, m) bounds, cold call with gradients and warm
    call -- through AL_mpc.MPC with PERSISTENT_SOLVE off and on, at the tolerances of
    test_gpu_integrator.py::test_al_mpc_two_calls_vs_reference (:224-232)."""
    from diff_qp_mpc_amd import AL_mpc, _lib, al_utils
    from diff_qp_mpc_amd.dynamics import DeviceDynamics
    monkeypatch.setattr(AL_mpc, "PERSISTENT_SOLVE", persistent)
    monkeypatch.setattr(AL_mpc, "PERSISTENT_SOLVE_MAX_BATCH", 6 if persistent else 0)
    g = dict(np.load(GOLDEN, allow_pickle=False))
    B, T = g["in_Qd"].shape[:2]
    assert g["in_u_lower"].shape == (B, T, 1)
    dyn = DeviceDynamics("pendulum_euler", dt=float(g["dt"]))
    x0 = dev(g["in_x0"])
    C = torch.diag_embed(dev(g["in_Qd"])).requires_grad_()
    c = dev(g["in_c"], grad=True)
    u_init = dev(g["in_u_init"])
    ctrl = AL_mpc.MPC(2, 1, T, u_lower=dev(g["in_u_lower"]), u_upper=dev(g["in_u_upper"]), n_batch=B, verbose=0, u_init=u_init,
                      al_iter=2, solver_type="dense", dtype=torch.float64, eps=1e-5, exit_unconverged=False, backprop=False)
    ctrl.reinitialize(x0, torch.ones(B, T, 1, device="cuda"))
    ctrl.u_init = u_init
    hist = lambda: (torch.stack([t.reshape(B) for t in ctrl.cost_lam_hist[0]]).cpu().numpy(),
                    torch.stack(list(ctrl.cost_lam_hist[1])).cpu().numpy(),
                    torch.stack([t.reshape(B) for t in ctrl.cost_lam_hist[2]]).cpu().numpy())
    with _lib.trace(512) as tr:
        x, u = ctrl(x0, al_utils.QuadCost(C, c), dyn, dyn.jac)
    kernels = [k for k, _ in tr.records]
    fused = [k for k in kernels if "al_solve_fused_kernel" in k]
    newton = [k for k in kernels if "al_banded_newton_kernel" in k]
    if persistent:
        assert len(fused) == 1 and "StridedBounds<dqp::dyn::PendulumEuler>" in fused[0] and not newton, kernels
    else:
        assert not fused and len(newton) == 8 and all("StridedBounds<dqp::dyn::PendulumEuler>" in k for k in newton), kernels
    assert not any(bool(f.any()) for f in ctrl.fail_log)
    (x.double().sum() + 2.0 * u.double().sum()).backward()
    o = {}
    hc, hl, hr = hist()
    o.update(x1=x.detach().cpu().numpy(), u1=u.detach().cpu().numpy(), lam1=ctrl.lamda_prev.cpu().numpy(),
             rho1=ctrl.rho_prev.cpu().numpy(), hist_cost1=hc, hist_lam1=hl, hist_rho1=hr,
             dC1=C.grad.diagonal(dim1=-2, dim2=-1).cpu().numpy(), dc1=c.grad.cpu().numpy())
    x2, u2 = ctrl(x0, al_utils.QuadCost(C.detach(), c.detach()), dyn, dyn.jac)
    hc, hl, hr = hist()
    o.update(x2=x2.cpu().numpy(), u2=u2.cpu().numpy(), lam2=ctrl.lamda_prev.cpu().numpy(), rho2=ctrl.rho_prev.cpu().numpy(),
             hist_cost2=hc, hist_lam2=hl, hist_rho2=hr)
    for call, lam_atol in (("1", 1e-7), ("2", 1e-6)):
        for k in ("x", "u"):
            np.testing.assert_allclose(o[k + call], g[k + call], rtol=1e-4, atol=1e-5, err_msg=k + call)
        for k in ("lam", "hist_lam", "hist_cost"):
            np.testing.assert_allclose(o[k + call], g[k + call], rtol=1e-5, atol=lam_atol, err_msg=k + call)
        for k in ("rho", "hist_rho"):
            np.testing.assert_array_equal(o[k + call], g[k + call], err_msg=k + call)
    np.testing.assert_allclose(o["dC1"], g["dC1"], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(o["dc1"], g["dc1"], rtol=1e-4, atol=1e-6)


# ------------------------------------------------------------------ 5
def test_graphed_mpc_with_strided_bounds_replays_bitwise():
    """AL_mpc.GraphedMPC captures the cold call with (B, T, m) bounds at cartpole1l T = 6, B = 3 on the default queue
    count and replays it bit for bit -- x, u and the gradients wrt C and c -- on the captured batch and on a second one
    (test_gpu_integrator.py::test_graphed_mpc_replay_bitwise_equal_to_eager, test_gpu_al.py:578-633)."""
    from diff_qp_mpc_amd import AL_mpc, al_utils
    from diff_qp_mpc_amd.dynamics import DeviceDynamics
    robot, T, B = "cartpole1l", 6, 3
    n, m = SIZES[robot]
    dyn = DeviceDynamics(robot)
    p = mpc_problem(robot, T, B)
    lo_np, hi_np = varying(p["mid"], p["width"], B, T, m)
    lo, hi = dev(lo_np), dev(hi_np)
    Qd = dev(p["Qd"])

    def batch(seed):
        q = mpc_problem(robot, T, B, seed=seed)
        x0, x_ref, u_ref = dev(q["x0"]), dev(q["x_init"]), dev(q["u_init"])
        C = torch.diag_embed(Qd).requires_grad_()
        c = dev(q["c"], grad=True)
        return x0, x_ref, u_ref, C, c

    def make():
        return AL_mpc.MPC(n, m, T, u_lower=lo, u_upper=hi, n_batch=B, verbose=0, solver_type="dense", dtype=torch.float64,
                          eps=1e-5, exit_unconverged=False, backprop=False)

    def eager(x0, x_ref, u_ref, C, c):
        ctrl = make()
        ctrl.reinitialize(x0, torch.ones(B, T, 1, device="cuda"))
        ctrl.x_init, ctrl.u_init = x_ref, u_ref
        x, u = ctrl(x0, al_utils.QuadCost(C, c), dyn, dyn.jac)
        gC, gc = torch.autograd.grad(x.double().sum() + 2.0 * u.double().sum(), (C, c))
        return x.detach(), u.detach(), gC, gc

    x0, x_ref, u_ref, C, c = batch(0)
    ctrl = make()
    ctrl.mask = torch.ones(B, T, 1, device="cuda")
    g = AL_mpc.GraphedMPC(ctrl, (x0, C, c), dyn, x_init=x_ref, u_init=u_ref)
    for seed in (0, 1):
        x0b, x_refb, u_refb, Cb, cb = batch(seed)
        g.x_init.copy_(x_refb); g.u_init.copy_(u_refb)
        x, u = g(x0b, Cb, cb)
        gC, gc = torch.autograd.grad(x.double().sum() + 2.0 * u.double().sum(), (Cb, cb))
        wb = eager(x0b, x_refb, u_refb, Cb, cb)
        gap = torch.minimum(hi - u.double(), u.double() - lo)
        assert bool((gap < 1e-3 * p["width"]).any())                # a (per-sample, per-knot) bound is active in the replay
        for a, b in zip((x, u, gC, gc), wb):
            assert torch.equal(a, b)
    assert not g.failed()
