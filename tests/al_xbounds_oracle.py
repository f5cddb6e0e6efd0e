"""State rows for the numpy oracle, from the test side (no test in here; imported by test_al_xbounds_cpu.py and
test_gpu_al_xbounds.py).

oracle/al_oracle.py's merit_grad / hessian / newton_update are generic in the number of rows, and
oracle/al_solve_oracle.py reaches its rows only through `residuals` and `al_oracle.constraint_jacobian`.  extended()
wraps those two for the duration of a `with` block: behind the rows they return it appends the state rows -- knot-major,
per knot [x_t - x_upper (n), x_lower - x_t (n)], +I / -I on the knot's x columns, the clamped copy for Jc -- so that
ncon = T n + 2 T m + 2 T n.  The oracle files are not edited and the algorithm stays the pinned one; only the row
builder is the test's.
"""
import contextlib

import numpy as np
import pytest

from oracle import al_oracle, al_solve_oracle as aso


def ncon_x(n, m, T):
    return T * n + 2 * T * m + 2 * T * n


def state_rows(xu, n, x_lower, x_upper):
    """(B, 2 T n): per knot [x - x_upper, x_lower - x]; the bounds broadcast against (B, T, n)"""
    x = xu[:, :, :n]
    return np.concatenate((x - x_upper, x_lower - x), 2).reshape(xu.shape[0], -1)


def state_jacobian(B, T, n, nt):
    J = np.zeros((B, 2 * T * n, T * nt))
    for t in range(T):
        r, c = t * 2 * n, t * nt
        J[:, r:r + n, c:c + n] = np.eye(n)
        J[:, r + n:r + 2 * n, c:c + n] = -np.eye(n)
    return J


def install(monkeypatch, x_lower, x_upper):
    """monkeypatch.setattr of the two row builders; x_lower / x_upper: anything that broadcasts against (B, T, n)"""
    x_lower, x_upper = np.asarray(x_lower, dtype=np.float64), np.asarray(x_upper, dtype=np.float64)
    base_res, base_jac = aso.residuals, al_oracle.constraint_jacobian

    def residuals(xu, x0, u_lower, u_upper, step):
        res, resc = base_res(xu, x0, u_lower, u_upper, step)
        sx = state_rows(xu, x0.shape[1], x_lower, x_upper)
        return np.concatenate((res, sx), 1), np.concatenate((resc, np.maximum(sx, 0.0)), 1)

    def constraint_jacobian(xu, x0, u_lower, u_upper, step=al_oracle.pendulum_step):
        res, resc, J, Jc = base_jac(xu, x0, u_lower, u_upper, step)
        B, T, nt = xu.shape
        n = x0.shape[1]
        sx = state_rows(xu, n, x_lower, x_upper)
        Jx = state_jacobian(B, T, n, nt)
        return (np.concatenate((res, sx), 1), np.concatenate((resc, np.maximum(sx, 0.0)), 1),
                np.concatenate((J, Jx), 1), np.concatenate((Jc, Jx * (sx > 0)[..., None]), 1))

    monkeypatch.setattr(aso, "residuals", residuals)
    monkeypatch.setattr(al_oracle, "constraint_jacobian", constraint_jacobian)


@contextlib.contextmanager
def extended(x_lower, x_upper):
    """the oracle over the extended rows inside the block (for references computed once and shared between tests)"""
    with pytest.MonkeyPatch.context() as mp:
        install(mp, x_lower, x_upper)
        yield
