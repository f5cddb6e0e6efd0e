"""Records the extended dense oracle's Newton update and factor solve for the two T = 30 wide cases of
tests/test_gpu_al_given_xbounds.py at B = 37 (ALGX_n13_m4_T30_b37.npz, ALGX_n24_m8_T30_b37.npz): the oracle's einsum
Hessian over 2640 rows x 960 columns takes minutes, too long for a test.  The data is the test's own (xproblem with
step_seed), the oracle oracle/al_oracle.py over the rows of tests/al_xbounds_oracle.py (oracle_xstep); the sums of the
inputs go into the file, so that the test can tell a file that belongs to other inputs.

    python tests/golden/make_golden_al_given_xbounds.py        (from the repository root, no GPU needed)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import test_gpu_al_given_xbounds as t  # noqa: E402
from oracle import al_oracle  # noqa: E402

if __name__ == "__main__":
    for n, m, T, B in t.RECORDED:
        p = t.xproblem(n, m, T, B=B, seed=t.step_seed(n, m, T))
        upd, L, info = t.oracle_xstep(p)
        assert not info.any()
        sol = al_oracle.chol_solve_neg(L, p["rhs"].reshape(B, -1))
        sums = {"sum_" + k: p[k].sum() for k in ("xu", "lam", "xl", "xh", "Jx", "rhs")}
        np.savez(t.GOLDEN % (n, m, T, B), upd=upd, sol=sol, info=info, **sums)
        print(t.GOLDEN % (n, m, T, B), upd.shape)
