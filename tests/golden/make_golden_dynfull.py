#!/usr/bin/env python3
"""Golden vectors for tests/test_gpu_dyn.py::test_vs_compiled_reference_full_size: the reference's CasADi-generated C
(oracle/_ref, built by oracle/Makefile; called through oracle/dyn_ref.py) on the 4000 sampled knots of that test's
B x (T-1) = 4096 x 19 random states, drawn with the test's own seed and sequence.  Stored per robot as
DYNFULL_<robot>_<part>.npz (consecutive slices of the 4000 samples, each file under 1 MiB): sub (the sample indices),
x, u (the inputs), x_next, Jx, Ju (the reference's outputs, dt 0.05).
Build container only; the fixtures are data (inputs + outputs).

Usage:  python tests/golden/make_golden_dynfull.py
"""
import glob
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import dyn_ref  # noqa: E402

N, S, DT = 4096 * 19, 4000, 0.05
MAX_FILE_BYTES = 900 * 1024


def samples(nq):
    """the random states of test_vs_compiled_reference_full_size, in its order of draws"""
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.uniform(-np.pi, np.pi, (N, nq)), rng.uniform(-8, 8, (N, nq))], 1)
    u = rng.uniform(-100, 100, (N, 1))
    sub = rng.choice(N, S, replace=False)
    return x, u, sub


if __name__ == "__main__":
    for robot, nq in dyn_ref.ROBOTS.items():
        assert dyn_ref.available(robot), "oracle/_ref/lib%s.so missing: make -C oracle ref" % robot
        x, u, sub = samples(nq)
        xs, us = x[sub], u[sub]
        xn = dyn_ref.step_x(robot, xs, us, DT)
        Jx, Ju = dyn_ref.jac_x(robot, xs, us, DT)
        n = 2 * nq
        per_sample = 8 * (1 + n + 1 + n + n * n + n)
        parts = -(-S * per_sample // MAX_FILE_BYTES)
        chunk = -(-S // parts)                          # equal slices
        for f in glob.glob(os.path.join(HERE, "DYNFULL_%s_*.npz" % robot)):
            os.remove(f)
        for part, a in enumerate(range(0, S, chunk)):
            b = min(S, a + chunk)
            np.savez(os.path.join(HERE, "DYNFULL_%s_%d.npz" % (robot, part)), sub=sub[a:b], x=xs[a:b], u=us[a:b],
                     x_next=xn[a:b], Jx=Jx[a:b], Ju=Ju[a:b])
        print(robot, "ok", part + 1, "file(s)")
