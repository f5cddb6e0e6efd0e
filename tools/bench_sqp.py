#!/usr/bin/env python3
"""qp_wrapper.MPC.forward (no backward) on registered device models with qp_wrapper.ONE_CALL_SQP off and on, in the same
process: off is the Python-driven SQP loop (torch linearisation, one QP and one line-search launch per round, the
bookkeeping in torch ops, two host reads per round), on is dqp_mpc_sqp_rounds (csrc/dqp_mpc_sqp.hip) with one host read
per round.

Shapes: pendulum_dx T 10 qp_iter 10 and cartpole1l T 100 qp_iter 20 (the reference's cartpole expert,
deqmpc/datagen_cp1.py:19-97: goal weights (1, 10, 1, 1) on (0, pi, 0, 0), control penalty 1e-4, eps 1e-5, line search
0.2 / 10), each at B 64 and 1024.  Per case the two variants alternate in blocks of `--block` calls after a warm-up of
both; a block is timed with a host clock around work that ends in a device synchronise; the figure is the median over
the `--reps` blocks with the quartiles as the spread (reps * block >= 20 timed calls per variant).  One traced call per
variant gives the launches of the library and their summed device time, and the rounds the solve ran.  One JSON line per
case.

    python tools/bench_sqp.py [--reps 5] [--block 4] [--warmup 4] [--out FILE.json]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from diff_qp_mpc_amd import _lib, qp_wrapper
from diff_qp_mpc_amd.dynamics import DeviceDynamics

CASES = [("pendulum_dx", 10, 10, 64), ("pendulum_dx", 10, 10, 1024), ("cartpole1l", 100, 20, 64), ("cartpole1l", 100, 20, 1024)]
F64 = dict(dtype=torch.float64, device="cuda")


def setup(robot, T, qp_iter, B):
    dyn = DeviceDynamics(robot)
    n, m = dyn.n_state, dyn.n_ctrl
    gen = torch.Generator().manual_seed(0)
    if robot == "pendulum_dx":          # qpth/env_dx/pendulum.py: goal (cos, sin, thdot) = (1, 0, 0), |u| <= 2
        th = (torch.rand(B, generator=gen, dtype=torch.float64) * 2 - 1) * math.pi
        x0 = torch.stack([th.cos(), th.sin(), torch.rand(B, generator=gen, dtype=torch.float64) * 2 - 1], 1).cuda()
        goal, w, pen, lim, eps = torch.tensor([1.0, 0.0, 0.0]), torch.tensor([1.0, 1.0, 0.1]), 1e-3, 2.0, 1e-4
    else:
        x0 = ((torch.rand(B, n, generator=gen, dtype=torch.float64) * 2 - 1) * torch.tensor([0.5, 0.5, 0.2, 0.2])).cuda()
        goal, w, pen, lim, eps = torch.tensor([0.0, math.pi, 0.0, 0.0]), torch.tensor([1.0, 10.0, 1.0, 1.0]), 1e-4, 100.0, 1e-5
    q = torch.cat([w, pen * torch.ones(m)]).double()
    p = torch.cat([-w.sqrt() * goal, torch.zeros(m)]).double()
    C = torch.diag(q)[None, None].repeat(T, B, 1, 1).cuda()
    c = p[None, None].repeat(T, B, 1).cuda()
    one = torch.full((m,), lim, **F64)
    mpc = qp_wrapper.MPC(n, m, T, u_lower=-one, u_upper=one, n_batch=B, verbose=-1, qp_iter=qp_iter, eps=eps,
                         linesearch_decay=0.2, max_linesearch_iter=10, grad_method=qp_wrapper.GradMethods.AUTO_DIFF)
    cost = qp_wrapper.QuadCost(C, c)

    def call():
        with torch.no_grad():
            return mpc(x0, cost, dyn, dyn.jac)
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="timed blocks per variant")
    ap.add_argument("--block", type=int, default=4, help="calls per timed block")
    ap.add_argument("--warmup", type=int, default=4, help="untimed calls per variant")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    assert args.reps * args.block >= 20, "at least 20 timed calls per variant"
    rows = []
    for robot, T, qp_iter, B in CASES:
        call = setup(robot, T, qp_iter, B)
        row = {"robot": robot, "T": T, "qp_iter": qp_iter, "B": B, "device": torch.cuda.get_device_name(0)}
        outs = {}
        for on in (False, True):            # warm-up, then one traced call per variant
            qp_wrapper.ONE_CALL_SQP = on
            for _ in range(args.warmup):
                outs[on] = call()
            torch.cuda.synchronize()
            with _lib.trace(1 << 16) as tr:
                call()
            key = "on" if on else "off"
            names = [k for k, _ in tr.records]
            row[key + "_launches"] = len(names)
            row[key + "_kernel_ms_sum"] = round(sum(ms for _, ms in tr.records), 4)
            # the line-search kernel also runs the initial rollout and the differentiable step's search
            row[key + "_rounds"] = sum("line_search_kernel" in k for k in names) - 2
        row["max_abs_diff_x"] = float((outs[True][0] - outs[False][0]).abs().max())
        row["max_abs_diff_u"] = float((outs[True][1] - outs[False][1]).abs().max())
        times = {False: [], True: []}
        for _ in range(args.reps):          # alternate the variants block by block
            for on in (False, True):
                qp_wrapper.ONE_CALL_SQP = on
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.block):
                    call()
                torch.cuda.synchronize()
                times[on].append((time.perf_counter() - t0) / args.block * 1e3)
        qp_wrapper.ONE_CALL_SQP = False
        for on in (False, True):
            qs = statistics.quantiles(times[on], n=4)
            row["on_ms" if on else "off_ms"] = {"median": round(statistics.median(times[on]), 4), "q1": round(qs[0], 4),
                                                "q3": round(qs[2], 4)}
        row["timed_calls"] = args.reps * args.block
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
