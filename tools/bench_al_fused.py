#!/usr/bin/env python3
"""AL_mpc.MPC forward + backward with the single-launch solve (AL_mpc.PERSISTENT_SOLVE, dqp_al_mpc_solve_fused) off
and on, in the same process, eager and under hipGraph replay (AL_mpc.GraphedMPC), on registered device models.

The switch-off rows are the multi-launch path (dqp_al_mpc_solve) and the comparator.  Per shape and mode the two
variants alternate in blocks of `--block` calls; a block is timed with a host clock around work that ends in a device
synchronise, the figure is the median over the blocks, with the quartiles as the spread.  A library trace of one
forward per variant gives the launch count and the per-kernel device time.

    python tools/bench_al_fused.py [--reps 30] [--block 20] [--state-box] [--shapes robot:T:B,...] [--out FILE.json]

--state-box puts an active per-sample, per-knot state box (x_lower / x_upper) on every problem: the switch-off rows are
then dqp_al_mpc_solve_xbounds and the switch-on rows dqp_al_mpc_solve_fused_xbounds; each row records how many samples
end the traced call with a positive state multiplier.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from diff_qp_mpc_amd import AL_mpc, al_utils, _lib
from diff_qp_mpc_amd.dynamics import DeviceDynamics

SHAPES = [("pendulum_euler", 5, 128), ("cartpole1l", 20, 128), ("cartpole2l", 5, 128),
          ("cartpole2l", 5, 32), ("cartpole2l", 5, 512), ("cartpole2l", 5, 2048), ("cartpole2l", 5, 8192)]


def dev(a):
    return torch.tensor(np.asarray(a), dtype=torch.float64, device="cuda")


def setup(robot, T, B, state_box=False):
    dyn = DeviceDynamics(robot)
    nx, nu = dyn.n_state, dyn.n_ctrl
    lim = 2.0 if robot == "pendulum_euler" else 250.0
    lo, hi = dev(np.full(nu, -lim)), dev(np.full(nu, lim))
    r = np.random.default_rng(0)
    x0 = dev(r.uniform(-0.5, 0.5, (B, nx)))
    Qd = dev(np.concatenate([np.ones(nx), 1e-3 * np.ones(nu)])).repeat(B, T, 1)
    x_ref = x0[:, None, :] * torch.linspace(1.0, 0.0, T, dtype=torch.float64, device="cuda")[None, :, None]
    u_ref = torch.zeros(B, T, nu, dtype=torch.float64, device="cuda")
    C = torch.diag_embed(Qd).requires_grad_()
    c = (-(Qd * torch.cat([x_ref, u_ref], -1))).clone().requires_grad_()
    box = {}
    if state_box:
        # around the reference line, 60 % of |x0| wide below and 18 % above at knot 1, narrowing along the horizon: knot 0
        # (pinned to x0) stays inside, later knots are cut where the solution swings past the line
        w = 0.6 * x0.abs().amax(1)[:, None, None] * torch.linspace(1.0, 0.25, T, dtype=torch.float64, device="cuda")[None, :, None]
        w = (w + 0.02).expand(B, T, nx).clone()
        w[:, 0] = x0.abs().amax(1)[:, None] + 0.05
        box = dict(x_lower=(x_ref - w).contiguous(), x_upper=(x_ref + 0.3 * w).contiguous())

    def make():
        ctrl = AL_mpc.MPC(nx, nu, T, u_lower=lo, u_upper=hi, n_batch=B, verbose=0, solver_type="dense", dtype=torch.float64,
                          eps=1e-5, exit_unconverged=False, backprop=False, **box)
        ctrl.mask = torch.ones(B, T, 1, device="cuda")
        return ctrl
    return dyn, make, x0, x_ref, u_ref, C, c


def set_switch(on):
    AL_mpc.PERSISTENT_SOLVE = on
    AL_mpc.PERSISTENT_SOLVE_MAX_BATCH = 1 << 30


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30, help="timed blocks per variant")
    ap.add_argument("--block", type=int, default=20, help="calls per timed block")
    ap.add_argument("--state-box", action="store_true", help="an active (B, T, n) state box on every problem")
    ap.add_argument("--shapes", default=None, help="robot:T:B,... instead of the built-in list")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    try:
        clocks = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=30).stdout
    except Exception as e:      # noqa: BLE001
        clocks = "rocm-smi --showclocks: %r" % (e,)
    result = {"device": torch.cuda.get_device_name(0), "clocks": clocks, "reps": args.reps, "block": args.block,
              "state_box": args.state_box, "rows": []}
    shapes = SHAPES
    if args.shapes:
        shapes = [(r, int(T), int(B)) for r, T, B in (s.split(":") for s in args.shapes.split(","))]
    for robot, T, B in shapes:
        dyn, make, x0, x_ref, u_ref, C, c = setup(robot, T, B, args.state_box)
        ctrl = make()

        def eager():
            ctrl.reinitialize(x0, ctrl.mask)
            ctrl.x_init, ctrl.u_init = x_ref, u_ref
            x, u = ctrl(x0, al_utils.QuadCost(C, c), dyn, dyn.jac)
            torch.autograd.grad(x.double().sum() + 2.0 * u.double().sum(), (C, c))

        graphs = {}
        for on in (False, True):
            set_switch(on)
            graphs[on] = AL_mpc.GraphedMPC(make(), (x0, C, c), dyn, x_init=x_ref, u_init=u_ref)

        def graphed(on):
            x, u = graphs[on](x0, C, c)
            torch.autograd.grad(x.double().sum() + 2.0 * u.double().sum(), (C, c))

        row = {"robot": robot, "T": T, "B": B}
        # launches and device time of the forward solve, one traced call per variant
        for on in (False, True):
            set_switch(on)
            eager()
            torch.cuda.synchronize()
            ctrl.reinitialize(x0, ctrl.mask)
            ctrl.x_init, ctrl.u_init = x_ref, u_ref
            with _lib.trace() as tr:
                ctrl(x0, al_utils.QuadCost(C, c), dyn, dyn.jac)
            key = "fused" if on else "multi"
            row[key + "_launches"] = len(tr.records)
            row[key + "_kernel_ms_sum"] = sum(ms for _, ms in tr.records)
            short = lambda k: k.replace("(anonymous namespace)::", "").split("(")[0][-60:]
            row[key + "_kernels"] = {short(k): (n, round(ms, 5)) for k, (n, ms) in tr.by_kernel().items()}
            if args.state_box:
                nu = dyn.n_ctrl
                row[key + "_samples_with_active_state_rows"] = int((ctrl.lamda_prev[:, T * (dyn.n_state + 2 * nu):] > 0).any(1).sum())
        for mode in ("eager", "graph"):
            times = {False: [], True: []}
            for on in (False, True):            # warm-up of both variants
                set_switch(on)
                for _ in range(args.block):
                    eager() if mode == "eager" else graphed(on)
            torch.cuda.synchronize()
            for _ in range(args.reps):          # alternate the variants block by block
                for on in (False, True):
                    set_switch(on)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.block):
                        eager() if mode == "eager" else graphed(on)
                    torch.cuda.synchronize()
                    times[on].append((time.perf_counter() - t0) / args.block * 1e3)
            for on in (False, True):
                q = statistics.quantiles(times[on], n=4)
                key = "%s_%s_ms" % (mode, "fused" if on else "multi")
                row[key] = {"median": statistics.median(times[on]), "q1": q[0], "q3": q[2]}
        set_switch(False)
        result["rows"].append(row)
        print("%-15s T=%-3d B=%-5d | eager multi %.3f fused %.3f ms | graph multi %.3f fused %.3f ms | launches %d -> %d, "
              "kernel time %.3f -> %.3f ms" % (robot, T, B, row["eager_multi_ms"]["median"], row["eager_fused_ms"]["median"],
                                                row["graph_multi_ms"]["median"], row["graph_fused_ms"]["median"],
                                                row["multi_launches"], row["fused_launches"], row["multi_kernel_ms_sum"],
                                                row["fused_kernel_ms_sum"]), flush=True)
    AL_mpc.PERSISTENT_SOLVE = False
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps({"rows": len(result["rows"])}))


if __name__ == "__main__":
    main()
