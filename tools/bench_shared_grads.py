"""QPFunction forward + backward with Q, G, A shared by the batch: the device reduction of the shared gradients
(qp.REDUCE_SHARED_GRADS = True, dqp_qp_backward_shared) against per-sample gradients + .mean(0) (False), in one process.

    python tools/bench_shared_grads.py [--root TREE] [--runs 7] [--medians 5] [--warmup 5]

HIP events around forward + backward; every figure is a median of `--runs` timed iterations after `--warmup` untimed
ones, and that median is taken `--medians` times over: the spread of those repeated medians is the noise floor a
difference has to clear.  Also: backward alone, peak memory of one iteration (torch.cuda.max_memory_allocated), and the
library-trace time of the two reduction kernels.  `--root TREE` imports the package from another checkout (e.g. the
parent commit, built), which has no switch: only the per-sample path is timed there.  One JSON line per shape.
"""
import argparse
import json
import os
import statistics
import sys

SHAPES = [(30, 30, 15, 4096), (100, 100, 0, 128)]


def problem(torch, nz, nineq, neq, B):
    g = torch.Generator().manual_seed(nz + B)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    L = rn(nz, nz)
    Q = L @ L.T + 1e-3 * torch.eye(nz, dtype=torch.float64)
    G, A, p, z0 = rn(nineq, nz), rn(neq, nz), rn(B, nz), rn(B, nz)
    h = z0 @ G.T + torch.rand(B, nineq, generator=g, dtype=torch.float64)
    b = z0 @ A.T
    ins = [t.cuda().requires_grad_() for t in (Q, p, G, h)]
    ins += [A.cuda().requires_grad_(), b.cuda().requires_grad_()] if neq else [torch.Tensor().cuda(), torch.Tensor().cuda()]
    return ins


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--medians", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    assert a.runs >= 5
    sys.path.insert(0, a.root)
    import torch
    import diff_qp_mpc_amd as dqp
    from diff_qp_mpc_amd import _lib, qp as qpmod
    has_switch = hasattr(qpmod, "REDUCE_SHARED_GRADS")

    for nz, nineq, neq, B in SHAPES:
        ins = problem(torch, nz, nineq, neq, B)
        fn = dqp.QPFunction(check_Q_spd=False, verbose=-1)
        ct = torch.randn(B, nz, dtype=torch.float64, device="cuda")

        def step(timed):
            for t in ins:
                t.grad = None
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            e[0].record()
            z = fn(*ins)
            e[1].record()
            z.backward(ct)
            e[2].record()
            if not timed:
                return None
            torch.cuda.synchronize()
            return e[0].elapsed_time(e[2]), e[1].elapsed_time(e[2])

        out = {"shape": [nz, nineq, neq], "B": B, "root": a.root}
        for switch in ((True, False) if has_switch else (False,)):
            if has_switch:
                qpmod.REDUCE_SHARED_GRADS = switch
            for _ in range(a.warmup):
                step(False)
            torch.cuda.synchronize()
            total, bwd = [], []
            for _ in range(a.medians):
                r = [step(True) for _ in range(a.runs)]
                total.append(statistics.median(x[0] for x in r))
                bwd.append(statistics.median(x[1] for x in r))
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            step(True)
            key = "reduce" if switch else "per_sample"
            out[key] = {"fwd_bwd_ms_medians": [round(x, 4) for x in total],
                        "fwd_bwd_ms": round(statistics.median(total), 4),
                        "fwd_bwd_ms_spread": round(max(total) - min(total), 4),
                        "bwd_ms": round(statistics.median(bwd), 4),
                        "bwd_ms_spread": round(max(bwd) - min(bwd), 4),
                        "max_memory_allocated": torch.cuda.max_memory_allocated()}
            if switch:
                with _lib.trace(64) as tr:
                    step(True)
                out[key]["trace_ms"] = {k.split("(")[0].split("::")[-1]: round(ms, 4) for k, (c, ms) in
                                        tr.by_kernel().items() if "shared_grad" in k}
        if has_switch:
            qpmod.REDUCE_SHARED_GRADS = True
        print(json.dumps(out))


if __name__ == "__main__":
    main()
