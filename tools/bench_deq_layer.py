#!/usr/bin/env python3
"""One policies.DEQLayer call with FUSED_DEQ_LAYER off (the torch path) and on (csrc/dqp_deq.hip), same process,
alternating off / on / off / on, at the config-5 size (B 65536, hdim 128, T 5, nx 6) and at the reference's training
batch (B 128):

  - forward and forward + backward: device-event time per call, median and spread (min, max, inter-quartile) of REPS
    timed repetitions after WARMUP untimed ones;
  - the summed device time of the kernels that are not GEMMs in one forward + backward (torch.profiler, as
    tools/cfg5_torch_breakdown.py reads it), median and spread over PROF_REPS profiled calls per variant;
  - the library's own trace of the fused kernels (dqp_trace_begin / _end) and their achieved GB/s against the bytes the
    algorithm needs: stage B moves 4 tensors forward and 6 backward, stage A 2 and 3, of nrows * hdim * 4 bytes each.

  - the config-5 training step at --graph-step-batch as ONE hipGraph (policies.GraphedTrainStep through bench.py's
    DEQMPCTrain), captured once with the flag off and once with it on, replays alternating: where the host no longer
    counts, the small-batch kernels do.

    python tools/bench_deq_layer.py [--batch 65536 128] [--hdim 128] [--reps 20] [--graph-step-batch 128]
"""
import argparse, os, statistics, sys, types
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from torch.profiler import profile, ProfilerActivity
from diff_qp_mpc_amd import _lib, policies

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, nargs="+", default=[65536, 128])
ap.add_argument("--hdim", type=int, default=128)
ap.add_argument("--T", type=int, default=5)
ap.add_argument("--nx", type=int, default=6)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--prof-reps", type=int, default=5)
ap.add_argument("--graph-step-batch", type=int, default=128, help="0: skip the graphed training step")
a = ap.parse_args()
assert torch.cuda.is_available(), "bench_deq_layer.py measures on a GPU"
dev = torch.device("cuda:0")
GEMM = ("Cijk_", "gemm", "Gemm", "GEMM", "rocblas", "hipblas")


def spread(xs):
    xs = sorted(xs)
    q = statistics.quantiles(xs, n=4) if len(xs) >= 4 else [xs[0], statistics.median(xs), xs[-1]]
    return "median %.4f  min %.4f  max %.4f  iqr %.4f  (n %d)" % (statistics.median(xs), xs[0], xs[-1], q[2] - q[0], len(xs))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def non_gemm_ms(fn):
    """(summed device ms of the non-GEMM kernels of one fn(), {kernel: ms})"""
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        fn(); torch.cuda.synchronize()
    per = {}
    for e in prof.key_averages():
        if e.device_type == torch.autograd.DeviceType.CUDA and e.self_device_time_total > 0 and not e.key.lower().startswith("memcpy"):
            per[e.key] = per.get(e.key, 0.0) + e.self_device_time_total * 1e-3
    return sum(t for k, t in per.items() if not any(s in k for s in GEMM)), per


for B in a.batch:
    env = types.SimpleNamespace(nx=a.nx, nu=1, dt=0.03)
    args = argparse.Namespace(T=a.T, nq=a.nx // 2, hdim=a.hdim, layer_type="mlp", deq_out_type=1)
    torch.manual_seed(0)
    layer = policies.DEQLayer(args, env).to(dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(B, layer.in_dim, device=dev, generator=gen)
    z = torch.randn(B, a.hdim, device=dev, generator=gen)
    w = torch.randn(B, a.hdim, device=dev, generator=gen)

    def fwd(flag):
        policies.FUSED_DEQ_LAYER = flag
        with torch.no_grad():
            return layer(x, z)

    def fwd_bwd(flag):
        policies.FUSED_DEQ_LAYER = flag
        layer.zero_grad(set_to_none=True)
        ref, z_out = layer(x, z)
        (ref.sum() + (z_out * w).sum()).backward()

    print("== DEQLayer B=%d hdim=%d T=%d nx=%d" % (B, a.hdim, a.T, a.nx))
    for name, fn in (("forward", fwd), ("forward+backward", fwd_bwd)):
        for _ in range(a.warmup):
            fn(False); fn(True)
        torch.cuda.synchronize()
        t = {False: [], True: []}
        for _ in range(a.reps):
            for flag in (False, True):           # off / on / off / on
                t[flag].append(timed(lambda: fn(flag)))
        print("%-17s ms  flag off: %s" % (name, spread(t[False])))
        print("%-17s ms  flag on : %s" % (name, spread(t[True])))
    ng, per = {False: [], True: []}, {}
    for _ in range(a.prof_reps):
        for flag in (False, True):
            s, per[flag] = non_gemm_ms(lambda: fwd_bwd(flag))
            ng[flag].append(s)
    print("non-GEMM kernels, forward+backward, ms  flag off: %s" % spread(ng[False]))
    print("non-GEMM kernels, forward+backward, ms  flag on : %s" % spread(ng[True]))
    for flag in (False, True):
        print("  kernels of the last profiled call, flag %s:" % ("on" if flag else "off"))
        for k, ms in sorted(per[flag].items(), key=lambda kv: -kv[1])[:14]:
            print("    %8.4f ms  %s%s" % (ms, "[GEMM] " if any(s in k for s in GEMM) else "", k[:110]))
    # the library's own per-launch timing of the fused kernels, and their byte rates
    recs = []
    for _ in range(a.prof_reps):
        with _lib.trace(64) as tr:
            fwd_bwd(True); torch.cuda.synchronize()
        recs.append(tr.by_kernel())
    tensors = {"deq_res_forward": 4, "deq_res_backward": 6, "deq_ln_forward": 2, "deq_ln_backward": 3}
    for k in sorted(recs[-1]):
        ms = statistics.median(r[k][1] for r in recs if k in r)
        n = next((v for s, v in tensors.items() if s in k), None)
        rate = "  %.0f GB/s of %d x nrows x hdim x 4 B" % (n * B * a.hdim * 4 / ms / 1e6, n) if n else ""
        print("  trace: %d x %.4f ms  %s%s" % (recs[-1][k][0], ms, k[:80], rate))
if a.graph_step_batch:
    import bench
    wl = {}
    for flag in (False, True):          # the flag is read while the step is captured
        policies.FUSED_DEQ_LAYER = flag
        wl[flag] = bench.DEQMPCTrain(torch, dev, 0, 1, argparse.Namespace(batch=a.graph_step_batch, graph=True, robot=None, T=None))
    for _ in range(a.warmup):
        wl[False].step(); wl[True].step()
    torch.cuda.synchronize()
    t = {False: [], True: []}
    for _ in range(a.reps):
        for flag in (False, True):
            t[flag].append(timed(lambda: [wl[flag].step() for _ in range(5)]) / 5)
    print("== graphed DEQ-MPC training step, cartpole-2 B=%d hdim=128 T=5 deq_iter=6 (5 replays per sample)" % a.graph_step_batch)
    print("step ms  flag off: %s" % spread(t[False]))
    print("step ms  flag on : %s" % spread(t[True]))
policies.FUSED_DEQ_LAYER = False
