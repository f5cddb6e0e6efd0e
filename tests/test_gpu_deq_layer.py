"""The fused DEQLayer stages on the GPU (csrc/dqp_deq.hip, deq_fused, policies.FUSED_DEQ_LAYER).

Correctness rule, for every output and gradient: the reference is the same expression evaluated by torch in fp64, the
comparator torch's own fp32 path on the same inputs, err(x) = max|x - ref| / max|ref|, and

    err(fused) <= 4 * err(torch fp32)

(the factor allows another summation order over at most 512 terms; a wrong statistic or index is off by 10^3 x and
more).  No absolute tolerance.  Each case prints its ratios.
Then: bit-identical parameter gradients from run to run, the whole DEQLayer with the flag on against off, the reference
policy's golden trajectories, loss and gradients with the flag on (hdim 32: two rows per wavefront), and the training
step captured as a hipGraph with the flag on."""
import argparse
import copy
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HDIMS = (32, 64, 128, 512)
NROWS = (1, 3, 65, 1030)     # odd rows at two rows per wavefront, the row tail, several workgroups and partials
EPS = 1e-5


def _err(x, ref):
    top = float(ref.abs().max())        # 0: a gradient that is zero in exact arithmetic (one constant row); then |x - 0|
    return float((x.double() - ref).abs().max()) / (top if top > 0 else 1.0)


def _check(tag, fused, plain, ref):
    """the ratio rule on dicts of tensors; prints the figures before it asserts"""
    bad = []
    for k in ref:
        ef, ep = _err(fused[k], ref[k]), _err(plain[k], ref[k])
        print("%s %-8s err fused %.3e  torch fp32 %.3e  ratio %s" % (tag, k, ef, ep, "%.2f" % (ef / ep) if ep > 0 else "-"))
        if not ef <= 4 * ep:
            bad.append((k, ef, ep))
    assert not bad, (tag, bad)


def _params(h, gen, n):
    return [(torch.randn(h, device="cuda", generator=gen) * 0.5 + (1.0 if i % 2 == 0 else 0.0)) for i in range(n)]


def _special_rows(nrows):
    """(row whose ReLU input is all negative or None, row with exact zeros at the ReLU)"""
    return (1, 2) if nrows >= 3 else (None, 0)


def _stage_a_inputs(h, nrows, seed=0):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    a = torch.randn(nrows, h, device="cuda", generator=gen)
    neg, zero = _special_rows(nrows)
    if neg is not None:
        a[neg] = -a[neg].abs() - 0.1         # zero variance behind the ReLU: rstd = 1 / sqrt(eps)
    a[zero, ::3] = 0.0
    gamma, beta = _params(h, gen, 2)
    dy = torch.randn(nrows, h, device="cuda", generator=gen)
    return a, gamma, beta, dy


def _stage_a_torch(a, gamma, beta, dy, relu, dtype):
    a, gamma, beta = [t.detach().to(dtype).clone().requires_grad_() for t in (a, gamma, beta)]
    y = F.layer_norm(F.relu(a) if relu else a, a.shape[-1:], gamma, beta, EPS)
    y.backward(dy.to(dtype))
    return {"y": y.detach(), "da": a.grad, "dgamma": gamma.grad, "dbeta": beta.grad}


def _stage_a_fused(a, gamma, beta, dy, relu):
    from diff_qp_mpc_amd import deq_fused
    a, gamma, beta = [t.clone().requires_grad_() for t in (a, gamma, beta)]
    y = deq_fused.LayerNormStage.apply(a, gamma, beta, EPS, relu)
    y.backward(dy)
    return {"y": y.detach(), "da": a.grad, "dgamma": gamma.grad, "dbeta": beta.grad}


def _stage_b_inputs(h, nrows, seed=0):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    xi, a2, z1 = [torch.randn(nrows, h, device="cuda", generator=gen) for _ in range(3)]
    g2, b2, g3, b3 = _params(h, gen, 4)
    neg, zero = _special_rows(nrows)
    if neg is not None:
        z1[neg] = -50.0                      # z1 + LN2(.) < 0 everywhere: zero variance at LN3
    # exact zeros at the ReLU in every arithmetic: a constant row xi + a2 makes LN2's output exactly beta2
    xi[zero] = 0.25
    a2[zero] = 0.25
    z1[zero, ::3] = -b2[::3]
    dz2 = torch.randn(nrows, h, device="cuda", generator=gen)
    return xi, a2, z1, g2, b2, g3, b3, dz2


def _stage_b_torch(xi, a2, z1, g2, b2, g3, b3, dz2, dtype):
    xi, a2, z1, g2, b2, g3, b3 = [t.detach().to(dtype).clone().requires_grad_() for t in (xi, a2, z1, g2, b2, g3, b3)]
    hs = xi.shape[-1:]
    z2 = F.layer_norm(F.relu(z1 + F.layer_norm(xi + a2, hs, g2, b2, EPS)), hs, g3, b3, EPS)
    z2.backward(dz2.to(dtype))
    return {"z2": z2.detach(), "dxi": xi.grad, "da2": a2.grad, "dz1": z1.grad, "dgamma2": g2.grad, "dbeta2": b2.grad,
            "dgamma3": g3.grad, "dbeta3": b3.grad}


def _stage_b_fused(xi, a2, z1, g2, b2, g3, b3, dz2):
    from diff_qp_mpc_amd import deq_fused
    xi, a2, z1, g2, b2, g3, b3 = [t.clone().requires_grad_() for t in (xi, a2, z1, g2, b2, g3, b3)]
    z2 = deq_fused.ResidualStage.apply(xi, a2, z1, g2, b2, g3, b3, EPS, EPS)
    z2.backward(dz2)
    return {"z2": z2.detach(), "dxi": xi.grad, "da2": a2.grad, "dz1": z1.grad, "dgamma2": g2.grad, "dbeta2": b2.grad,
            "dgamma3": g3.grad, "dbeta3": b3.grad}


@pytest.mark.parametrize("nrows", NROWS)
@pytest.mark.parametrize("h", HDIMS)
@pytest.mark.parametrize("relu", [0, 1])
def test_stage_a_against_fp64(h, nrows, relu):
    a, gamma, beta, dy = _stage_a_inputs(h, nrows)
    fused = _stage_a_fused(a, gamma, beta, dy, relu)
    if relu and nrows >= 3:                  # the all-negative row: y = beta, no gradient to a
        assert torch.equal(fused["y"][1], beta) and not bool(fused["da"][1].any())
    _check("A h%d n%d relu%d" % (h, nrows, relu), fused, _stage_a_torch(a, gamma, beta, dy, relu, torch.float32),
           _stage_a_torch(a, gamma, beta, dy, relu, torch.float64))


@pytest.mark.parametrize("nrows", NROWS)
@pytest.mark.parametrize("h", HDIMS)
def test_stage_b_against_fp64(h, nrows):
    ins = _stage_b_inputs(h, nrows)
    fused = _stage_b_fused(*ins)
    assert torch.equal(fused["dxi"], fused["da2"])
    neg, zero = _special_rows(nrows)
    assert not bool(fused["dz1"][zero, ::3].any())          # exact zeros at the ReLU pass no gradient
    if neg is not None:
        assert torch.equal(fused["z2"][neg], ins[6]) and not bool(fused["dz1"][neg].any())
    _check("B h%d n%d" % (h, nrows), fused, _stage_b_torch(*ins, torch.float32), _stage_b_torch(*ins, torch.float64))


def test_hdim_256_one_16_byte_access_per_lane():
    """the fifth supported width, which the table above leaves out: both stages at 65 rows, same rule"""
    a, gamma, beta, dy = _stage_a_inputs(256, 65)
    _check("A h256 n65 relu1", _stage_a_fused(a, gamma, beta, dy, 1), _stage_a_torch(a, gamma, beta, dy, 1, torch.float32),
           _stage_a_torch(a, gamma, beta, dy, 1, torch.float64))
    ins = _stage_b_inputs(256, 65)
    _check("B h256 n65", _stage_b_fused(*ins), _stage_b_torch(*ins, torch.float32), _stage_b_torch(*ins, torch.float64))


@pytest.mark.parametrize("h", HDIMS)
def test_parameter_gradients_are_bit_identical_from_run_to_run(h):
    a, gamma, beta, dy = _stage_a_inputs(h, 1030, seed=1)
    r1, r2 = _stage_a_fused(a, gamma, beta, dy, 1), _stage_a_fused(a, gamma, beta, dy, 1)
    for k in ("dgamma", "dbeta", "da"):
        assert torch.equal(r1[k], r2[k]), k
    ins = _stage_b_inputs(h, 1030, seed=1)
    r1, r2 = _stage_b_fused(*ins), _stage_b_fused(*ins)
    for k in ("dgamma2", "dbeta2", "dgamma3", "dbeta3", "dxi", "dz1"):
        assert torch.equal(r1[k], r2[k]), k


def _count_fused_calls(monkeypatch):
    from diff_qp_mpc_amd import _lib
    seen, call = {}, _lib.call

    def counting(name, *args):
        seen[name] = seen.get(name, 0) + 1
        return call(name, *args)
    monkeypatch.setattr(_lib, "call", counting)
    return seen


def test_whole_layer_flag_on_against_off(monkeypatch):
    from diff_qp_mpc_amd import policies
    B, hdim, T, nx = 257, 128, 5, 6
    env = types.SimpleNamespace(nx=nx, nu=1, dt=0.05)
    args = argparse.Namespace(T=T, nq=nx // 2, hdim=hdim, layer_type="mlp", deq_out_type=1)
    torch.manual_seed(0)
    layer = policies.DEQLayer(args, env).to("cuda")
    with torch.no_grad():                    # non-trivial affine parameters
        for ln in (layer.inp_layer[1], layer.lndeq1, layer.lndeq2, layer.lndeq3):
            ln.weight.add_(0.3 * torch.randn_like(ln.weight))
            ln.bias.add_(0.3 * torch.randn_like(ln.bias))
    gen = torch.Generator(device="cuda").manual_seed(2)
    x = torch.randn(B, layer.in_dim, device="cuda", generator=gen)
    z = torch.randn(B, hdim, device="cuda", generator=gen)
    w1 = torch.randn(B, T - 1, nx, device="cuda", generator=gen)
    w2 = torch.randn(B, hdim, device="cuda", generator=gen)

    def run(mod, dtype):
        mod.zero_grad(set_to_none=True)
        ref, z_out = mod(x.to(dtype), z.to(dtype))
        ((ref * w1.to(dtype)).sum() + (z_out * w2.to(dtype)).sum()).backward()
        out = {"x_ref": ref.detach(), "z_out": z_out.detach()}
        out.update({"d" + k: p.grad.clone() for k, p in mod.named_parameters()})
        return out

    plain = run(layer, torch.float32)
    exact = run(copy.deepcopy(layer).double(), torch.float64)
    seen = _count_fused_calls(monkeypatch)
    monkeypatch.setattr(policies, "FUSED_DEQ_LAYER", True)
    fused = run(layer, torch.float32)
    assert seen == {"dqp_deq_ln_forward": 2, "dqp_deq_res_forward": 1, "dqp_deq_ln_backward": 2, "dqp_deq_res_backward": 1}
    assert len(exact) == 2 + len(list(layer.parameters()))
    _check("layer", fused, plain, exact)


def make_policy(g, B, solver_type="al"):
    from diff_qp_mpc_amd import policies
    from diff_qp_mpc_amd.dynamics import DeviceDynamics
    dyn = DeviceDynamics("pendulum_euler", dt=float(g["dt"]))
    env = types.SimpleNamespace(nx=2, nu=1, nq=1, dt=float(g["dt"]), dynamics=dyn, dynamics_derivatives=dyn.jac,
                                action_space=types.SimpleNamespace(high=g["u_upper"], low=g["u_lower"]))
    args = argparse.Namespace(T=int(g["T"]), nq=1, hdim=int(g["hdim"]), layer_type="mlp", deq_out_type=1,
                              policy_out_type=1, deq_iter=int(g["deq_iter"]), solver_type=solver_type, qp_iter=1,
                              eps=1e-2, warm_start=True, bsz=B, Q=torch.tensor(g["Q"]), R=torch.tensor(g["R"]),
                              dtype="double", device="cuda")
    torch.manual_seed(0)
    policy = policies.DEQMPCPolicy(args, env)
    sd = {k[2:]: torch.tensor(v) for k, v in g.items() if k.startswith("w_")}
    policy.model.load_state_dict(sd)                 # the reference's own state-dict keys
    return policies, policy


def test_deqmpc_policy_vs_reference_with_the_fused_layer(monkeypatch):
    """the body of test_gpu_policies.test_deqmpc_policy_vs_reference, at its tolerances, with the flag on"""
    from diff_qp_mpc_amd import policies as pol
    monkeypatch.setattr(pol, "FUSED_DEQ_LAYER", True)
    seen = _count_fused_calls(monkeypatch)
    g = dict(np.load(os.path.join(GOLDEN, "DEQMPC_pendulum_T5_b6.npz")))
    assert int(g["hdim"]) == 32
    B = g["x"].shape[0]
    policies, policy = make_policy(g, B)
    f32 = lambda a: torch.tensor(a, dtype=torch.float32, device="cuda")
    x, gs, ga, mask = f32(g["x"]), f32(g["gt_states"]), f32(g["gt_actions"]), f32(g["mask"])
    trajs, dyn_res = policy(x, gs, ga, mask, qp_solve=True)
    assert len(trajs) == int(g["deq_iter"])
    for i, (net, xs, us) in enumerate(trajs):
        np.testing.assert_allclose(net.detach().cpu().numpy(), g["it%d_net" % i], rtol=1e-3, atol=2e-4, err_msg="net %d" % i)
        np.testing.assert_allclose(xs.detach().cpu().numpy(), g["it%d_x" % i], rtol=1e-3, atol=2e-4, err_msg="x %d" % i)
        np.testing.assert_allclose(us.detach().cpu().numpy(), g["it%d_u" % i], rtol=1e-3, atol=2e-4, err_msg="u %d" % i)
    loss, loss_end = policies.compute_loss_deqmpc(policy, gs, ga, mask, trajs)
    np.testing.assert_allclose(float(loss.detach()), float(g["loss"]), rtol=1e-4)
    np.testing.assert_allclose(float(loss_end.detach()), float(g["loss_end"]), rtol=1e-4)
    policy.zero_grad()
    loss.backward()
    for k, p in policy.model.named_parameters():
        ref = g["g_" + k]
        got = p.grad.cpu().numpy() if p.grad is not None else np.zeros_like(ref)
        np.testing.assert_allclose(got, ref, rtol=2e-2, atol=2e-3 * max(np.abs(ref).max(), 1e-3), err_msg=k)
    n = int(g["deq_iter"])
    assert seen.get("dqp_deq_res_forward") == n and seen.get("dqp_deq_ln_forward") == 2 * n
    assert seen.get("dqp_deq_res_backward") == n and seen.get("dqp_deq_ln_backward") == 2 * n


def _train_losses(mode, g, B, T, x, gs, ga, mask, steps=4):
    policies, policy = make_policy(g, B)
    opt = torch.optim.Adam(policy.model.parameters(), lr=3e-3, capturable=True)
    step = None
    if mode == "graph":
        w0 = {k: v.clone() for k, v in policy.model.state_dict().items()}
        step = policies.GraphedTrainStep(policy, opt, x, gs, ga, mask, warmup=2)
        assert step.step_in_graph
        policy.model.load_state_dict(w0)            # warm-up ran optimiser steps: weights and Adam state back to the start
        for st in opt.state.values():
            for v in st.values():
                v.zero_()
        run = lambda: step(x, gs, ga, mask)
    else:
        run = lambda: policies.train_step(policy, opt, x, gs, ga, mask)
    losses = [float(run()[0]) for _ in range(steps)]
    if step is not None:
        assert not step.failed()
    return losses


def test_graphed_train_step_with_the_fused_layer(monkeypatch):
    """GraphedTrainStep with the flag on: the fused stages only enqueue, so the captured step replays them; losses of
    four successive optimiser steps against the eager step with the flag on, at the rtol of
    test_graphed_train_step_matches_eager."""
    from diff_qp_mpc_amd import policies as pol
    monkeypatch.setattr(pol, "FUSED_DEQ_LAYER", True)
    seen = _count_fused_calls(monkeypatch)
    g = dict(np.load(os.path.join(GOLDEN, "DEQMPC_pendulum_T5_b6.npz")))
    B, T = 128, int(g["T"])
    gen = torch.Generator(device="cuda").manual_seed(0)
    x = torch.rand(B, 2, device="cuda", generator=gen) - 0.5
    gs = x[:, None, :] * torch.linspace(1, 0, T, device="cuda")[None, :, None]
    ga = torch.zeros(B, T, 1, device="cuda")
    mask = torch.ones(B, T, device="cuda")
    eager = _train_losses("eager", g, B, T, x, gs, ga, mask)
    assert seen.get("dqp_deq_res_backward", 0) > 0
    graph = _train_losses("graph", g, B, T, x, gs, ga, mask)
    print("eager", eager, "graph", graph)
    np.testing.assert_allclose(graph, eager, rtol=1e-6)
    assert graph[-1] < graph[0]
