"""The DEQLayer's LayerNorm stages on the fused fp32 kernels of csrc/dqp_deq.hip (include/dqp.h, "network-side
kernels"): what policies.DEQLayer runs between its three GEMMs when policies.FUSED_DEQ_LAYER is on.

    layer_norm(a, ln, relu)            ln(relu(a)) or ln(a)                    stage A: one pass forward, one backward
    residual_block(xi, a2, z1, ln2, ln3)   ln3(relu(z1 + ln2(xi + a2)))        stage B: the same

Both are once-differentiable autograd Functions that save their inputs and the per-row statistics (mean, rstd) only; the
backward recomputes the intermediates.  usable() is the permission test: CUDA fp32 activations of a supported width and
LayerNorms with an element-wise affine; callers run their torch code otherwise.
"""
import torch
from torch.autograd.function import once_differentiable

from . import _lib


def _dims(t):
    h = t.shape[-1]
    return _lib.dqp_deq_dims(t.numel() // h, h)


def _dense(t):
    """contiguous and 16-byte aligned, as the entries read it"""
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _scratch(d, like, want):
    if not want:
        return None
    return torch.empty(_lib.load().dqp_deq_partial_bytes(d) // 4, dtype=torch.float32, device=like.device)


def usable(lns, tensors):
    """the fused stages serve these LayerNorms on these activations"""
    if tensors[0].dim() < 1 or tensors[0].numel() == 0 or tensors[0].numel() // tensors[0].shape[-1] >= 2 ** 31:
        return False
    h = tensors[0].shape[-1]
    for t in tensors:
        if not (t.is_cuda and t.dtype == torch.float32 and t.shape == tensors[0].shape and t.device == tensors[0].device):
            return False
    for ln in lns:
        if not (ln.elementwise_affine and ln.weight is not None and ln.bias is not None
                and tuple(ln.normalized_shape) == (h,) and ln.weight.dtype == torch.float32
                and ln.weight.device == tensors[0].device):
            return False
    d = _lib.dqp_deq_dims(tensors[0].numel() // h, h)
    return _lib.load().dqp_deq_supported(d) == 1


class LayerNormStage(torch.autograd.Function):
    """y = LN(relu ? max(a, 0) : a; gamma, beta, eps)  (dqp_deq_ln_forward / _backward)"""

    @staticmethod
    def forward(ctx, a, gamma, beta, eps, relu):
        a, gamma, beta = _dense(a), _dense(gamma), _dense(beta)
        d = _dims(a)
        y = torch.empty_like(a)
        stats = torch.empty(d.nrows, 2, dtype=torch.float32, device=a.device)
        _lib.call("dqp_deq_ln_forward", a.device, d, a, gamma, beta, float(eps), int(relu), y, stats)
        ctx.save_for_backward(a, gamma, stats)
        ctx.relu = int(relu)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        a, gamma, stats = ctx.saved_tensors
        dy = _dense(dy)
        d = _dims(a)
        need = ctx.needs_input_grad
        da = torch.empty_like(a) if need[0] else None
        dgamma = torch.empty_like(gamma) if need[1] else None
        dbeta = torch.empty_like(gamma) if need[2] else None
        part = _scratch(d, a, need[1] or need[2])
        _lib.call("dqp_deq_ln_backward", a.device, d, a, gamma, stats, ctx.relu, dy, da, dgamma, dbeta, part)
        return da, dgamma, dbeta, None, None


class ResidualStage(torch.autograd.Function):
    """z2 = LN3(ReLU(z1 + LN2(xi + a2)))  (dqp_deq_res_forward / _backward)"""

    @staticmethod
    def forward(ctx, xi, a2, z1, gamma2, beta2, gamma3, beta3, eps2, eps3):
        xi, a2, z1 = _dense(xi), _dense(a2), _dense(z1)
        gamma2, beta2, gamma3, beta3 = _dense(gamma2), _dense(beta2), _dense(gamma3), _dense(beta3)
        d = _dims(xi)
        z2 = torch.empty_like(xi)
        stats = torch.empty(d.nrows, 4, dtype=torch.float32, device=xi.device)
        _lib.call("dqp_deq_res_forward", xi.device, d, xi, a2, z1, gamma2, beta2, gamma3, beta3, float(eps2), float(eps3),
                  z2, stats)
        ctx.save_for_backward(xi, a2, z1, gamma2, beta2, gamma3, stats)
        return z2

    @staticmethod
    @once_differentiable
    def backward(ctx, dz2):
        xi, a2, z1, gamma2, beta2, gamma3, stats = ctx.saved_tensors
        dz2 = _dense(dz2)
        d = _dims(xi)
        need = ctx.needs_input_grad
        ds = torch.empty_like(xi) if (need[0] or need[1]) else None
        dz1 = torch.empty_like(xi) if need[2] else None
        grads = [torch.empty_like(gamma2) if need[k] else None for k in (3, 4, 5, 6)]
        part = _scratch(d, xi, any(need[3:7]))
        _lib.call("dqp_deq_res_backward", xi.device, d, xi, a2, z1, gamma2, beta2, gamma3, stats, dz2, ds, dz1, *grads,
                  part)
        return (ds if need[0] else None, ds if need[1] else None, dz1) + tuple(grads) + (None, None)


def layer_norm(a, ln, relu):
    return LayerNormStage.apply(a, ln.weight, ln.bias, ln.eps, relu)


def residual_block(xi, a2, z1, ln2, ln3):
    return ResidualStage.apply(xi, a2, z1, ln2.weight, ln2.bias, ln3.weight, ln3.bias, ln2.eps, ln3.eps)
