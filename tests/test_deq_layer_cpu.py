"""The host side of the fused DEQLayer stages (include/dqp.h "network-side kernels": dqp_deq_*; csrc/dqp_deq.hip;
policies.FUSED_DEQ_LAYER): the declared and exported names, what is supported, the scratch formula of the header, the
argument checks in front of any launch, and that the flag is a permission -- off by default, no new parameters, CPU
tensors on the torch path.  Needs only the built library: no test here touches a GPU."""
import argparse
import ctypes
import os
import types

import numpy as np
import pytest
import torch

NAMES = ("dqp_deq_supported", "dqp_deq_partial_bytes", "dqp_deq_ln_forward", "dqp_deq_ln_backward",
         "dqp_deq_res_forward", "dqp_deq_res_backward")
HDIMS = (32, 64, 128, 256, 512)
P = ctypes.c_void_p(4096)        # a dummy device pointer (16-byte aligned): the argument checks never dereference it


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from diff_qp_mpc_amd import _lib
    return _lib.load()


def _dims(nrows, hdim):
    from diff_qp_mpc_amd import _lib
    return _lib.dqp_deq_dims(nrows, hdim)


def test_names_declared_bound_and_exported(lib):
    from diff_qp_mpc_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "dqp.h")) as f:
        header = f.read()
    for name in NAMES:
        assert name + "(" in header, name
        assert name in _lib.SYMBOLS, name
        assert hasattr(lib, name), name
    for name in NAMES[2:]:
        restype, argtypes, params = _lib.PROTOTYPES[name]
        assert params[-1] == "stream" and params[0] == "dims", name
        assert argtypes[0] == ctypes.POINTER(_lib.dqp_deq_dims), name
        assert ctypes.c_float not in argtypes                     # scalars are double / int32_t only
    for name in NAMES[:2]:
        assert _lib.PROTOTYPES[name][2] == ("dims",)
    assert lib.dqp_version() == 303


def test_supported(lib):
    for h in HDIMS:
        for n in (0, 1, 3, 65536):
            assert lib.dqp_deq_supported(ctypes.byref(_dims(n, h))) == 1, (n, h)
        assert lib.dqp_deq_supported(ctypes.byref(_dims(-1, h))) == 0
    for h in (16, 48, 96, 1024):
        for n in (0, 1, 3, 65536):
            assert lib.dqp_deq_supported(ctypes.byref(_dims(n, h))) == 0, (n, h)
    assert lib.dqp_deq_supported(None) == 0


def _header_formula(nrows, hdim):
    """16 * hdim * ceil(U / (4 * max(2, ceil(U / 4096)))), U = nrows or, at hdim 32, ceil(nrows / 2)"""
    cdiv = lambda a, b: -(-a // b)
    u = cdiv(nrows, 2) if hdim == 32 else nrows
    return 16 * hdim * cdiv(u, 4 * max(2, cdiv(u, 4096)))


def test_partial_bytes_is_the_header_formula(lib):
    for n, h, want in ((1, 32, 16 * 32), (65, 128, 16 * 128 * 9), (65536, 512, 16 * 512 * 1024)):
        assert _header_formula(n, h) == want
        assert lib.dqp_deq_partial_bytes(ctypes.byref(_dims(n, h))) == want, (n, h)
    for n in (0, 2, 7, 1030, 8191, 16385, 100001):
        for h in HDIMS:
            assert lib.dqp_deq_partial_bytes(ctypes.byref(_dims(n, h))) == _header_formula(n, h), (n, h)
    for d in (_dims(5, 48), _dims(5, 1024), _dims(-1, 128)):
        assert lib.dqp_deq_partial_bytes(ctypes.byref(d)) == 0
    assert lib.dqp_deq_partial_bytes(None) == 0


def _calls(lib):
    """{entry: (call(dims, **{array: pointer}), its arrays, the gradient outputs that may be NULL)}"""
    ref = lambda d: None if d is None else ctypes.byref(d)

    def ln_fwd(d, a=P, gamma=P, beta=P, y=P, stats=P):
        return lib.dqp_deq_ln_forward(ref(d), a, gamma, beta, 1e-5, 1, y, stats, None)

    def ln_bwd(d, a=P, gamma=P, stats=P, dy=P, da=P, dgamma=P, dbeta=P, partial=P):
        return lib.dqp_deq_ln_backward(ref(d), a, gamma, stats, 1, dy, da, dgamma, dbeta, partial, None)

    def res_fwd(d, xi=P, a2=P, z1=P, gamma2=P, beta2=P, gamma3=P, beta3=P, z2=P, stats=P):
        return lib.dqp_deq_res_forward(ref(d), xi, a2, z1, gamma2, beta2, gamma3, beta3, 1e-5, 1e-5, z2, stats, None)

    def res_bwd(d, xi=P, a2=P, z1=P, gamma2=P, beta2=P, gamma3=P, stats=P, dz2=P, ds=P, dz1=P, dgamma2=P, dbeta2=P,
                dgamma3=P, dbeta3=P, partial=P):
        return lib.dqp_deq_res_backward(ref(d), xi, a2, z1, gamma2, beta2, gamma3, stats, dz2, ds, dz1, dgamma2, dbeta2,
                                        dgamma3, dbeta3, partial, None)

    return {"ln_forward": (ln_fwd, ("a", "gamma", "beta", "y", "stats"), ()),
            "ln_backward": (ln_bwd, ("a", "gamma", "stats", "dy"), ("da", "dgamma", "dbeta")),
            "res_forward": (res_fwd, ("xi", "a2", "z1", "gamma2", "beta2", "gamma3", "beta3", "z2", "stats"), ()),
            "res_backward": (res_bwd, ("xi", "a2", "z1", "gamma2", "beta2", "gamma3", "stats", "dz2"),
                             ("ds", "dz1", "dgamma2", "dbeta2", "dgamma3", "dbeta3"))}


def test_return_codes_in_the_headers_order_need_no_gpu(lib):
    OK, BAD, LARGE = 0, -1, -2
    for entry, (call, arrays, grads) in _calls(lib).items():
        none = dict.fromkeys(arrays + grads)
        if grads:
            none["partial"] = None
        assert call(None) == BAD, entry
        assert call(None, **none) == BAD, entry
        assert call(_dims(-1, 128)) == BAD, entry
        assert call(_dims(-1, 48)) == BAD, entry                      # the sign of nrows is looked at before hdim
        for h in (16, 48, 96, 1024):
            assert call(_dims(4, h)) == LARGE, (entry, h)
            assert call(_dims(0, h)) == LARGE, (entry, h)             # ... and hdim before nrows == 0
            assert call(_dims(4, h), **none) == LARGE, (entry, h)     # ... and before the arrays
        for h in HDIMS:
            assert call(_dims(0, h), **none) == OK, (entry, h)        # nothing to do, nothing touched
            for name in arrays:
                assert call(_dims(4, h), **{name: None}) == BAD, (entry, h, name)
        if grads:
            # a parameter gradient needs the scratch; without one the scratch may be NULL
            assert call(_dims(4, 128), partial=None) == BAD, entry
        assert call(_dims(4, 128), **{arrays[0]: ctypes.c_void_p(4100)}) == BAD, entry     # not 16-byte aligned


def _layer(hdim=32, T=5, nx=6, device="cpu"):
    from diff_qp_mpc_amd import policies
    env = types.SimpleNamespace(nx=nx, nu=1, dt=0.05)
    args = argparse.Namespace(T=T, nq=nx // 2, hdim=hdim, layer_type="mlp", deq_out_type=1)
    torch.manual_seed(0)
    return policies.DEQLayer(args, env).to(device)


def test_flag_is_off_and_adds_no_parameters(monkeypatch):
    from diff_qp_mpc_amd import policies
    assert policies.FUSED_DEQ_LAYER is False
    off = {k: tuple(v.shape) for k, v in _layer().state_dict().items()}
    monkeypatch.setattr(policies, "FUSED_DEQ_LAYER", True)
    on = {k: tuple(v.shape) for k, v in _layer().state_dict().items()}
    assert list(on.items()) == list(off.items())


def test_cpu_tensors_take_the_torch_path(monkeypatch):
    from diff_qp_mpc_amd import policies

    def run():
        layer = _layer(hdim=32)
        g = torch.Generator().manual_seed(1)
        x = torch.randn(7, layer.in_dim, generator=g)
        ref, z = layer(x, layer.init_z(7))
        (ref.square().sum() + z.sum()).backward()
        return [ref.detach().numpy(), z.detach().numpy()] + [p.grad.numpy() for p in layer.parameters()]

    off = run()
    monkeypatch.setattr(policies, "FUSED_DEQ_LAYER", True)
    on = run()
    assert len(on) == len(off)
    for a, b in zip(on, off):
        np.testing.assert_array_equal(a, b)
