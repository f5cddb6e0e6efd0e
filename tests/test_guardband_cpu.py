"""tests/guardband.py on CPU tensors: the helper the GPU guard-band tests (test_gpu_guardband.py) stand on must itself
see a byte written one element before or after a payload, and must not change what the code under test is handed."""
import struct

import numpy as np
import pytest
import torch

import guardband as gb


@pytest.mark.parametrize("shape,dtype", [((3, 5), torch.float64), ((7,), torch.float32), ((2, 3, 4), torch.float64),
                                         ((5, 2), torch.int32), ((3,), torch.int32), ((1,), torch.float64)])
@pytest.mark.parametrize("fill", ["nan", "zero"])
def test_payload_shape_dtype_contiguity_alignment(shape, dtype, fill):
    t, h = gb.guarded(shape, dtype, "cpu", fill)
    assert tuple(t.shape) == shape and t.dtype == dtype and t.is_contiguous() and t.device.type == "cpu"
    assert h.payload is t and h.nbytes == t.numel() * t.element_size()
    # the guards: a multiple of 256 B, at least 4096 B and at least 8 leading-dimension strides
    lead = t.element_size() * int(np.prod(shape[1:]))
    assert h.guard_bytes % 512 == 0 and h.guard_bytes >= max(4096, 8 * lead)
    # the payload sits at the alignment of the raw allocation itself (the guard is a multiple of 256), i.e. that of
    # a plain allocation: the CPU allocator aligns to 64 bytes
    assert (t.data_ptr() - h.raw.data_ptr()) == h.guard_bytes
    assert t.data_ptr() % 256 == h.raw.data_ptr() % 256
    assert t.data_ptr() % 64 == torch.empty(shape, dtype=dtype).data_ptr() % 64 == 0
    # the back guard starts at the payload's last byte + 1
    front, back = h._guards()
    assert front.data_ptr() + front.numel() == t.data_ptr()
    assert back.data_ptr() == t.data_ptr() + h.nbytes and back.numel() >= h.guard_bytes
    h.check()


def test_guard_grows_with_the_leading_stride():
    t, h = gb.guarded((3, 40, 40), torch.float64, "cpu", "nan")
    assert h.guard_bytes >= 8 * 40 * 40 * 8 and h.guard_bytes % 256 == 0
    t, h = gb.guarded((3, 4), torch.float64, "cpu", "nan", guard_bytes=512)
    assert h.guard_bytes == 512
    for bad in (100, 256, 768):         # 256 B would move the payload off the 512 B a fresh device allocation has
        with pytest.raises(ValueError):
            gb.guarded((3, 4), torch.float64, "cpu", "nan", guard_bytes=bad)
    with pytest.raises(ValueError):
        gb.guarded((3, 4), torch.float64, "cpu", "ones")


def test_fills_are_bit_exact():
    t, h = gb.guarded((5, 3), torch.float64, "cpu", "nan")
    assert (h.raw.view(torch.int64) == 0x7ff8dead7fc0beef).all()              # guards and payload alike
    assert (t.view(torch.int64) == 0x7ff8dead7fc0beef).all()
    assert h.raw.numpy().tobytes()[:8] == struct.pack("<Q", 0x7ff8dead7fc0beef)
    t, h = gb.guarded((5, 3), torch.float64, "cpu", "zero")
    assert (h.raw == 0).all() and (t == 0).all()
    # an odd number of 4-byte elements: the back guard starts in the middle of a word and still checks clean
    t, h = gb.guarded((3,), torch.int32, "cpu", "nan")
    assert h.nbytes == 12
    h.check()


def test_the_pattern_is_nan_as_fp64_and_as_fp32_and_huge_as_int32():
    t, _ = gb.guarded((4,), torch.float64, "cpu", "nan")
    assert torch.isnan(t).all()
    t, _ = gb.guarded((8,), torch.float32, "cpu", "nan")
    assert torch.isnan(t).all()                                               # both halves of the word
    assert sorted(set(t.view(torch.int32).tolist())) == [0x7fc0beef, 0x7ff8dead]
    t, _ = gb.guarded((8,), torch.int32, "cpu", "nan")
    assert int(t.min()) > 2 ** 30


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32, torch.int32])
@pytest.mark.parametrize("fill", ["nan", "zero"])
def test_a_write_one_element_outside_is_named(dtype, fill):
    shape = (3, 5)
    for where in ("before", "after"):
        t, h = gb.guarded(shape, dtype, "cpu", fill)
        item = t.element_size()
        whole = h.raw.view(dtype)                                             # the raw buffer, typed
        first = h.guard_bytes // item
        idx = first - 1 if where == "before" else first + t.numel()
        whole[idx] = 1                                                        # neither fill has this bit pattern
        with pytest.raises(AssertionError) as e:
            h.check()
        lo = -item if where == "before" else h.nbytes
        msg = str(e.value)
        assert "buffer" in msg and "first at payload offset" in msg
        first_off = int(msg.split("first at payload offset ")[1].split(",")[0])
        last_off = int(msg.split("last at payload offset ")[1])
        assert lo <= first_off <= last_off < lo + item, msg
        assert bool(h.corrupted())


def test_a_single_byte_is_seen_and_a_write_inside_is_not():
    t, h = gb.guarded((4, 4), torch.float64, "cpu", "nan", name="ws")
    t.fill_(3.0)
    t[3, 3] = float("inf")
    t[0, 0] = -1.0
    h.check()
    assert not bool(h.corrupted())
    h.raw[h.guard_bytes + h.nbytes + 777] ^= 1
    with pytest.raises(AssertionError, match=r"guard of ws .* first at payload offset %d, last at payload offset %d"
                       % (h.nbytes + 777, h.nbytes + 777)):
        h.check()
    t, h = gb.guarded((4, 4), torch.float64, "cpu", "zero")
    h.raw[0] = 1
    with pytest.raises(AssertionError, match="first at payload offset -%d," % h.guard_bytes):
        h.check()


def test_patched_allocations_registers_sizes_and_restores():
    orig = [getattr(torch, k) for k in gb._PATCHED]
    kw = dict(dtype=torch.float64, device="cpu")
    with gb.patched_allocations("nan", "cpu") as reg:
        assert all(getattr(torch, k) is not o for k, o in zip(gb._PATCHED, orig))
        a = torch.empty(3, 5, **kw)
        b = torch.empty((7,), dtype=torch.int32, device="cpu")
        c = torch.zeros(2, 2, **kw)
        d = torch.full((4,), 2.5, **kw)
        e = torch.empty_like(a)
        f = torch.zeros_like(b)
        g = torch.empty(11, dtype=torch.float32)                   # no device: the default one, the CPU
        # forms that are delegated untouched
        n0 = len(reg.handles)
        z = torch.empty(3, 0, **kw)                                # empty result
        p = torch.empty(2, dtype=torch.bool, pin_memory=False)     # another keyword
        q = torch.zeros(3, dtype=torch.float64, device="meta")     # another device
        r = torch.empty_like(a, memory_format=torch.contiguous_format)
        assert len(reg.handles) == n0
    assert reg.sizes == [120, 28, 32, 32, 120, 28, 44]
    assert torch.isnan(a).all() and torch.isnan(e).all() and torch.isnan(g).all()
    assert (c == 0).all() and (f == 0).all() and (d == 2.5).all()
    assert a.shape == (3, 5) and b.dtype == torch.int32 and f.dtype == torch.int32 and f.shape == (7,)
    assert z.shape == (3, 0) and q.device.type == "meta" and p.dtype == torch.bool and r.shape == a.shape
    assert all(getattr(torch, k) is o for k, o in zip(gb._PATCHED, orig))
    # zero fill
    with gb.patched_allocations("zero", "cpu") as reg:
        a = torch.empty(3, **kw)
    assert (a == 0).all() and reg.sizes == [24]


def test_patched_allocations_restores_when_the_body_raises_and_checks_on_exit():
    orig = [getattr(torch, k) for k in gb._PATCHED]
    with pytest.raises(KeyError):
        with gb.patched_allocations("nan", "cpu"):
            raise KeyError("body")
    assert all(getattr(torch, k) is o for k, o in zip(gb._PATCHED, orig))
    # a store past the end of an intercepted allocation fails the exit check, and the functions are still restored
    with pytest.raises(AssertionError, match="first at payload offset 24,"):
        with gb.patched_allocations("nan", "cpu") as reg:
            a = torch.empty(3, dtype=torch.float64, device="cpu")
            reg.handles[0].raw.view(torch.float64)[reg.handles[0].guard_bytes // 8 + 3] = 0.0
    assert all(getattr(torch, k) is o for k, o in zip(gb._PATCHED, orig))


def test_run_guarded_passes_clean_code_and_catches_the_three_faults():
    x = np.arange(12.0).reshape(3, 4)

    def make(put):
        return put(x, "x")

    def clean(t):
        out = torch.empty(3, dtype=torch.float64, device="cpu")
        out.copy_(t.sum(1))
        return out, None

    (out, none), sizes = gb.run_guarded(clean, make, device="cpu")
    assert none is None and sizes == [24]
    np.testing.assert_array_equal(out.numpy(), x.sum(1))

    def raw_of(t):                # the whole allocation behind a guarded tensor, typed
        return torch.empty(0, dtype=t.dtype).set_(t.untyped_storage())

    def reads_past_the_end(t):
        out = torch.empty(3, dtype=torch.float64, device="cpu")
        out.copy_(t.sum(1))
        out[2] += raw_of(t)[t.storage_offset() + t.numel()]          # NaN under "nan", 0 under "zero"
        return out

    with pytest.raises(AssertionError, match="depends on bytes outside the extents"):
        gb.run_guarded(reads_past_the_end, make, device="cpu")

    def writes_before_the_input(t):
        raw_of(t)[t.storage_offset() - 1] = 0.5
        return t.sum(1)

    with pytest.raises(AssertionError, match="guard of x .* first at payload offset -8, last at payload offset -"):
        gb.run_guarded(writes_before_the_input, make, device="cpu")

    def forgets_an_element(t):
        out = torch.empty(3, dtype=torch.float64, device="cpu")
        out[:2] = t.sum(1)[:2]
        return out

    with pytest.raises(AssertionError, match="depends on bytes outside the extents"):
        gb.run_guarded(forgets_an_element, make, device="cpu")


def test_newton_solve_bytes_is_exactly_the_carve():
    """dqp_al_newton_solve_bytes: per problem the update (nz), 20 candidate merits, the current merit and one double's
    room for the int32 pivot flag -- the carve of newton_work (csrc/dqp_al.hip), without the two doubles of slack
    earlier versions added -- and the dense form's arrays in front of the same tail; the other AL workspace sizes are
    this one (include/dqp.h).  Host functions: no GPU."""
    import ctypes
    from diff_qp_mpc_amd import _lib
    lib = _lib.load()
    for B, n, m, T in ((1, 2, 1, 2), (3, 2, 1, 5), (5, 6, 1, 6), (3, 12, 4, 4)):
        d = _lib.dqp_al_mpc_dims(B, n, m, T)
        r = ctypes.byref(d)
        nz, ncon = T * (n + m), T * n + 2 * T * m
        assert lib.dqp_al_newton_solve_bytes(r, 1) == 8 * B * (nz + 20 + 1 + 1)
        assert lib.dqp_al_newton_solve_bytes(r, 0) == 8 * B * ((T - 1) * n * n + (T - 1) * n * m + ncon + ncon * nz + 2 * nz + 22)
        for f in (lib.dqp_al_mpc_solve_bytes, lib.dqp_al_mpc_solve_fused_bytes, lib.dqp_al_newton_solve_xbounds_bytes,
                  lib.dqp_al_mpc_solve_xbounds_bytes):
            assert f(r) == lib.dqp_al_newton_solve_bytes(r, 1)


def test_the_python_layer_allocates_what_the_size_functions_say():
    """A lint, no more: no `// 8 + 1` next to a `*_bytes` call on a torch.empty line of the package.  It sees one
    spelling on one line; what holds the Python layer to the size functions is tests/test_gpu_guardband.py, where every
    workspace the layer allocates has a guard band right behind its last byte."""
    import os
    import re
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "diff-qp-mpc_amd")
    for name in sorted(os.listdir(root)):
        if name.endswith(".py"):
            with open(os.path.join(root, name)) as f:
                for i, line in enumerate(f, 1):
                    if "_bytes(" in line and "torch.empty" in line:
                        assert not re.search(r"//\s*[48]\s*\+\s*\d", line), "%s:%d: %s" % (name, i, line.strip())
