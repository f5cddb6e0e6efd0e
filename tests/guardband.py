"""Guard bands around tensors: does an entry point read or write outside the extents its arguments declare?

Imported by the tests the way families.py is.  Three pieces:

  guarded(shape, dtype, device, fill)   one raw allocation [front guard | payload | back guard]; the payload comes back
                                        as an ordinary contiguous tensor, the handle's check() looks at the guards
  patched_allocations(fill, device)     a context manager that turns the torch.empty / zeros / full / empty_like /
                                        zeros_like calls of the package's Python layer into guarded allocations, so a
                                        test runs the product's own allocation code (workspaces sized by the `*_bytes`
                                        functions of include/dqp.h, outputs) and checks every guard afterwards
  run_guarded(fn, make_inputs)          the case runner: three runs ("nan", "nan", "zero"), every guard intact, and the
                                        outputs bit-identical over the runs -- a result may not depend on a byte
                                        outside the extents

What the fill is for.  "nan" is the 8-byte word 0x7ff8dead7fc0beef: a NaN read as fp64, each 4-byte half a NaN read as
fp32, a huge value read as int32.  A STORE outside the extents changes a guard; a LOAD outside them that reaches a
result poisons it under "nan" and not under "zero", so the two runs differ.  The payload starts with the same fill, so
an output element that the kernel never writes shows too.

What this cannot see: a guard has a finite size (at least 4096 bytes, at least eight leading-dimension strides), so a
store farther away than that -- more than eight problem strides past the end -- lands outside it.  That limit is stated
here, not pushed out by growing the guards.
"""
import contextlib

import numpy as np
import torch

NAN_WORD = 0x7ff8dead7fc0beef
ALIGN = 512            # a multiple of 256 B; 512 is what the caching allocator hands out, so the payload keeps that too
MIN_GUARD = 4096
LANES = 8              # up to 8 problems share a wavefront in the DPP-row families

_FILLS = {"nan": NAN_WORD, "zero": 0}
_full, _empty = torch.full, torch.empty       # the real ones: this module allocates while the patches are in place


def _word(fill):
    if fill not in _FILLS:
        raise ValueError("fill must be 'nan' or 'zero', not %r" % (fill,))
    return _FILLS[fill]


def default_guard_bytes(shape, dtype):
    """max(4096 B, 8 x the leading-dimension stride in bytes), rounded up to a multiple of ALIGN"""
    item = _empty((), dtype=dtype).element_size()
    lead = item
    for s in tuple(shape)[1:]:
        lead *= int(s)
    g = max(MIN_GUARD, LANES * lead)
    return (g + ALIGN - 1) // ALIGN * ALIGN


class Guarded:
    """The handle of one guarded allocation: .payload (the tensor handed out), .raw (every byte, uint8), .guard_bytes,
    .nbytes (of the payload), .name, .fill."""

    def __init__(self, name, raw, payload, guard_bytes, nbytes, fill):
        self.name, self.raw, self.payload = name, raw, payload
        self.guard_bytes, self.nbytes, self.fill = guard_bytes, nbytes, fill

    def _guards(self):
        """(front, back) uint8 views; back starts at the payload's last byte + 1 and runs to the end of the allocation"""
        g, n = self.guard_bytes, self.nbytes
        return self.raw[:g], self.raw[g + n:]

    def _mismatch(self):
        """(front, back) bool tensors: which guard bytes are not the fill (the word pattern is laid from raw offset 0, so
        the expected bytes are one more buffer of the same words on the same device)"""
        g, n = self.guard_bytes, self.nbytes
        want = _full((self.raw.numel() // 8,), _word(self.fill), dtype=torch.int64, device=self.raw.device).view(torch.uint8)
        return self.raw[:g] != want[:g], self.raw[g + n:] != want[g + n:]

    def corrupted(self):
        """a 0-dim bool tensor on the buffer's device (no synchronisation): is any guard byte not the fill?"""
        front, back = self._mismatch()
        return front.any() | back.any()

    def report(self):
        """None when both guards are intact, else a message with the first and last corrupted byte offset relative to
        the payload (negative: before it; >= nbytes: after it)"""
        g, n = self.guard_bytes, self.nbytes
        front, back = self._mismatch()
        offs = torch.cat([torch.nonzero(front).flatten().cpu() - g, torch.nonzero(back).flatten().cpu() + n])
        if offs.numel() == 0:
            return None
        return ("guard of %s (%d payload bytes, shape %s, %s) corrupted: %d bytes, first at payload offset %d, last at "
                "payload offset %d" % (self.name, n, tuple(self.payload.shape), self.payload.dtype, offs.numel(),
                                       int(offs.min()), int(offs.max())))

    def check(self):
        msg = self.report()
        assert msg is None, msg


def guarded(shape, dtype, device, fill, guard_bytes=None, name="buffer"):
    """-> (payload, handle).  One raw allocation [front guard | payload | back guard], every byte of it the fill."""
    if isinstance(shape, int):
        shape = (shape,)
    shape = tuple(int(s) for s in shape)
    word = _word(fill)
    item = _empty((), dtype=dtype).element_size()
    numel = 1
    for s in shape:
        numel *= s
    nbytes = numel * item
    g = default_guard_bytes(shape, dtype) if guard_bytes is None else int(guard_bytes)
    if g <= 0 or g % ALIGN:            # anything less would move the payload off the alignment of a fresh allocation
        raise ValueError("guard_bytes must be a positive multiple of %d" % ALIGN)
    total = (g + nbytes + g + 7) // 8 * 8          # whole 8-byte words; the few bytes of padding belong to the back guard
    words = _full((total // 8,), word, dtype=torch.int64, device=device)
    raw = words.view(torch.uint8)
    payload = raw[g:g + nbytes].view(dtype).view(shape)
    return payload, Guarded(name, raw, payload, g, nbytes, fill)


def guarded_copy(src, device, fill, name="input", dtype=None):
    """a guarded tensor on `device` that holds the values of `src` (numpy array or tensor)"""
    t = torch.as_tensor(np.ascontiguousarray(src) if isinstance(src, np.ndarray) else src)
    if dtype is not None:
        t = t.to(dtype)
    payload, h = guarded(tuple(t.shape), t.dtype, device, fill, name=name)
    payload.copy_(t)
    return payload, h


_PATCHED = ("empty", "zeros", "full", "empty_like", "zeros_like")


class patched_allocations(contextlib.AbstractContextManager):
    """with patched_allocations(fill, device) as reg: ...   Inside, torch.empty / zeros / full / empty_like / zeros_like
    give guarded tensors when the result is on `device` and the call has the plain form `shape, dtype=, device=` (for
    the _like twins: one tensor, optionally dtype=); every other form, and every empty result, goes to the real
    function untouched.  On a clean exit the device is synchronised and every guard checked (AssertionError listing the
    corrupted ones); the torch functions are restored in every case.  reg.sizes: payload bytes of every intercepted
    allocation, in order; reg.handles: their handles."""

    def __init__(self, fill, device="cuda"):
        _word(fill)
        self.fill = fill
        self.device = torch.device(device)
        self.handles = []
        self._orig = {}

    @property
    def sizes(self):
        return [h.nbytes for h in self.handles]

    def _on_device(self, dev):
        dev = torch.device("cpu" if dev is None else dev)
        return dev.type == self.device.type and (dev.index is None or self.device.index is None or
                                                 dev.index == self.device.index)

    def _make(self, kind, shape, dtype, device, value=None):
        payload, h = guarded(shape, dtype, device, self.fill, name="%s#%d%s" % (kind, len(self.handles), tuple(shape)))
        if kind.startswith("zeros"):
            payload.zero_()
        elif kind == "full":
            payload.fill_(value)
        self.handles.append(h)
        return payload

    @staticmethod
    def _shape(args):
        if len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)):
            args = tuple(args[0])
        if args and all(isinstance(s, int) and not isinstance(s, bool) for s in args):
            return tuple(args)
        return None

    def _wrap(self, kind, orig):
        def plain(*args, **kw):
            if set(kw) <= {"dtype", "device"}:
                if kind == "full":
                    shape = self._shape(args[:1]) if len(args) == 2 else None
                else:
                    shape = self._shape(args)
                if (shape is not None and 0 not in shape and self._on_device(kw.get("device")) and
                        (kind != "full" or "dtype" in kw)):
                    dtype = kw.get("dtype") or torch.get_default_dtype()
                    dev = kw.get("device") or "cpu"
                    return self._make(kind, shape, dtype, dev, args[1] if kind == "full" else None)
            return orig(*args, **kw)

        def like(*args, **kw):
            if (len(args) == 1 and isinstance(args[0], torch.Tensor) and set(kw) <= {"dtype"} and
                    args[0].numel() > 0 and args[0].layout == torch.strided and self._on_device(args[0].device)):
                return self._make(kind, tuple(args[0].shape), kw.get("dtype") or args[0].dtype, args[0].device)
            return orig(*args, **kw)

        return like if kind.endswith("_like") else plain

    def __enter__(self):
        for k in _PATCHED:
            self._orig[k] = getattr(torch, k)
        for k in _PATCHED:
            setattr(torch, k, self._wrap(k, self._orig[k]))
        return self

    def __exit__(self, et, ev, tb):
        for k, f in self._orig.items():
            setattr(torch, k, f)
        if et is None:
            self.check()
        return False

    def check(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        check_all(self.handles)


def check_all(handles):
    """every guard of `handles` intact, with one device-to-host transfer when they are"""
    if not handles:
        return
    flags = torch.stack([h.corrupted() for h in handles])
    if bool(flags.any()):
        msgs = [m for m in (h.report() for h in handles) if m is not None]
        raise AssertionError("; ".join(msgs))


def _flatten(out):
    if out is None:
        return []
    if isinstance(out, torch.Tensor):
        return [out]
    if isinstance(out, dict):
        out = [out[k] for k in out]
    flat = []
    for o in out:
        flat.extend(_flatten(o))
    return flat


def _bits(t):
    return t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes() if t.numel() else b""


def run_guarded(fn, make_inputs, device="cuda"):
    """fn(inputs) -> a tensor, or a tuple / list / dict of tensors (None entries are skipped); make_inputs(put) builds
    the inputs, with put(array, name) -> a guarded device tensor holding the array's values (dtype kept).

    Three runs, fills "nan", "nan", "zero": the inputs are rebuilt with that fill, `fn` runs under
    patched_allocations(fill), every guard (inputs' and intercepted allocations') must be intact, and the outputs of
    the three runs must be bit-identical (every path of the package is bit-reproducible from run to run, so no
    tolerance between fills exists here).
    -> (outputs of the first "nan" run as `fn` returned them, sizes of the intercepted allocations of that run)."""
    runs = []
    for fill in ("nan", "nan", "zero"):
        handles = []

        def put(a, name="input", dtype=None):
            payload, h = guarded_copy(a, device, fill, name=name, dtype=dtype)
            handles.append(h)
            return payload

        inputs = make_inputs(put)
        with patched_allocations(fill, device) as reg:
            out = fn(inputs)
        if torch.device(device).type == "cuda":
            torch.cuda.synchronize()
        check_all(handles)
        runs.append((fill, out, list(reg.sizes), [t.detach().clone() for t in _flatten(out)]))
    ref = runs[0]
    for fill, _, _, flat in runs[1:]:
        assert len(flat) == len(ref[3])
        for i, (a, b) in enumerate(zip(ref[3], flat)):
            assert a.shape == b.shape and a.dtype == b.dtype
            if _bits(a) != _bits(b):
                d = (a.double() - b.double()).abs()
                raise AssertionError("output %d of the %r run differs from the first 'nan' run in %d of %d elements "
                                     "(max |diff| %s): the result depends on bytes outside the extents, or the path "
                                     "is not reproducible" % (i, fill, int((a != b).sum()), a.numel(),
                                                              float(d[~d.isnan()].max()) if (~d.isnan()).any() else "nan"))
    return ref[1], ref[2]
