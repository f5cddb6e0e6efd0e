"""ctypes binding of the C ABI in include/dqp.h (csrc/libdqp_hip.so).

The library is loaded lazily on first use and there is deliberately no fallback: a missing
or unloadable library raises RuntimeError naming the build command.  The prototypes are read from
include/dqp.h (prototypes()): the header is the one place that says what an entry point takes.  The
structs and the few constants are written out here; tests pin the constants against the header.
"""
import ctypes
import os
import re

import torch

from . import _build


class dqp_dims(ctypes.Structure):
    _fields_ = [("nbatch", ctypes.c_int32), ("nz", ctypes.c_int32), ("nineq", ctypes.c_int32),
                ("neq", ctypes.c_int32),
                ("stride_Q", ctypes.c_int64), ("stride_p", ctypes.c_int64),
                ("stride_G", ctypes.c_int64), ("stride_h", ctypes.c_int64),
                ("stride_A", ctypes.c_int64), ("stride_b", ctypes.c_int64)]


class dqp_opts(ctypes.Structure):
    _fields_ = [("eps", ctypes.c_double), ("stall_tol", ctypes.c_double),
                ("max_iter", ctypes.c_int32),
                ("not_improved_lim", ctypes.c_int32), ("flags", ctypes.c_uint32),
                ("reserved", ctypes.c_int32),
                ("dyn_id", ctypes.c_int32), ("dyn_T", ctypes.c_int32), ("dyn_dt", ctypes.c_double),
                ("dyn_x0", ctypes.c_void_p)]


DQP_OK = 0
DQP_FLAG_DENSE_BACKWARD = 1
DQP_FLAG_GENERIC_ONLY = 2
DQP_FLAG_NO_NULLSPACE = 4
DQP_FLAG_RIC_GLOBAL_WS = 64
DQP_FLAG_BACKWARD_CTX = 8
DQP_FLAG_BATCH_TERMINATION = 16
DQP_FLAG_HISTORY_ONLY = 32
DQP_FLAG_STRICT_GET_STEP = 128
DQP_FLAG_STAGEWISE = 256
DQP_STATUS_Q_NOT_PD = 1
DQP_STATUS_A_RANK_DEF = 2
DQP_MAX_DIM = 64
DQP_MAX_DIM_LARGE = 512
SHARED_GRAD_KC = 64      # samples per split-K chunk of dqp_qp_backward_shared (csrc/dqp_shared_grad.hip: KC)


class dqp_al_mpc_dims(ctypes.Structure):
    _fields_ = [("nbatch", ctypes.c_int32), ("n_state", ctypes.c_int32), ("n_ctrl", ctypes.c_int32),
                ("T", ctypes.c_int32)]


class dqp_al_bounds(ctypes.Structure):
    """lower / upper of (sample b, knot t, control k) at [b * stride_b + t * stride_t + k] (include/dqp.h)"""
    _fields_ = [("lower", ctypes.c_void_p), ("upper", ctypes.c_void_p), ("stride_b", ctypes.c_int64),
                ("stride_t", ctypes.c_int64)]


class dqp_al_dims(ctypes.Structure):
    _fields_ = [("nbatch", ctypes.c_int32), ("nz", ctypes.c_int32), ("ncon", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


class dqp_mpc_dims(ctypes.Structure):
    _fields_ = [("nbatch", ctypes.c_int32), ("n_state", ctypes.c_int32), ("n_ctrl", ctypes.c_int32),
                ("T", ctypes.c_int32), ("has_bounds", ctypes.c_int32), ("dyn_id", ctypes.c_int32),
                ("n_state_host", ctypes.c_int32)]     # 0 unless given: positional constructions keep the native routes


class dqp_deq_dims(ctypes.Structure):
    _fields_ = [("nrows", ctypes.c_int32), ("hdim", ctypes.c_int32)]


class dqp_trace_record(ctypes.Structure):
    _fields_ = [("kernel", ctypes.c_char * 248), ("ms", ctypes.c_float), ("reserved", ctypes.c_int32)]


_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "double": ctypes.c_double, "size_t": ctypes.c_size_t}
_STRUCTS = {c.__name__: c for c in (dqp_dims, dqp_opts, dqp_mpc_dims, dqp_al_dims, dqp_al_mpc_dims, dqp_al_bounds,
                                    dqp_deq_dims, dqp_trace_record)}
_STRUCTS["dqp_mpc_bounds"] = dqp_al_bounds        # a typedef in the header


def prototypes(header):
    """{name: (restype, argtypes, parameter names)} of every `ret dqp_name(args);` in the text of include/dqp.h.
    int, int32_t, double, size_t are the ctypes scalars, a returned `const char *` is c_char_p, a pointer to a struct
    of this module is POINTER of it, every other pointer c_void_p; anything else is a RuntimeError naming the prototype."""
    text = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    out = {}
    for ret, name, params in re.findall(r"([\w \t*]+?)\s*\b(dqp_\w+)\s*\(([^()]*)\)\s*;", text):
        def ctype(decl, returned=False):
            t = " ".join(re.sub(r"\bconst\b", " ", decl).replace("*", " * ").split())
            if t in _SCALARS:
                return _SCALARS[t]
            if returned and t == "char *":
                return ctypes.c_char_p
            if t.endswith(" *") and not returned:
                base = t[:-2]
                return ctypes.POINTER(_STRUCTS[base]) if base in _STRUCTS else ctypes.c_void_p
            raise RuntimeError("diff_qp_mpc_amd: include/dqp.h: no ctypes rule for %r in the prototype of %s"
                               % (" ".join(decl.split()), name))
        argtypes, names = [], []
        for p in ([] if params.strip() in ("", "void") else params.split(",")):
            m = re.fullmatch(r"\s*(.*?)(\w+)\s*", p, flags=re.S)
            argtypes.append(ctype(m.group(1)))
            names.append(m.group(2))
        out[name] = (ctype(ret, returned=True), argtypes, tuple(names))
    return out


def dyn_ids(header):
    """{"pendulum1l": 1, ...}: the `DQP_DYN_NAME = k` enumerators in the text of include/dqp.h, lower-cased without the prefix"""
    text = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    return {name.lower(): int(k) for name, k in re.findall(r"\bDQP_DYN_([A-Z0-9_]+)\s*=\s*(\d+)", text)}


with open(os.path.join(os.path.dirname(_build.HERE), "include", "dqp.h")) as _f:
    _header = _f.read()
PROTOTYPES = prototypes(_header)
DQP_DYN = dyn_ids(_header)       # the registered device models; load() checks that the library knows each
SYMBOLS = tuple(PROTOTYPES)      # every symbol include/dqp.h declares
_launches = {}                   # the entries call() serves (last parameter `stream`), filled by load()
_lib = None


def path():
    # DQP_HIP_LIBRARY: A/B runs of an alternative build of the same library (tools/, profiling)
    return os.environ.get("DQP_HIP_LIBRARY") or _build.SO


def load():
    """Returns the ctypes CDLL; raises if the HIP library has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    so = path()
    if not os.path.exists(so):
        raise RuntimeError(
            "diff_qp_mpc_amd: %s is missing. Build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` (hipcc --offload-arch=gfx950). There is no CPU fallback." % so)
    try:
        lib = ctypes.CDLL(so)
    except OSError as e:  # pragma: no cover
        raise RuntimeError("diff_qp_mpc_amd: cannot load %s: %s" % (so, e))
    for name, (restype, argtypes, params) in PROTOTYPES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise RuntimeError("diff_qp_mpc_amd: %s does not export %s, which include/dqp.h declares" % (so, name))
        fn.restype, fn.argtypes = restype, argtypes
        if params and params[-1] == "stream":
            _launches[name] = fn
    for name, k in DQP_DYN.items():
        if lib.dqp_dyn_sizes(k, None, None) != DQP_OK:
            raise RuntimeError("diff_qp_mpc_amd: include/dqp.h declares DQP_DYN_%s = %d, which %s does not register"
                               % (name.upper(), k, so))
    _lib = lib
    return lib


def call(name, dev, *args):
    """The one way the package launches: lib.<name>(*args, current stream of `dev`) under torch.cuda.device(dev), for
    the entries whose last parameter is `stream`; a return code other than DQP_OK raises, naming the entry.  A
    torch.Tensor goes in as its data pointer (None or an empty tensor as NULL; a tensor that is not on a GPU is
    refused), a ctypes.Structure by reference, anything else (ints, floats, DeviceBounds.ref()) as it is.  Callers hand
    over the tensors themselves, so `args` references every converted temporary until the call has been enqueued."""
    fn = _launches.get(name)
    if fn is None:                  # the first call, or not a launching entry
        load()
        if name not in _launches:
            raise RuntimeError("diff_qp_mpc_amd: %s is not an entry point of include/dqp.h that takes a stream" % name)
        fn = _launches[name]
    conv = []
    for a in args:
        if isinstance(a, torch.Tensor):
            if a.is_cuda:
                a = a.data_ptr()            # 0 for an empty tensor
            elif a.numel() == 0:
                a = None
            else:
                raise RuntimeError("diff_qp_mpc_amd runs only on a GPU (HIP): %s got a %s tensor. "
                                   "There is no CPU fallback." % (name, a.device))
        elif isinstance(a, ctypes.Structure):
            a = ctypes.byref(a)
        conv.append(a)
    with torch.cuda.device(dev):
        rc = fn(*conv, torch.cuda.current_stream(dev).cuda_stream)
    if rc != DQP_OK:
        check(rc, name)


def check(rc, what):
    if rc != DQP_OK:
        msg = load().dqp_error_string(rc).decode()
        raise RuntimeError("diff_qp_mpc_amd: %s failed: %s (code %d)" % (what, msg, rc))


class trace:
    """with _lib.trace(max_launches) as t: ...  -> t.records = [(kernel name, ms)], t.by_kernel() = {name: (count, mean ms)}:
    HIP-event timing of every kernel launch the library makes inside the block (dqp_trace_begin / dqp_trace_end)."""

    def __init__(self, max_launches=4096):
        self.cap = int(max_launches)
        self.records = []

    def __enter__(self):
        check(load().dqp_trace_begin(self.cap), "dqp_trace_begin")
        return self

    def __exit__(self, *exc):
        buf = (dqp_trace_record * self.cap)()
        n = ctypes.c_int32(0)
        rc = load().dqp_trace_end(buf, self.cap, ctypes.byref(n))
        self.records = [(buf[i].kernel.decode(errors="replace"), float(buf[i].ms)) for i in range(min(n.value, self.cap))]
        if exc[0] is None:
            check(rc, "dqp_trace_end")
        return False

    def by_kernel(self):
        acc = {}
        for k, ms in self.records:
            c, t = acc.get(k, (0, 0.0))
            acc[k] = (c + 1, t + ms)
        return {k: (c, t / c) for k, (c, t) in acc.items()}
