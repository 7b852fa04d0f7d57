"""ctypes binding of libhig.so (the C ABI declared in include/hig.h).

The product path has NO CPU fallback: if the shared library is missing or a tensor is not on a
ROCm device, calls raise.  PyTorch is used only for device memory, streams and autograd plumbing.
"""
import ctypes as C
import os

import torch

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libhig.so")

HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "hig.h")
if not os.path.exists(HEADER_PATH):
    raise RuntimeError("include/hig.h not found at %s -- the binding of libhig.so is derived from it" % HEADER_PATH)
with open(HEADER_PATH) as _f:
    _constants, _structs, _callbacks, _prototypes = _abi.parse_header(_f.read())

# the Structure class of every struct of the header (keyword construction: Dims(B=..., T=..., ...))
STRUCT_NAMES = {"hig_dims": "Dims", "hig_text_dims": "TextDims", "hig_eval_dims": "EvalDims", "hig_gemm_desc": "GemmDesc",
                "hig_gemm16_desc": "Gemm16Desc"}
_classes, _hooks, SIGNATURES = _abi.bind(_structs, _callbacks, _prototypes, STRUCT_NAMES)
LAYER_HOOK = _hooks["hig_layer_hook"]
# every symbol include/hig.h declares
SYMBOLS = tuple(_prototypes)

# every constant of the header under its name without `HIG_` (P_SEQ_EMB, EPI_BIAS_GELU, NORM_BLOCKS, ...), and the Structures
for _name, _value in [(n[len("HIG_"):], v) for n, v in _constants.items()] + list(_classes.items()):
    if _name in globals():
        raise RuntimeError("include/hig.h: %s would shadow an attribute of the binding" % _name)
    globals()[_name] = _value
T_NLAYER = TL_NLAYER  # noqa: F821  (the text head's per-layer block is HIG_TL_* in the header)

# what hig_denoiser_plan is asked besides the header's codes: the environment switches in the struct's order, their defaults,
# and the names its answer's slots go by
DN_SWITCHES = ("HIG_TEXT_BATCH", "HIG_TEXT_FORK", "HIG_FWD_SPLIT", "HIG_LNFOLD32", "HIG_FWD16_FORK", "HIG_CTX16", "HIG_JOINT16",
               "HIG_FUSE_APPLY", "HIG_FUSE_OUT", "HIG_EDGE16", "HIG_BWD_OVERLAP")
DN_SWITCH_DEFAULTS = (1, 1, -1, 1, -1, 1, 1, 2, 1, 1, -1)
DN_PLAN_SLOTS = ("entry", "text_batched", "text_fork", "fuse_apply", "fold32", "split", "fork_emb", "fork_text", "ctx_mm16", "joint16",
                 "fuse_mm16", "fuse_out", "fuse_front", "wgrad_fork", "edge16", "Fp", "wants_side_stream")

_lib = None


def lib():
    """Loads libhig.so once and gives every prototype of the header its argtypes and restype.  Raises (never falls back) when
    the library is missing or lacks a declared symbol."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "libhig.so not found at %s -- build it with `python -c 'import __graft_entry__ as g; "
                "g.build()'` (hipcc --offload-arch=gfx950); there is no CPU fallback" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in SIGNATURES.items():
            try:
                fn = getattr(L, name)
            except AttributeError:
                raise RuntimeError("libhig.so is older than include/hig.h: rebuild (%s is missing)" % name) from None
            fn.restype, fn.argtypes = restype, argtypes
        _lib = L
    return _lib


def last_error():
    buf = C.create_string_buffer(512)
    lib().hig_last_error(buf, 512)
    return buf.value.decode(errors="replace")


def check(rc):
    if rc != 0:
        raise RuntimeError("libhig error %d: %s" % (rc, last_error()))


def denoiser_plan(dims, entry, training=0, has_xf_out=0, facts=0, capturing=0, chip_cus=256, wsp32_active=1, switches=None):
    """hig_denoiser_plan as {slot name: value}; switches: {switch name: value} over the defaults, or None for the process's."""
    sw = None
    if switches is not None:
        unknown = set(switches) - set(DN_SWITCHES)
        assert not unknown, unknown
        sw = (C.c_int32 * DN_NSWITCHES)(*[switches.get(n, v) for n, v in zip(DN_SWITCHES, DN_SWITCH_DEFAULTS)])
    out = (C.c_int32 * DN_PLAN_NSLOTS)()
    api.hig_denoiser_plan(dims, entry, training, has_xf_out, facts, capturing, chip_cus, wsp32_active, sw, out, DN_PLAN_NSLOTS)
    return dict(zip(DN_PLAN_SLOTS, out))


def denoiser_last_schedule():
    """What the most recent denoiser entry point on this thread ran, as {slot name: value} (None: none yet)."""
    out = (C.c_int32 * DN_PLAN_NSLOTS)()
    return dict(zip(DN_PLAN_SLOTS, out)) if api.hig_denoiser_last_schedule(out, DN_PLAN_NSLOTS) >= 0 else None


def stream_ptr():
    """The hipStream_t torch is currently launching on (so torch.cuda.graph captures us)."""
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    """Device pointer of a tensor (None -> NULL).  Refuses host tensors: no CPU path exists."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("libhig needs ROCm device tensors (got a %s tensor); there is no CPU fallback"
                           % t.device.type)
    return C.c_void_p(t.data_ptr())


def _current_stream():
    return torch.cuda.current_stream().cuda_stream


class _Api:
    """The package's way into libhig.so: api.<name>(*args) under the header's own names, every argument held to the type the header
    declares for it (_abi.gateway states what each type takes), all of it on the host before anything is launched.  A trailing
    hig_stream_t may be left out and is then torch's current stream at the time of the call, so a call under torch.cuda.graph is
    captured.  A status other than HIG_OK raises as check() does, a negative size raises with the library's message, the functions
    of _abi.NOT_STATUS and every other integer return their value.  Contiguity is not checked: the entry points take leading
    dimensions, and strided views are legitimate operands.  A name the header does not declare is an AttributeError."""

    def __getattr__(self, name):
        if name not in _GATEWAY:
            raise AttributeError("include/hig.h declares no %s" % name)
        entry, rule, convert = _GATEWAY[name], _GATEWAY[name][3], _abi.convert

        def call(*args):                                    # (the entry is asked of lib() at every call, as a raw call asks it)
            result = getattr(lib(), name)(*convert(name, entry, args, _current_stream))
            if rule == "status" and result != 0:
                raise RuntimeError("libhig error %d: %s" % (result, last_error()))
            if rule == "size" and result < 0:
                raise RuntimeError("libhig: " + last_error())
            return None if rule == "status" else result
        call.__name__ = call.__qualname__ = name
        setattr(self, name, call)                           # (the next lookup finds it without coming here)
        return call


_GATEWAY = _abi.gateway(_prototypes, {c: _classes[py] for c, py in STRUCT_NAMES.items()}, _hooks)
api = _Api()
