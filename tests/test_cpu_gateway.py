"""The gateway (hig_amd/_abi.py gateway() / convert(), hig_amd/_lib.py api): what each declared parameter type takes and refuses,
the two accepted argument counts, which results are statuses, and that no file of the package calls the library around it.  CPU
only: the converters are pure, so every refusal below is shown on host tensors with nothing launched; the few calls that reach the
library are host functions of it."""
import ctypes as C
import os
import re

import pytest
import torch

from hig_amd import _abi, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PACKAGE = os.path.join(ROOT, "human-interaction-generation_amd")


def convert(name, *args, stream=lambda: 0xBEEF):
    return _abi.convert(name, _lib._GATEWAY[name], args, stream)


def test_gateway_builds_for_every_prototype_and_names_what_it_cannot_pass():
    parsed = _abi.parse_header(open(_lib.HEADER_PATH).read())
    classes, hooks, _ = _abi.bind(*parsed[1:], _lib.STRUCT_NAMES)
    by_c_name = {c: classes[py] for c, py in _lib.STRUCT_NAMES.items()}
    gw = _abi.gateway(parsed[3], by_c_name, hooks)
    assert tuple(gw) == _lib.SYMBOLS == tuple(_lib._GATEWAY) and len(gw) >= 130
    for name, (ret, params) in parsed[3].items():
        names, ctypes_, converters, rule = gw[name]
        assert names == tuple(n for n, _ in params) and ctypes_ == tuple(t for _, t in params) and len(converters) == len(params)
        assert all(callable(c) for c in converters) and rule in ("status", "size", "value")
        assert (rule == "status") == (ret == "int" and name not in _abi.NOT_STATUS), name
        assert (rule == "size") == (ret == "int64_t" and name.endswith(("_bytes", "_floats", "_ints"))), name
        if "hig_stream_t" in ctypes_:                       # every launcher returns a status
            assert rule == "status", name
    # the value-returning `int` functions are declared, return int, and take no stream
    assert {"hig_version", "hig_last_error", "hig_colsum_chunks"} <= set(_abi.NOT_STATUS) and len(set(_abi.NOT_STATUS)) == len(_abi.NOT_STATUS)
    for name in _abi.NOT_STATUS:
        assert name in parsed[3] and parsed[3][name][0] == "int", name
        assert "hig_stream_t" not in [t for _, t in parsed[3][name][1]], name
    # a parameter type outside the classes: named by function and parameter
    for decl, fn, param in (("int hig_made_up(const float* x, const double* weights);", "hig_made_up", "weights"),
                            ("int hig_made_up2(uint8_t flag);", "hig_made_up2", "flag"),
                            ("int hig_made_up3(const uint16_t*);", "hig_made_up3", "arg0")):
        with pytest.raises(_abi.HeaderError, match=r"%s.*`%s`" % (fn, param)):
            _abi.gateway(_abi.parse_header(decl)[3], {}, {})


def test_pointer_parameters_take_device_tensors_of_their_dtype_and_raw_values():
    f32, i32, i64 = torch.zeros(4), torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int64)
    raw = (None, C.c_void_p(64), (C.c_int64 * 2)(), 4096)
    # hig_masked_mse(pred, target, length, B, T, F, loss, dpred, scratch, s): the wrong dtype, by name and before anything else
    with pytest.raises(TypeError) as e:
        convert("hig_masked_mse", None, None, i32, 2, 3, 5, None, None, None)
    for part in ("hig_masked_mse", "`length`", "const int64_t*", "torch.int32"):
        assert part in str(e.value), (part, str(e.value))
    with pytest.raises(TypeError, match=r"hig_masked_mse.*`dpred` \(float\*\).*torch\.int64"):
        convert("hig_masked_mse", None, None, None, 2, 3, 5, None, i64, None)
    with pytest.raises(TypeError, match=r"`kpad` \(const uint8_t\*\).*torch\.float32"):
        _lib._GATEWAY["hig_fullattn_fwd_kpad"][2][11](f32)
    # the right dtype on the host: the no-CPU-fallback refusal, ptr()'s wording, with the parameter named
    with pytest.raises(RuntimeError, match=r"hig_masked_mse.*`pred` \(const float\*\).*needs ROCm device tensors \(got a cpu tensor\); there is no CPU fallback"):
        convert("hig_masked_mse", f32, None, None, 2, 3, 5, None, None, None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        convert("hig_masked_mse", None, None, i64, 2, 3, 5, None, None, None)
    with pytest.raises(RuntimeError, match=r"`dst` \(void\*\).*no CPU fallback"):                 # void*: any dtype, still a device tensor
        convert("hig_cast_bf16", None, i32, 4)
    # NULL, ctypes objects and plain addresses pass unchecked, as they are
    for v in raw:
        got = convert("hig_masked_mse", v, v, v, 2, 3, 5, v, v, v)
        assert all(g is v for g in got[:3] + got[6:9]) and got[3:6] == [2, 3, 5] and got[9] == 0xBEEF
    for bad in ("x", 1.5, [1, 2], b"abc"):
        with pytest.raises(TypeError, match=r"hig_masked_mse.*`pred`"):
            convert("hig_masked_mse", bad, None, None, 2, 3, 5, None, None, None)


def test_scalars_tables_structs_callbacks_and_streams():
    f32 = torch.zeros(4)
    # scalars: Python numbers, bool as int; a tensor would be a hidden synchronisation
    assert convert("hig_masked_mse", None, None, None, True, 3, 5, None, None, None)[3:6] == [1, 3, 5]
    assert convert("hig_cfg_combine", None, 2, 1, 1, 1, None)[1] == 2.0 and convert("hig_cfg_combine", None, 2.5, 1, 1, 1, None)[1] == 2.5
    for bad in (torch.tensor(2), torch.tensor([2]), 2.0, "2", None):
        with pytest.raises(TypeError, match=r"hig_masked_mse.*`B` \(int32_t\)"):
            convert("hig_masked_mse", None, None, None, bad, 3, 5, None, None, None)
    with pytest.raises(TypeError, match=r"`scale` \(float\).*hidden synchronisation"):
        convert("hig_cfg_combine", None, torch.tensor(2.0), 1, 1, 1, None)
    # pointer tables: ctypes arrays or None, never a tensor
    dims, table = _lib.Dims(B=2), (C.c_void_p * 3)()
    assert convert("hig_text_context", dims, table, None, None, 0)[1] is table
    assert convert("hig_text_context", dims, None, None, None, 0)[1] is None
    for name, args in (("hig_text_context", (dims, f32, None, None, 0)), ("hig_transpose_batch", (1, f32, None, None, None)),
                       ("hig_transpose_batch", (1, None, torch.zeros(2, dtype=torch.int64), None, None))):
        with pytest.raises(TypeError, match=r"%s.*(const void\* const\*|float\* const\*).*ctypes array" % name):
            convert(name, *args)
    # host extent arrays an entry reads before it returns: ctypes arrays for a typed pointer
    rows = (C.c_int32 * 2)(3, 4)
    assert convert("hig_transpose_batch", 2, None, None, rows, rows)[3] is rows
    # structs: the Structure itself goes by reference; a reference passes; another struct does not
    by_ref = convert("hig_workspace_bytes", dims, 0)[0]
    assert type(by_ref) is type(C.byref(dims)) and convert("hig_workspace_bytes", C.byref(dims), 0)[0] is not None
    for bad in (_lib.TextDims(), None, f32, 7):
        with pytest.raises(TypeError, match=r"hig_workspace_bytes.*`dims` \(const hig_dims\*\).*Dims"):
            convert("hig_workspace_bytes", bad, 0)
    # callbacks and streams (the hooked entries carry the stream in the middle: every argument is passed)
    cb = _lib.LAYER_HOOK(lambda user, layer: None)
    n = len(_lib._GATEWAY["hig_denoiser_bwd_hooked"][0])
    args = [dims] + [None] * (n - 5) + [None, cb, None, None]
    assert convert("hig_denoiser_bwd_hooked", *args)[-3] is cb
    args[-3] = None
    assert convert("hig_denoiser_bwd_hooked", *args)[-3] is None
    args[-3] = lambda user, layer: None
    with pytest.raises(TypeError, match=r"`hook` \(hig_layer_hook\)"):
        convert("hig_denoiser_bwd_hooked", *args)
    with pytest.raises(TypeError, match=r"hig_denoiser_bwd_hooked takes %d arguments \(or %d, without the stream\), got %d" % (n, n - 1, n - 2)):
        convert("hig_denoiser_bwd_hooked", *args[:-2])

    class FakeStream:
        cuda_stream = 0x1234

    sp = C.c_void_p(5)
    for given, passed in ((None, None), (77, 77), (sp, sp), (FakeStream(), 0x1234)):
        assert convert("hig_dec_timesteps", None, 2, given)[-1] is passed or convert("hig_dec_timesteps", None, 2, given)[-1] == passed
    with pytest.raises(TypeError, match=r"`s` \(hig_stream_t\)"):
        convert("hig_dec_timesteps", None, 2, f32)


def test_argument_counts():
    declared = "const float* pred, const float* target, const int64_t* length, int32_t B, int32_t T, int32_t F, float* loss, " \
               "float* dpred, float* scratch, hig_stream_t s"
    full = (None, None, None, 2, 3, 5, None, None, None)
    reads = []
    assert convert("hig_masked_mse", *full, 42, stream=lambda: reads.append(1))[-1] == 42 and not reads     # the declared count
    assert convert("hig_masked_mse", *full, stream=lambda: reads.append(1) or 7)[-1] == 7 and reads == [1]  # minus the stream: read now
    for args in (full + (42, 43), full[:-1], ()):                                                           # one too many, two too few
        with pytest.raises(TypeError) as e:
            convert("hig_masked_mse", *args)
        assert "hig_masked_mse takes 10 arguments (or 9, without the stream), got %d" % len(args) in str(e.value) and declared in str(e.value)
    # an entry whose last parameter is no stream takes the declared count only
    assert convert("hig_colsum_chunks", 1000) == [1000]
    for args in ((), (1000, 1)):
        with pytest.raises(TypeError, match=r"hig_colsum_chunks takes 1 arguments, got %d: \(int64_t rows\)" % len(args)):
            convert("hig_colsum_chunks", *args)
    with pytest.raises(TypeError, match=r"hig_workspace_bytes takes 2 arguments, got 1: \(const hig_dims\* dims, int training\)"):
        convert("hig_workspace_bytes", _lib.Dims())
    with pytest.raises(TypeError, match=r"hig_version takes 0 arguments, got 1"):
        convert("hig_version", 1)


def test_no_file_of_the_package_calls_the_library_around_the_gateway():
    pattern = re.compile(r"\b(L|lib\(\))\.hig_\w+\(")
    seen = 0
    for folder, _, files in os.walk(PACKAGE):
        for f in files:
            if f.endswith(".py") and f != "_lib.py":
                seen += 1
                text = open(os.path.join(folder, f)).read()
                assert not pattern.search(text), (f, pattern.search(text).group())
                assert "_lib.stream_ptr()" not in text and "P_ = _lib.ptr" not in text, f
    assert seen >= 20


def test_through_the_library_values_statuses_and_sizes():
    L = _lib.lib()
    assert _lib.api.hig_version() == L.hig_version() >= 100
    assert _lib.api.hig_colsum_chunks(1000) == L.hig_colsum_chunks(1000) == 62
    with pytest.raises(AttributeError, match="include/hig.h declares no hig_no_such_entry"):
        _lib.api.hig_no_such_entry
    assert _lib.api.hig_version is _lib.api.hig_version and _lib.api.hig_version.__name__ == "hig_version"
    # a size query the library refuses: its own message, not a 16-byte buffer
    bad = _lib.Dims(B=-1)
    assert L.hig_workspace_bytes(C.byref(bad), 0) < 0
    message = _lib.last_error()
    assert message
    for query in (lambda: _lib.api.hig_workspace_bytes(bad, 0), lambda: _lib.api.hig_bwd_workspace_bytes(bad),
                  lambda: _lib.api.hig_textctx_bytes(bad, 1)):
        with pytest.raises(RuntimeError) as e:
            query()
        assert str(e.value) == "libhig: " + _lib.last_error() and "libhig: " + message == str(e.value)
    # a status: check()'s exception, same text
    out = (C.c_int32 * _lib.DN_PLAN_NSLOTS)()
    rc = L.hig_denoiser_plan(C.byref(bad), _lib.DN_ENTRY_FWD32, 0, 0, 0, 0, 256, 1, None, out, _lib.DN_PLAN_NSLOTS)
    with pytest.raises(RuntimeError) as raw:
        _lib.check(rc)
    with pytest.raises(RuntimeError) as e:
        _lib.api.hig_denoiser_plan(bad, _lib.DN_ENTRY_FWD32, 0, 0, 0, 0, 256, 1, None, out, _lib.DN_PLAN_NSLOTS)
    assert rc != 0 and str(e.value) == str(raw.value) and str(e.value).startswith("libhig error %d: " % rc)
    with pytest.raises(RuntimeError, match="libhig error"):
        _lib.denoiser_plan(bad, _lib.DN_ENTRY_FWD32)
    # a value that may be negative ("none yet") is returned, not raised
    assert isinstance(_lib.api.hig_denoiser_last_schedule(out, _lib.DN_PLAN_NSLOTS), int)
    # importing the reader needs no torch
    import subprocess
    import sys
    code = "import sys, importlib.util as u; s = u.spec_from_file_location('a', %r); m = u.module_from_spec(s); s.loader.exec_module(m); " \
           "assert m.NOT_STATUS and 'torch' not in sys.modules" % os.path.join(PACKAGE, "_abi.py")
    assert subprocess.run([sys.executable, "-c", code], capture_output=True, timeout=60).returncode == 0
