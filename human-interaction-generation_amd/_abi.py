"""Reader of include/hig.h: the C ABI of libhig.so as data, and the ctypes classes that follow from it.

The header stays inside a small, closed subset of C (its opening comment lists the forms).  parse_header() takes the header's
text and returns its constants, structs, callback typedefs and prototypes; bind() turns those into ctypes Structures, CFUNCTYPEs
and (restype, argtypes) pairs; gateway() turns the prototypes into what every parameter of every function takes from Python and
what every result means, and convert() applies that to one call's arguments.  A declaration outside the subset raises HeaderError
naming it: nothing ever falls back to ctypes' default `int` conversion.  Pure functions: no file is read, no library loaded, torch
is not imported (a tensor is known by its attributes).
"""
import ctypes as C
import numbers
import re

# `#define HIG_*` names whose body is not an integer: the include guard and the two function-like table-size macros
IGNORED_DEFINES = ("HIG_H", "HIG_D32_COUNT", "HIG_D16_COUNT")
# `int` functions whose result is a value and not a status: a version, a length, a count of chunks or of table slots, a yes / no.
# Every other `int` function returns HIG_OK or an error code (each one that takes a hig_stream_t is a launcher and does)
NOT_STATUS = ("hig_version", "hig_last_error", "hig_text_head_layout", "hig_eval_encoder_layout", "hig_gemm_bf16_lnfold_plan",
              "hig_bf16_train_layout", "hig_f32_train_layout", "hig_colsum_chunks")

_SCALARS = {"int": C.c_int32, "int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float, "hig_stream_t": C.c_void_p}
_INT = re.compile(r"\(?\s*(-?\d+)\s*\)?$")


class HeaderError(ValueError):
    """A declaration of the header that the binding does not understand."""


def _statements(code):
    """The top-level declarations of `code`, split at each `;` outside braces (the closing brace of extern "C" is dropped)."""
    out, depth, start = [], 0, 0
    for m in re.finditer(r"[{};]", code):
        i, ch = m.start(), m.group()
        if ch == "{":
            depth += 1
        elif ch == "}" and depth == 0:
            if code[start:i].strip():
                raise HeaderError("declaration not understood: `%s }`" % " ".join(code[start:i].split())[:120])
            start = i + 1
        elif ch == "}":
            depth -= 1
        elif ch == ";" and depth == 0:
            out.append(" ".join(code[start:i].split()))
            start = i + 1
    out.append(" ".join(code[start:].split()))
    return [s for s in out if s]


def _spell(toks):
    return " ".join(toks).replace(" *", "*")


def _declarator(decl):
    """`const float* loss` -> ("const float*", "loss"); an unnamed parameter gives ("int64_t", None)."""
    toks = re.findall(r"\w+|\.\.\.|\S", decl)
    name = None
    if len(toks) > 1 and re.match(r"[A-Za-z_]\w*$", toks[-1]) and any(re.match(r"[A-Za-z_]", t) and t != "const" for t in toks[:-1]):
        name = toks.pop()
    return _spell(toks), name


def _params(text):
    text = text.strip()
    if text in ("", "void"):
        return []
    return [(name or "arg%d" % i, ctype) for i, (ctype, name) in enumerate(_declarator(p) for p in text.split(","))]


def _fields(struct, body):
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        first, *more = (d.strip() for d in decl.split(","))
        ctype, name = _declarator(first)
        if name is None or not all(re.match(r"[A-Za-z_]\w*$", m) for m in more) or re.search(r"[\[\]:()]", decl):
            raise HeaderError("%s: field declaration `%s` is not `type name[, name...]`" % (struct, decl))
        fields += [(n, ctype) for n in [name] + more]
    return fields


def parse_header(text):
    """(constants, structs, callbacks, prototypes) of the header `text`:
    constants  {name: int}: every `#define HIG_X <integer>` and every enum member (implicit values count on from the previous one)
    structs    {name: [(field, C type), ...]} of every `typedef struct hig_x { ... } hig_x;`
    callbacks  {name: (return C type, [(parameter, C type), ...])} of every `typedef ret (*name)(...);`
    prototypes {name: (return C type, [(parameter, C type), ...])} of every function, in the header's order
    An unnamed parameter goes by `arg<i>`, i its position."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    constants, structs, callbacks, prototypes = {}, {}, {}, {}

    def constant(name, value):
        if name in constants:
            raise HeaderError("%s: defined twice" % name)
        constants[name] = value

    code = []
    for line in text.split("\n"):
        if not line.lstrip().startswith("#"):
            code.append(line)
            continue
        m = re.match(r"\s*#\s*define\s+(\w+)(\([^)]*\))?\s*(.*?)\s*$", line)
        if m is None:
            continue                                        # #include / #if* / #endif
        name, args, body = m.groups()
        if name in IGNORED_DEFINES:
            continue
        value = _INT.match(body)
        if not name.startswith("HIG_") or args or value is None:
            raise HeaderError("%s: #define whose body `%s` is not an integer literal (and not in IGNORED_DEFINES)" % (name, body))
        constant(name, int(value.group(1)))
    code = re.sub(r'extern\s+"C"\s*\{', " ", "\n".join(code))

    for st in _statements(code):
        m = re.match(r"enum\s*\w*\s*\{(.*)\}$", st)
        if m:
            value = 0
            for member in filter(None, (s.strip() for s in m.group(1).split(","))):
                name, _, init = (s.strip() for s in member.partition("="))
                if init and not _INT.match(init):
                    raise HeaderError("%s: enum value `%s` is not an integer literal" % (name, init))
                value = int(_INT.match(init).group(1)) if init else value
                constant(name, value)
                value += 1
            continue
        m = re.match(r"typedef struct (\w+) \{(.*)\} (\w+)$", st)
        if m:
            if m.group(1) != m.group(3):
                raise HeaderError("%s: struct tag and typedef name differ (%s)" % (m.group(1), m.group(3)))
            structs[m.group(1)] = _fields(m.group(1), m.group(2))
            continue
        m = re.match(r"typedef (.+?)\(\s*\*\s*(\w+)\s*\)\s*\((.*)\)$", st)
        if m:
            callbacks[m.group(2)] = (_spell(re.findall(r"\w+|\S", m.group(1))), _params(m.group(3)))
            continue
        if st == "typedef void* hig_stream_t":
            continue
        m = re.match(r"([\w\s\*]+?)\b(\w+)\s*\((.*)\)$", st)
        if m is None or st.startswith("typedef") or "{" in st:
            raise HeaderError("declaration not understood: `%s`" % st[:120])
        if m.group(2) in prototypes:
            raise HeaderError("%s: declared twice" % m.group(2))
        prototypes[m.group(2)] = (_spell(re.findall(r"\w+|\S", m.group(1))), _params(m.group(3)))
    return constants, structs, callbacks, prototypes


def bind(structs, callbacks, prototypes, struct_names):
    """ctypes side of a parse: ({Python name: Structure}, {callback name: CFUNCTYPE}, {function: (restype, [argtypes])}).
    struct_names maps every header struct to the name of its Structure class."""
    classes, hooks = {}, {}

    def ctype(decl, where, is_return=False):
        bare = re.sub(r"^const ", "", decl)
        if decl.endswith("*"):
            if bare == "char*":
                return C.c_char_p
            return C.POINTER(classes[bare[:-1]]) if bare[:-1] in classes else C.c_void_p
        if bare == "void" and is_return:
            return None
        if bare in hooks:
            return hooks[bare]
        if bare in _SCALARS:
            return _SCALARS[bare]
        raise HeaderError("%s: %s, which the binding does not pass" % (where, "struct %s by value" % bare if bare in structs else
                                                                     "variadic arguments" if decl == "..." else "type `%s`" % decl))

    for name, fields in structs.items():
        if name not in struct_names:
            raise HeaderError("%s: a struct of the header without a Python name" % name)
        classes[name] = type(struct_names[name], (C.Structure,), {"_fields_": [(f, ctype(t, "%s.%s" % (name, f))) for f, t in fields]})
    for name, (ret, params) in callbacks.items():
        hooks[name] = C.CFUNCTYPE(ctype(ret, name, True), *[ctype(t, name) for _, t in params])
    signatures = {name: (ctype(ret, name, True), [ctype(t, name) for _, t in params]) for name, (ret, params) in prototypes.items()}
    return {struct_names[n]: c for n, c in classes.items()}, hooks, signatures


# ---- the gateway: what each parameter of each prototype accepts, and what each result means ----------------------------------

_TENSOR_OF = {"float": "torch.float32", "int32_t": "torch.int32", "int64_t": "torch.int64", "uint8_t": "torch.uint8"}
_DTYPE_NAMES = {}                                           # torch dtype -> its name, as the calls meet them
# what ctypes itself takes for a pointer: references (POINTER instances, byref() results), c_void_p / c_char buffers, arrays
_REF = (C._Pointer, type(C.byref(C.c_int32())))
_RAW = (C._SimpleCData, C.Array) + _REF


def _is_tensor(v):
    return hasattr(v, "data_ptr") and hasattr(v, "is_cuda")


def _got(v):
    return "a %s tensor of %s" % (v.device.type, v.dtype) if _is_tensor(v) else "%s (%s)" % (repr(v)[:60], type(v).__name__)


def _converter(fn, name, ctype, classes, hooks):
    """What turns one Python argument into what ctypes passes for parameter `name` of `fn`, declared `ctype`."""
    where = "%s: parameter `%s` (%s)" % (fn, name, ctype)
    bare = re.sub(r"^const ", "", ctype)

    def refuse(v, takes):
        return TypeError("%s takes %s, got %s" % (where, takes, _got(v)))

    if bare in ("int", "int32_t", "int64_t", "float"):
        kind, cast = (numbers.Real, float) if bare == "float" else (numbers.Integral, int)

        def scalar(v):
            if type(v) is cast:
                return v
            if isinstance(v, kind):
                return cast(v)
            raise refuse(v, "a Python number (reading a tensor here would be a hidden synchronisation)" if _is_tensor(v) else "a Python number")
        return scalar
    if bare == "hig_stream_t":
        def stream(v):
            if v is None or type(v) is int or isinstance(v, C.c_void_p):
                return v
            if hasattr(v, "cuda_stream"):
                return v.cuda_stream
            raise refuse(v, "a torch.cuda.Stream, a c_void_p, an address or None")
        return stream
    if bare in hooks:
        def callback(v):
            if v is None or isinstance(v, hooks[bare]):
                return v
            raise refuse(v, "a %s instance or None" % bare)
        return callback
    if not bare.endswith("*"):
        raise HeaderError("%s, which the gateway does not pass" % where)
    pointee = bare[:-1]
    if pointee in classes:
        def struct(v):
            if isinstance(v, classes[pointee]):
                return C.byref(v)
            if isinstance(v, _REF):
                return v
            raise refuse(v, "a %s (passed by reference)" % classes[pointee].__name__)
        return struct
    if "*" in pointee:                                      # `void* const*`, `const float* const*`, ...
        def table(v):
            if v is None or isinstance(v, _RAW):
                return v
            raise refuse(v, "a ctypes array of pointers or None")
        return table
    if pointee == "char":
        def chars(v):
            if isinstance(v, _RAW):
                return v
            raise refuse(v, "a ctypes character buffer")
        return chars
    if pointee != "void" and pointee not in _TENSOR_OF:
        raise HeaderError("%s, which the gateway does not pass" % where)
    dtype = _TENSOR_OF.get(pointee)
    takes = "a ROCm device tensor%s, None, or a raw ctypes value / address" % (" of %s" % dtype if dtype else "")

    def pointer(v):
        if v is None:
            return None
        got = getattr(v, "dtype", None)
        if got is not None and hasattr(v, "data_ptr"):      # a tensor
            if dtype is not None and (_DTYPE_NAMES.get(got) or _DTYPE_NAMES.setdefault(got, str(got))) != dtype:
                raise refuse(v, takes)
            if not v.is_cuda:
                raise RuntimeError("%s: libhig needs ROCm device tensors (got a %s tensor); there is no CPU fallback" % (where, v.device.type))
            return v.data_ptr()
        if type(v) is int or isinstance(v, _RAW):
            return v
        raise refuse(v, takes)
    return pointer


def gateway(prototypes, classes, hooks):
    """{function: (names, C types, converters, result rule)} for every prototype of a parse; classes / hooks: {header name:
    Structure / CFUNCTYPE}.  One converter per parameter takes what the declared type admits and refuses the rest by name:
      float, int, int32_t, int64_t     Python numbers (bool as int); a tensor is refused
      T* / const T*                    T in float, int32_t, int64_t, uint8_t: a ROCm device tensor of exactly that dtype, None for
                                       NULL; a ctypes object or a plain integer address passes unchecked (raw workspace bytes given to
                                       a typed parameter on purpose, and host arrays an entry reads before it returns)
      void* / const void*              any device tensor, None, or a raw value as above
      pointer to pointer               ctypes arrays or None
      const hig_x*                     the Structure itself (passed by reference), or a reference
      a callback type                  its CFUNCTYPE instance or None
      hig_stream_t                     c_void_p, an address, None, or a torch.cuda.Stream
    Contiguity, shape and alignment are not checked: the header does not state them, the entry points take leading dimensions, and
    strided views are legitimate operands.  The result rule is "status" (an `int` that is HIG_OK or an error code), "size" (an
    int64_t count of bytes / floats / ints, negative on refusal) or "value".  A type outside these raises HeaderError."""
    out = {}
    for fn, (ret, params) in prototypes.items():
        rule = "status" if ret == "int" and fn not in NOT_STATUS else \
               "size" if ret == "int64_t" and fn.endswith(("_bytes", "_floats", "_ints")) else "value"
        out[fn] = (tuple(n for n, _ in params), tuple(t for _, t in params),
                   tuple(_converter(fn, n, t, classes, hooks) for n, t in params), rule)
    return out


def convert(fn, entry, args, current_stream):
    """The ctypes arguments of one call of `fn` (entry: its gateway() value).  The declared count is accepted, and one fewer when
    the last parameter is a hig_stream_t, which then is current_stream(), read now."""
    names, ctypes_, converters, _ = entry
    if len(args) != len(names):
        if len(args) != len(names) - 1 or not names or ctypes_[-1] != "hig_stream_t":
            raise TypeError("%s takes %d arguments%s, got %d: (%s)" % (
                fn, len(names), " (or %d, without the stream)" % (len(names) - 1) if names and ctypes_[-1] == "hig_stream_t" else "",
                len(args), ", ".join("%s %s" % (t, n) for n, t in zip(names, ctypes_))))
        return [c(a) for c, a in zip(converters, args)] + [current_stream()]
    return [c(a) for c, a in zip(converters, args)]
