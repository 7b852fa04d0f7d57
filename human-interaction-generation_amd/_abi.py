"""Reader of include/hig.h: the C ABI of libhig.so as data, and the ctypes classes that follow from it.

The header stays inside a small, closed subset of C (its opening comment lists the forms).  parse_header() takes the header's
text and returns its constants, structs, callback typedefs and prototypes; bind() turns those into ctypes Structures, CFUNCTYPEs
and (restype, argtypes) pairs.  A declaration outside the subset raises HeaderError naming it: nothing ever falls back to ctypes'
default `int` conversion.  Pure functions: no file is read, no library loaded, torch is not imported.
"""
import ctypes as C
import re

# `#define HIG_*` names whose body is not an integer: the include guard and the two function-like table-size macros
IGNORED_DEFINES = ("HIG_H", "HIG_D32_COUNT", "HIG_D16_COUNT")

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
    return [] if text in ("", "void") else [_declarator(p)[0] for p in text.split(",")]


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
    callbacks  {name: (return C type, [parameter C types])} of every `typedef ret (*name)(...);`
    prototypes {name: (return C type, [parameter C types])} of every function, in the header's order"""
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
        hooks[name] = C.CFUNCTYPE(ctype(ret, name, True), *[ctype(p, name) for p in params])
    signatures = {name: (ctype(ret, name, True), [ctype(p, name) for p in params]) for name, (ret, params) in prototypes.items()}
    return {struct_names[n]: c for n, c in classes.items()}, hooks, signatures
