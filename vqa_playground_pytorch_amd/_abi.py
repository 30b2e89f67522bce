"""A C-ABI header (include/vqa_mi355x.h) read as the binding's one source: prototypes, structs and integer #defines -> ctypes.

    parse(text)            -> (functions, structs, defines)
                              functions  {name: (return C type, [(parameter name, C type), ...])}, in declaration order
                              structs    {name: [(field name, C type), ...]}
                              defines    {name: int}
    ctype(c_type, where)   the ctypes type of a C type by the table below; a type that is not in it raises AbiError naming `where`
                           and the type -- a new header type fails at import, it never binds as something else
    signatures(functions)  -> ({name: (restype, [argtypes])}, {name: [parameter names]})
    struct_class(name, fields)

C types are compared with `const` dropped and every `*` set apart ("const float* const*" is "float * *").  Every pointer is a
c_void_p -- device pointers, host arrays of them, workspaces, the stream -- except `char *`, a c_char_p.  Text that is neither a
prototype, a struct, a plain typedef nor the extern "C" bracket raises as well: nothing of the header is skipped in silence.
This module imports nothing of the package; _lib.py hands it the header's text."""
import ctypes
import re

SCALARS = {
    "int": ctypes.c_int,
    "long": ctypes.c_long,
    "long long": ctypes.c_longlong,
    "unsigned long long": ctypes.c_ulonglong,
    "size_t": ctypes.c_size_t,
    "uint64_t": ctypes.c_uint64,
    "uint32_t": ctypes.c_uint32,
    "float": ctypes.c_float,
    "double": ctypes.c_double,
    "vqa_stream_t": ctypes.c_void_p,
}

_DEFINE = re.compile(r"^[ \t]*#[ \t]*define[ \t]+(VQA_\w+)[ \t]+\(?[ \t]*(-?\d+)[ \t]*\)?[ \t]*$", re.M)
_STRUCT = re.compile(r"typedef\s+struct\s+\w+\s*\{([^{}]*)\}\s*(\w+)\s*;")
_PROTOTYPE = re.compile(r"([\w \t*]+?)\b(vqa_\w+)\s*\(([^()]*)\)\s*;")
_IGNORED = re.compile(r'typedef[^;{}]*;|extern\s+"C"\s*\{|\}')


class AbiError(ValueError):
    """the header holds something this reader does not know"""


def _norm(c_type):
    return " ".join(t for t in c_type.replace("*", " * ").split() if t != "const")


def ctype(c_type, where, ret=False):
    t = _norm(c_type)
    if t == "void" and ret:
        return None
    if t == "char *":
        return ctypes.c_char_p
    if t.endswith("*"):
        return ctypes.c_void_p
    if t not in SCALARS:
        raise AbiError("%s: no ctypes type for the C type %r" % (where, t))
    return SCALARS[t]


def _declarator(text):
    """'const float* const* w1' -> ('w1', 'float * *')"""
    tokens = _norm(text).split()
    return tokens[-1], " ".join(tokens[:-1])


def parse(text):
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    defines = {m.group(1): int(m.group(2)) for m in _DEFINE.finditer(text)}
    text = re.sub(r"^[ \t]*#[^\n]*", " ", text, flags=re.M)
    structs = {}
    for m in _STRUCT.finditer(text):
        fields = structs[m.group(2)] = []
        for decl in filter(None, (d.strip() for d in m.group(1).split(";"))):
            first, *more = decl.split(",")          # `int a, b;`: every name of a list has the first one's type
            name, c_type = _declarator(first)
            fields += [(name, c_type)] + [(n.strip(), c_type) for n in more]
            if not all(re.fullmatch(r"\w+", f) for f, _ in fields):
                raise AbiError("%s: cannot read the declaration %r" % (m.group(2), decl))
    text = _STRUCT.sub(" ", text)
    functions = {}
    for m in _PROTOTYPE.finditer(text):
        params = m.group(3).strip()
        functions[m.group(2)] = (_norm(m.group(1)), [] if params == "void" else [_declarator(p) for p in params.split(",")])
    rest = _IGNORED.sub(" ", _PROTOTYPE.sub(" ", text)).strip()
    if rest:
        raise AbiError("cannot read the header from %r on" % rest[:60])
    return functions, structs, defines


def signatures(functions):
    sigs, names = {}, {}
    for fn, (ret, params) in functions.items():
        sigs[fn] = (ctype(ret, fn, ret=True), [ctype(t, "%s(%s)" % (fn, p)) for p, t in params])
        names[fn] = [p for p, _ in params]
    return sigs, names


def struct_class(name, fields):
    return type(name, (ctypes.Structure,), {"_fields_": [(f, ctype(t, "%s.%s" % (name, f))) for f, t in fields]})
