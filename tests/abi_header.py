"""include/rt_amd.h read once, for every test that holds the binding (rt_amd.py) to it.  A helper module: no tests here.

PROTOTYPES[name] = (restype, [argtypes]), PARAM_NAMES[name] = [parameter names] and PARAM_C_TYPES[name] = [their C types as the header
spells them, one space between words, * or [n] at the end] for every function the header declares,
STRUCTS[rt_X] = [(field, ctype)] for every `typedef struct rt_X { ... }`, DEFINES[RT_NAME] = int or float for every #define whose value
is one numeric literal (in parentheses or with an f suffix at most; any other #define is left out).
The ctypes of a prototype follow one rule: scalars by name, rt_partition by value, a pointer to a struct that rt_amd mirrors as
POINTER(that class), `const char*` as c_char_p, any other pointer or array as c_void_p; EXCEPTIONS names what departs from it.  A type
the rule does not know raises HeaderError: nothing falls back to c_void_p."""
import ctypes as C
import os
import re

import rt_amd

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rt_amd.h")


class HeaderError(Exception):
    pass


SCALARS = {"int": C.c_int, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t, "int32_t": C.c_int32, "uint32_t": C.c_uint32,
           "int64_t": C.c_int64, "uint64_t": C.c_uint64, "uint16_t": C.c_uint16}
# header struct -> the ctypes.Structure of rt_amd that mirrors it (the other structs travel as numpy dtypes or opaque handles)
MIRRORS = {"rt_partition": rt_amd.Partition, "rt_adaptive": rt_amd.Adaptive, "rt_budget": rt_amd.Budget, "rt_denoise_params": rt_amd.DenoiseParams,
           "rt_denoise_var_params": rt_amd.DenoiseVarParams, "rt_temporal_params": rt_amd.TemporalParams,
           "rt_temporal_rectify": rt_amd.TemporalRectify, "rt_temporal_inputs": rt_amd.TemporalInputs, "rt_levels_params": rt_amd.LevelsParams,
           "rt_frame_metrics": rt_amd.FrameMetrics}
# (function, parameter) -> ctype, where the rule above is not what the binding should send, each with its reason
EXCEPTIONS = {
    # a DEVICE pointer the kernel writes the record through: the binding passes a tensor's address, never a host FrameMetrics
    ("rt_frame_compare", "d_metrics"): C.c_void_p,
    # rt_gather_fn, the header's one function-pointer typedef: the binding passes the address of a CFUNCTYPE thunk
    ("rt_multi_init_custom", "gather"): C.c_void_p,
}


def _ctype(base, pointer, known, where):
    """the rule: base is the type without const, pointer whether a * or [] follows it"""
    const = "const" in base.split()
    base = " ".join(w for w in base.split() if w not in ("const", "struct"))
    if pointer:
        if base in MIRRORS and base != "rt_partition":
            return C.POINTER(MIRRORS[base])
        if base == "char" and const:
            return C.c_char_p
        if base in ("void", "char") or base in SCALARS or base in known:
            return C.c_void_p
    elif base in SCALARS:
        return SCALARS[base]
    elif base == "rt_partition":
        return MIRRORS[base]
    raise HeaderError("%s: unknown type %r%s" % (where, base, " (pointer)" if pointer else ""))


def _declarator(text, where):
    """'const float lookfrom[3]' -> ('const float', 'lookfrom', True, 3)"""
    m = re.fullmatch(r"(.*?)(\**)\s*(\w+)\s*(?:\[(\w*)\])?", text.strip(), re.S)
    if not m or not m.group(1).strip():
        raise HeaderError("%s: cannot read %r" % (where, text))
    return m.group(1).strip(), m.group(3), bool(m.group(2)) or m.group(4) is not None, m.group(4)


def parse(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    defines = {}
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(RT_\w+)[ \t]+(\S.*?)[ \t]*$", text, re.M):
        v = value.strip("()")
        if re.fullmatch(r"-?\d+", v):
            defines[name] = int(v)
        elif re.fullmatch(r"-?(\d+\.?\d*|\.\d+)(e-?\d+)?f?", v):
            defines[name] = float(v.rstrip("f"))
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{', " ", text)
    bodies = re.findall(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;", text, re.S)
    text = re.sub(r"typedef\s+struct\s+\w+\s*\{.*?\}\s*\w+\s*;", " ", text, flags=re.S)
    known = {n for n, _, _ in bodies} | set(re.findall(r"typedef\s+struct\s+(\w+)\s+\1\s*;", text))
    text = re.sub(r"typedef\b[^;]*;", " ", text)
    structs = {}
    for name, body, alias in bodies:
        if name != alias:
            raise HeaderError("typedef struct %s is named %s" % (name, alias))
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            first, *more = decl.split(",")
            base, field, pointer, count = _declarator(first, name)
            for f, p, c in [(field, pointer, count)] + [_declarator(base + " " + d, name)[1:] for d in more]:
                if c:
                    fields.append((f, _ctype(base, False, known, name) * int(c)))
                else:
                    fields.append((f, _ctype(base, p, known, name)))
        structs[name] = fields
    prototypes, names, c_types = {}, {}, {}
    for stmt in filter(None, (s.strip() for s in text.split(";"))):
        m = re.fullmatch(r"(.*?)\b(rt_\w+)\s*\((.*)\)", stmt, re.S)
        if not m:
            if stmt != "}":             # the end of extern "C"
                raise HeaderError("cannot read %r" % stmt)
            continue
        ret, fn, params = m.groups()
        args, argnames, spelt = [], [], []
        if params.strip() != "void":
            for p in params.split(","):
                base, arg, pointer, count = _declarator(p, fn)
                spelt.append(" ".join(base.split()) + ("*" if count is None and pointer else "") + ("" if count is None else "[%s]" % count))
                args.append(EXCEPTIONS.get((fn, arg)) or _ctype(base, pointer, known, "%s(%s)" % (fn, arg)))
                argnames.append(arg)
        pointer = ret.strip().endswith("*")
        prototypes[fn] = (_ctype(ret.replace("*", " "), pointer, known, fn), args)
        names[fn], c_types[fn] = argnames, spelt
    for fn, arg in EXCEPTIONS:
        if arg not in names.get(fn, ()):
            raise HeaderError("the exception %s(%s) names nothing the header declares" % (fn, arg))
    return prototypes, names, c_types, structs, defines


PROTOTYPES, PARAM_NAMES, PARAM_C_TYPES, STRUCTS, DEFINES = parse(open(HEADER).read())


def layout(name):
    """a ctypes.Structure laid out as the C compiler lays out the header's struct: sizeof and the field offsets are the header's"""
    return type("hdr_" + name, (C.Structure,), {"_fields_": STRUCTS[name]})


def check_bound(rt, names):
    """every name is declared by the header, bound with the header's types, and exported by the library"""
    L = rt.lib()
    for name in names:
        assert name in PROTOTYPES, "%s is not declared in rt_amd.h" % name
        assert name in rt.SYMBOLS, "%s is not in rt_amd.SYMBOLS" % name
        assert tuple(rt.SYMBOLS[name]) == PROTOTYPES[name], "%s: binding %s, header %s" % (name, rt.SYMBOLS[name], PROTOTYPES[name])
        assert hasattr(L, name), "librt_amd.so does not export %s" % name


def check_struct(cls, name):
    """the Structure `cls` has the fields of the header's struct, in order, and its size"""
    assert MIRRORS[name] is cls
    assert cls._fields_ == STRUCTS[name], "%s: binding %s, header %s" % (name, cls._fields_, STRUCTS[name])
    assert C.sizeof(cls) == C.sizeof(layout(name)), name
