"""The C ABI as ctypes, read from the header that declares it (include/mobgt_hip.h, include/mobgt_cpu.h), so that the binding
cannot drift from what the compiler checked the definitions against.  Standard library only.

The headers are regular: `ret mobgt_name(args);` prototypes and `#define MOBGT_NAME <int>` constants.  Anything the rules below
do not cover raises; nothing is guessed."""
import ctypes
import re

_SCALAR = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "double": ctypes.c_double,
           "uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32, "unsigned": ctypes.c_uint32, "unsigned int": ctypes.c_uint32}


def _scalar(decl, named):
    """ctypes twin of `int64_t ld` / `unsigned int` / ..., or None.  `named`: a parameter, whose last word may be its name."""
    words = [w for w in decl.split() if w != "const"]
    for w in (words, words[:-1]) if named else (words,):
        if " ".join(w) in _SCALAR:
            return _SCALAR[" ".join(w)]
    return None


def parse(text):
    """Header text -> ({name: (restype, [argtypes])} of every mobgt_* prototype, in order; {MOBGT_*: int} of the #defines)."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    consts = {m[1]: int(m[2]) for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(MOBGT_\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$", text, re.M)}
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)              # (a #define right in front of a prototype is not its type)
    protos = {}
    for stmt in re.split(r"[;{}]", text):
        m = re.fullmatch(r"\s*(.*?)\b(mobgt_\w+)\s*\((.*)\)\s*", stmt, re.S)
        if m is None:
            if re.search(r"\bmobgt_\w+\s*\(", stmt):
                raise ValueError(f"cannot read the declaration {' '.join(stmt.split())!r}")
            continue
        ret, name, params = " ".join(m[1].split()), m[2], m[3].strip()
        res = ctypes.c_char_p if ret.replace(" ", "") == "constchar*" else None if "*" in ret else _scalar(ret, named=False)
        if res is None:
            raise ValueError(f"{name}: unknown return type {ret!r}")
        args = []
        for p in ([] if params in ("", "void") else params.split(",")):
            t = ctypes.c_void_p if "*" in p else _scalar(p, named=True)
            if t is None:
                raise ValueError(f"{name}: unknown type in parameter {' '.join(p.split())!r}")
            args.append(t)
        protos[name] = (res, args)
    return protos, consts


def load(path):
    try:
        with open(path, encoding="utf-8") as f:
            return parse(f.read())
    except OSError as e:
        raise RuntimeError(f"{path}: the ctypes binding is derived from this header and cannot be built without it ({e})") from e


def bind(handle, signatures):
    for name, (res, args) in signatures.items():
        fn = getattr(handle, name)          # AttributeError here = header/library mismatch
        fn.restype = res
        fn.argtypes = args
    return handle
