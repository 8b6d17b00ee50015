"""The one reader of include/mmloam_hip.h for the tests: every mml_* declaration as (return kind, [parameter kinds]) and the
header's integer #defines.  Kinds are the words of the package's type rule (SIGNATURES in multi-modal-loam_amd/__init__.py):
"ptr" for any pointer, else the C scalar type with `const` dropped; a return is "int", "void", "char*" or "ptr"."""
import ctypes as C
import re

SCALAR_KINDS = ("int", "unsigned", "long", "long long", "int64_t", "uint64_t", "size_t", "float", "double")
CTYPE_OF_KIND = {"ptr": C.c_void_p, "int": C.c_int, "unsigned": C.c_uint, "long": C.c_long, "long long": C.c_longlong,
                 "int64_t": C.c_int64, "uint64_t": C.c_uint64, "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double}
RESTYPE_OF_KIND = {"int": C.c_int, "void": None, "char*": C.c_char_p, "ptr": C.c_void_p}

_DECL = re.compile(r"(?:^|[;}])\s*((?:const\s+)?\w[\w\s]*?[\s*]+)(mml_\w+)\s*\(([^()]*)\)\s*(?=;)")


def strip_comments(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def _param_kind(p):
    if "*" in p or "[" in p:
        return "ptr"
    words = [w for w in p.split() if w != "const"]
    kind = " ".join(words[:-1])          # the last word is the parameter's name
    if kind not in SCALAR_KINDS:
        raise ValueError("parameter %r: not a pointer and not one of %s" % (p, SCALAR_KINDS))
    return kind


def _return_kind(r):
    r = " ".join(r.replace("*", " * ").split())
    if r == "const char *":
        return "char*"
    if "*" in r:
        return "ptr"
    if r not in ("int", "void"):
        raise ValueError("return type %r: not int, void or a pointer" % r)
    return r


def parse_declarations(text):
    """{name: (return kind, [parameter kinds])} for every mml_* function declared in the C text."""
    body = "\n".join(l for l in strip_comments(text).splitlines() if not l.lstrip().startswith("#"))
    out = {}
    for ret, name, params in _DECL.findall(body):
        if "typedef" in ret.split():
            continue
        params = " ".join(params.split())
        kinds = [] if params in ("", "void") else [_param_kind(p.strip()) for p in params.split(",")]
        if name in out and out[name] != (_return_kind(ret), kinds):
            raise ValueError("%s is declared twice, differently" % name)
        out[name] = (_return_kind(ret), kinds)
    return out


def parse_defines(text):
    """{NAME: int} for every object-like #define whose value is an integer expression (digits, shifts, + - *, parentheses)."""
    out = {}
    for name, val in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+([^\n]+)$", strip_comments(text), flags=re.M):
        val = re.sub(r"\b(\d+)[uUlL]+\b", r"\1", val.strip())
        if re.fullmatch(r"[\d\s()<>+*-]+", val) and re.search(r"\d", val):
            out[name] = int(eval(val, {"__builtins__": {}}))   # (only digits and operators reach this)
    return out


def ctypes_signature(decl):
    """(restype, [argtypes]) the type rule gives for one (return kind, [parameter kinds])."""
    ret, kinds = decl
    return RESTYPE_OF_KIND[ret], [CTYPE_OF_KIND[k] for k in kinds]


def read_header(path):
    """(declarations, defines) of the header at `path`."""
    text = open(path).read()
    return parse_declarations(text), parse_defines(text)
