"""ctypes binding of libvlhip.so (C ABI declared in include/vlhip.h).

The product path has NO fallback: if the shared library is missing or a symbol cannot be resolved the
import of the native ops fails loudly (RuntimeError), and every native op refuses CPU tensors.
"""
import ctypes
import os
import re
from ctypes import c_char_p, c_float, c_int, c_int64, c_uint64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VLHIP_LIBRARY") or os.path.join(_HERE, "csrc", "libvlhip.so")  # override: A/B builds
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "vlhip.h")

_SCALARS = {"int": c_int, "int64_t": c_int64, "uint64_t": c_uint64, "float": c_float}
_header = _constants = None


def _header_text():
    """include/vlhip.h without its comments; read once per process."""
    global _header
    if _header is None:
        with open(HEADER_PATH) as f:
            _header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return _header


def header_symbols():
    """Every function name declared in include/vlhip.h."""
    return sorted(set(re.findall(r"\b(vl_[a-z0-9_]+)\s*\(", _header_text())))


def header_constants():
    """{name: value} of the `NAME = value` enumerators and `#define NAME value` integer constants of include/vlhip.h
    (descriptor field indices of vl_stack_*, table widths, epilogue / activation codes): the header is the single source of
    truth for the binding.  Parsed once; every call returns a dict of its own."""
    global _constants
    if _constants is None:
        text, out = _header_text(), {}
        for name, val in re.findall(r"\b(VL_[A-Z0-9_]+)\s*=\s*(-?\d+)", text):
            out[name] = int(val)
        for name, val in re.findall(r"#define\s+(VL_[A-Z0-9_]+)\s+(0x[0-9a-fA-F]+|-?\d+)(?:ll)?\b", text):
            out[name] = int(val, 0)
        _constants = out
    return dict(_constants)


def parse_signatures(text):
    """{name: (restype, [argtypes])} of every `RET vl_name(args);` declaration of the comment-stripped header `text`: a
    parameter with a `*` is a c_void_p, a scalar one must be of a type in _SCALARS, `(void)` is no arguments.  Raises
    RuntimeError on whatever it does not understand -- a guessed binding would pass garbage to a kernel."""
    text = re.sub(r'^\s*#.*$|extern\s+"C"\s*\{', "", text, flags=re.M)
    sigs = {}
    stmts = text.split(";")
    for i, stmt in enumerate(stmts):
        names = re.findall(r"\bvl_\w+", stmt)
        if not names:
            continue
        m = i + 1 < len(stmts) and re.fullmatch(r"\s*([\w\s*]+?)\s*\b(vl_\w+)\s*\(([^()]*)\)\s*", stmt)
        if not m:  # (what follows the last `;` is no declaration)
            raise RuntimeError("clg_vqa_amd: cannot parse the declaration of %s in include/vlhip.h: %r"
                               % (names[0], " ".join(stmt.split())))
        ret, name, args = " ".join(m.group(1).split()), m.group(2), m.group(3).strip()
        if ret != "const char*" and ret not in _SCALARS:
            raise RuntimeError("clg_vqa_amd: %s in include/vlhip.h: unknown return type %r" % (name, ret))
        argtypes = []
        for arg in ([] if args == "void" else args.split(",")):
            arg = " ".join(arg.split())
            scalar = re.fullmatch(r"(?:const )?(\w+) \w+", arg)
            if "*" in arg:
                argtypes.append(c_void_p)
            elif scalar is not None and scalar.group(1) in _SCALARS:
                argtypes.append(_SCALARS[scalar.group(1)])
            else:
                raise RuntimeError("clg_vqa_amd: %s in include/vlhip.h: unknown parameter %r" % (name, arg))
        if name in sigs:
            raise RuntimeError("clg_vqa_amd: %s is declared twice in include/vlhip.h" % name)
        sigs[name] = (c_char_p if ret == "const char*" else _SCALARS[ret], argtypes)
    return sigs


_SIGS = parse_signatures(_header_text())  # the whole binding: declaring an entry point in the header is all it takes

_lib = None


def lib():
    """The loaded library; raises RuntimeError (never falls back) when it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "clg_vqa_amd: native library %s is missing -- run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or `make -C clg-vqa_amd/csrc`).  There is no CPU / eager fallback for the product path." % LIB_PATH)
        handle = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            try:
                fn = getattr(handle, name)
            except AttributeError as e:
                raise RuntimeError("clg_vqa_amd: %s does not export %s" % (LIB_PATH, name)) from e
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


def check(rc, what=""):
    if rc != 0:
        msg = lib().vl_last_error().decode(errors="replace")
        raise RuntimeError("vlhip %s failed (code %d): %s" % (what, rc, msg))
