"""ctypes binding of libiswm_hip.so, derived from include/iswm_hip.h (and its extension headers include/iswm_hip_sep.h,
include/iswm_hip_kd.h, include/iswm_hip_bd.h, include/iswm_hip_bm.h and include/iswm_hip_cr.h, whose prototypes go to tables of
their own, EXT_EXPORTS / _EXT_SIGS, KD_EXPORTS / _KD_SIGS, BD_EXPORTS / _BD_SIGS, BM_EXPORTS / _BM_SIGS and CR_EXPORTS / _CR_SIGS,
parsed with the main header's types in scope) at import.

The header is the only declaration of the C ABI.  It is parsed once here -- `re` and `ctypes`, nothing generated, neither
the library nor torch loaded -- into
    CONSTANTS   every `#define ISWM_* <integer>` and `enum { NAME = <integer>, ... };`
    STRUCTS     a ctypes.Structure per `typedef struct [tag] { ... } name;` (scalars, `T name[N]`, `int H, W;`, pointers)
    _SIGS       (restype, argtypes) per prototype, in header order
so an entry point needs its header line and its definition to be callable from Python.  The header keeps to that subset
of C; a declaration outside it (an unknown type, a function pointer, a bit-field, a prototype that does not split)
raises ValueError at import with the declaration in the message -- the parser never guesses.

Types: the scalars of `_SCALARS`; `char*` -> c_char_p; a pointer to one of the header's records -> POINTER(record);
every other pointer (`T**`, `T* const*`, `T name[]` included) -> c_void_p.  Host arrays (mean3 / std3, the ASPP ksize /
dil lists, arrays of device pointers, `int*` outputs) are therefore c_void_p like device pointers: they take the ctypes
arrays and byref() results the callers pass, and a bare integer passed there is no longer an ArgumentError.

The product path has NO fallback: if the shared library is missing or a symbol
cannot be resolved, importing the ops raises -- nothing silently routes through
torch ops or the CPU oracle.
"""
import ctypes
import functools
import os
import re
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int64, c_size_t, c_uint64, c_void_p

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libiswm_hip.so")
HEADER = os.path.join(os.path.dirname(HERE), "include", "iswm_hip.h")
EXT_HEADER = os.path.join(os.path.dirname(HERE), "include", "iswm_hip_sep.h")
KD_HEADER = os.path.join(os.path.dirname(HERE), "include", "iswm_hip_kd.h")
BD_HEADER = os.path.join(os.path.dirname(HERE), "include", "iswm_hip_bd.h")
BM_HEADER = os.path.join(os.path.dirname(HERE), "include", "iswm_hip_bm.h")
CR_HEADER = os.path.join(os.path.dirname(HERE), "include", "iswm_hip_cr.h")

# (`long long` is 8 bytes on every ABI the library is built for; tests/test_abi_cpu.py holds that)
_SCALARS = {"int": c_int, "int64_t": c_int64, "long long": c_int64, "size_t": c_size_t, "float": c_float,
            "double": c_double, "uint64_t": c_uint64}
_POINTEES = {"void", "char", "unsigned char", "signed char", "uint8_t", "int32_t", "uint32_t"}    # pointed to, never by value


def parse_header(text, base=None):
    """(CONSTANTS, STRUCTS, _SIGS) of a header written in the subset of C the module docstring names.  base: the text of the
    header this one includes; its records and typedefs may be used, and only what `text` itself declares is returned (a name
    declared in both is a ValueError)."""
    if base is None:
        return tuple(dict(t) for t in _parsed(text)[:3])
    tables = tuple(dict(t) for t in _parsed(base))         # (the record classes are the base's own: one POINTER type each)
    inherited = [set(t) for t in tables[:3]]
    redeclared = _scan_header(text, *tables, taken=set().union(*inherited))
    if redeclared:
        raise ValueError("iswm_hip.h: an extension header declares %s again" % sorted(redeclared))
    return tuple({k: v for k, v in t.items() if k not in old} for t, old in zip(tables, inherited))


@functools.lru_cache(maxsize=None)
def _parsed(text):
    """(constants, structs, sigs, typedef'd scalars, resolved types) of one header text, parsed once"""
    tables = ({}, {}, {}, dict(_SCALARS), {})
    _scan_header(text, *tables)
    return tables


def _scan_header(text, constants, structs, sigs, scalars, known, taken=()):
    """parse_header's pass over one header text, into the tables; returns the names of `taken` it declares again"""
    declared = []

    def bad(why, decl):
        return ValueError("iswm_hip.h: %s: %r" % (why, " ".join(decl.split())))

    def integer(v, decl):
        try:
            return int(v, 0)
        except ValueError:
            raise bad("%r is not an integer" % v.strip(), decl)

    def declarator(d, decl):
        """(type text, name, array) of `T name`, `T name[]` (array "") or `T name[N]`; array None otherwise"""
        m = re.fullmatch(r"([\w\s*]*[\s*])(\w+)\s*(?:\[\s*(\d*)\s*\])?", d.strip())
        if not m:
            raise bad("cannot read %r" % d.strip(), decl)
        return m.groups()

    def ctype(t, decl, array=None):
        if (t, array) not in known:
            known[t, array] = resolve(t, decl, array)
        return known[t, array]

    def resolve(t, decl, array):
        m = re.fullmatch(r"(?:const\s+)?(\w+(?:\s+\w+)*?)(?:\s+const)?((?:\s*\*(?:\s*const)?)*)", t.strip())
        if not m:
            raise bad("cannot read the type %r" % t.strip(), decl)
        base, stars = " ".join(m.group(1).split()), m.group(2).count("*")
        if base not in scalars and base not in structs and base not in _POINTEES:
            raise bad("unknown type %r" % base, decl)
        if stars == 0 and base not in scalars:
            raise bad("%r is only taken by pointer" % base, decl)
        one = (scalars[base] if stars == 0 else c_char_p if (stars, base) == (1, "char") else
               POINTER(structs[base]) if stars == 1 and base in structs else c_void_p)
        if array == "":
            raise bad("an array member needs a length", decl)
        return one if array is None else one * int(array)

    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    for line in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(\S[^\n]*)", text, re.M):    # (the include guard has no value)
        constants[line[0]] = integer(line[1], "#define %s %s" % line)
        declared.append(line[0])
    text = re.sub(r"^[ \t]*#[^\n]*", " ", text, flags=re.M)
    m = re.fullmatch(r'\s*extern\s+"C"\s*\{(.*)\}\s*', text, re.S)
    body, one = m.group(1) if m else text, r"((?:[^;{}]|\{[^{}]*\})*);"          # up to the next `;` outside braces
    if re.sub(one, "", body).strip():
        raise bad("no `;` behind", re.sub(one, "", body))
    for decl in (d.strip() for d in re.findall(one, body)):
        m = re.fullmatch(r"enum\s*\{(.*)\}", decl, re.S)
        if m:
            for item in m.group(1).split(","):
                name, eq, value = item.partition("=")
                if not eq or not re.fullmatch(r"\s*\w+\s*", name):
                    raise bad("an enumerator needs `NAME = <integer>`", decl)
                constants[name.strip()] = integer(value, decl)
                declared.append(name.strip())
            continue
        m = re.fullmatch(r"typedef\s+struct(?:\s+\w+)?\s*\{(.*)\}\s*(\w+)", decl, re.S)
        if m:
            *members, rest = m.group(1).split(";")
            if rest.strip():
                raise bad("no `;` behind %r" % rest.strip(), decl)
            fields = []
            for first, *more in (member.split(",") for member in members):
                t, name, array = declarator(first, decl)
                if more and "*" in t:
                    raise bad("a comma list of pointers", decl)
                fields += [(name, ctype(t, decl, array))] + [(n, ctype(t, decl, a)) for _, n, a in
                                                             (declarator(t + d, decl) for d in more)]
            structs[m.group(2)] = type(m.group(2), (ctypes.Structure,), {"_fields_": fields})
            declared.append(m.group(2))
            continue
        m = re.fullmatch(r"typedef\s+([\w\s*]*[\s*])(\w+)", decl)
        if m:
            scalars[m.group(2)] = ctype(m.group(1), decl)
            continue
        m = re.fullmatch(r"([\w\s*]*[\s*])(\w+)\s*\(([^()]*)\)", decl)
        if not m:
            raise bad("neither constants, a record nor a prototype `T name(T name, ...)`", decl)
        args = [] if m.group(3).strip() in ("", "void") else [declarator(a, decl) for a in m.group(3).split(",")]
        # (an array parameter `T name[]` is the pointer `T* name`)
        sigs[m.group(2)] = (ctype(m.group(1), decl), [ctype(t if array is None else t + "*", decl) for t, _, array in args])
        declared.append(m.group(2))
    return {n for n in declared if n in taken}


with open(HEADER) as _f:
    _TEXT = _f.read()
CONSTANTS, STRUCTS, _SIGS = parse_header(_TEXT)
# the extension header: prototypes added without touching the tables above (it declares no record and no constant)
with open(EXT_HEADER) as _f:
    _EXT_CONSTANTS, _EXT_STRUCTS, _EXT_SIGS = parse_header(_f.read(), base=_TEXT)
if _EXT_CONSTANTS or _EXT_STRUCTS:
    raise ValueError("iswm_hip_sep.h declares prototypes only, not %s" % sorted(set(_EXT_CONSTANTS) | set(_EXT_STRUCTS)))
# the distillation header, the same way; a name of either earlier header is refused
with open(KD_HEADER) as _f:
    _KD_CONSTANTS, _KD_STRUCTS, _KD_SIGS = parse_header(_f.read(), base=_TEXT)
if _KD_CONSTANTS or _KD_STRUCTS:
    raise ValueError("iswm_hip_kd.h declares prototypes only, not %s" % sorted(set(_KD_CONSTANTS) | set(_KD_STRUCTS)))
if set(_KD_SIGS) & set(_EXT_SIGS):
    raise ValueError("iswm_hip_kd.h declares %s again (iswm_hip_sep.h has it)" % sorted(set(_KD_SIGS) & set(_EXT_SIGS)))
# the distance-map and boundary-loss header, the same way; a name of any earlier header is refused
with open(BD_HEADER) as _f:
    _BD_CONSTANTS, _BD_STRUCTS, _BD_SIGS = parse_header(_f.read(), base=_TEXT)
if _BD_CONSTANTS or _BD_STRUCTS:
    raise ValueError("iswm_hip_bd.h declares prototypes only, not %s" % sorted(set(_BD_CONSTANTS) | set(_BD_STRUCTS)))
if set(_BD_SIGS) & (set(_EXT_SIGS) | set(_KD_SIGS)):
    raise ValueError("iswm_hip_bd.h declares %s again (an earlier extension header has it)" %
                     sorted(set(_BD_SIGS) & (set(_EXT_SIGS) | set(_KD_SIGS))))
# the boundary-metrics header, the same way; a name of any earlier header is refused
with open(BM_HEADER) as _f:
    _BM_CONSTANTS, _BM_STRUCTS, _BM_SIGS = parse_header(_f.read(), base=_TEXT)
if _BM_CONSTANTS or _BM_STRUCTS:
    raise ValueError("iswm_hip_bm.h declares prototypes only, not %s" % sorted(set(_BM_CONSTANTS) | set(_BM_STRUCTS)))
if set(_BM_SIGS) & (set(_EXT_SIGS) | set(_KD_SIGS) | set(_BD_SIGS)):
    raise ValueError("iswm_hip_bm.h declares %s again (an earlier extension header has it)" %
                     sorted(set(_BM_SIGS) & (set(_EXT_SIGS) | set(_KD_SIGS) | set(_BD_SIGS))))
# the CRF-refinement header, the same way; a name of any earlier header is refused
with open(CR_HEADER) as _f:
    _CR_CONSTANTS, _CR_STRUCTS, _CR_SIGS = parse_header(_f.read(), base=_TEXT)
if _CR_CONSTANTS or _CR_STRUCTS:
    raise ValueError("iswm_hip_cr.h declares prototypes only, not %s" % sorted(set(_CR_CONSTANTS) | set(_CR_STRUCTS)))
if set(_CR_SIGS) & (set(_EXT_SIGS) | set(_KD_SIGS) | set(_BD_SIGS) | set(_BM_SIGS)):
    raise ValueError("iswm_hip_cr.h declares %s again (an earlier extension header has it)" %
                     sorted(set(_CR_SIGS) & (set(_EXT_SIGS) | set(_KD_SIGS) | set(_BD_SIGS) | set(_BM_SIGS))))
ConvDesc, QConvDesc, PredictView = STRUCTS["iswm_conv_desc"], STRUCTS["iswm_qconv_desc"], STRUCTS["iswm_predict_view"]


class ScenePlan(STRUCTS["iswm_scene_plan"]):
    """iswm_scene_plan: nty x ntx windows of th x tw every (sy, sx) pixels over an H x W scene, the last window of an
    axis pulled back inside it; ramp = the blending ramp.  Windows are numbered k = ty * ntx + tx."""

    @property
    def ntiles(self):
        return self.nty * self.ntx

    def origins_y(self):
        return [min(k * self.sy, self.H - self.th) for k in range(self.nty)]

    def origins_x(self):
        return [min(k * self.sx, self.W - self.tw) for k in range(self.ntx)]

    def astuple(self):
        return tuple(getattr(self, n) for n, _ in self._fields_)


EXPORTS = tuple(_SIGS)
EXT_EXPORTS = tuple(_EXT_SIGS)
KD_EXPORTS = tuple(_KD_SIGS)
BD_EXPORTS = tuple(_BD_SIGS)
BM_EXPORTS = tuple(_BM_SIGS)
CR_EXPORTS = tuple(_CR_SIGS)
_lib = None


class IswmError(RuntimeError):
    pass


def load():
    """Load the library once; raise loudly when it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "libiswm_hip.so is not built (%s). Run `python -m iswm_amd.build` (hipcc, gfx950). "
            "iswm_amd has no CPU or torch-op fallback." % LIB_PATH)
    # torch first: its HIP runtime is then the one the library binds to.  Loaded the other way round, the process holds
    # two runtimes and the library's launches on torch's streams fail ("no ROCm-capable device is detected").
    import torch  # noqa: F401
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in (list(_SIGS.items()) + list(_EXT_SIGS.items()) + list(_KD_SIGS.items()) + list(_BD_SIGS.items()) +
                              list(_BM_SIGS.items()) + list(_CR_SIGS.items())):
        fn = getattr(lib, name)  # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def call(name, *args):
    """Call a status-returning entry point; non-zero status -> IswmError(message)."""
    lib = load()
    rc = getattr(lib, name)(*args)
    if rc != 0:
        msg = lib.iswm_last_error()
        raise IswmError("%s failed (%d): %s" % (name, rc, msg.decode() if msg else "?"))
