"""Reader of include/mjx355.h: the header is the only declaration of the C ABI, and the ctypes binding
(`abi.py`: constants and the two structs; `_lib.py`: every entry point's signature) is derived from it.

Not a C parser. It accepts exactly the forms the header uses — include guards, one-line integer
`#define`s, `enum { A = n, ... };`, `typedef struct S { scalars and fixed arrays } S;`, opaque
`typedef struct S S;` handles and prototypes over the types below — and raises `HeaderError` on
anything else, so a construct it does not understand fails at import instead of reaching ctypes'
`int` default. The library's stamp covers the header (`_srchash.py`), so a binding read from this
file cannot disagree with the library the loader accepts.
"""
from __future__ import annotations

import ctypes as C
import re
from typing import NamedTuple

from . import _srchash

SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "float": C.c_float, "double": C.c_double,
           "long long": C.c_longlong, "unsigned": C.c_uint, "uint64_t": C.c_uint64}
_POINTEES = set(SCALARS) | {"void", "char", "uint8_t", "uint32_t"}  # plus the header's own struct names

_FORM = re.compile(r"""\s*(?:
      extern\s+"C"\s*\{ | \}
    | enum\s*\{(?P<enum>[^{}]*)\}\s*;
    | typedef\s+struct\s+(?P<struct>\w+)\s*\{(?P<body>[^{}]*)\}\s*(?P=struct)\s*;
    | typedef\s+struct\s+(?P<opaque>\w+)\s+(?P=opaque)\s*;
    | (?P<ret>\w[\w\s]*?[\s*]+)(?P<fn>mjl_\w+)\s*\((?P<args>[^(){};]*)\)\s*;
    )""", re.X)
_DIRECTIVE = re.compile(r"#\s*(?:(?:ifndef|ifdef|include)\s+\S+|endif|define\s+\w+|define\s+(\w+)\s+(-?\d+))\s*")


class HeaderError(ValueError):
    pass


class Header(NamedTuple):
    defines: dict  # NAME -> int
    enums: dict    # NAME -> int, every enum's constants together
    structs: dict  # struct name -> [(field, scalar type, array dims)], None for an opaque handle
    protos: list   # [(return type, name, [argument types])], header order; "const" dropped, "T*" / "T**"


def _ctype(t: str, pointees) -> str:
    """A C type as written -> "T", "T*" or "T**" without qualifiers; an unknown T raises."""
    words = " ".join(w for w in t.replace("*", " ").split() if w != "const")
    if words not in (pointees if "*" in t else SCALARS):
        raise HeaderError(f"unknown type {t.strip()!r}")
    return words + "*" * t.count("*")


def parse(text: str) -> Header:
    h = Header({}, {}, {}, [])
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    code = []
    for line in text.splitlines():
        if line.lstrip().startswith("#"):
            m = _DIRECTIVE.fullmatch(line.strip())
            if not m:
                raise HeaderError(f"unsupported directive: {line.strip()}")
            if m.group(1):
                h.defines[m.group(1)] = int(m.group(2))
        else:
            code.append(line)
    text, pos = "\n".join(code), 0
    while text[pos:].strip():
        m = _FORM.match(text, pos)
        if not m:
            raise HeaderError(f"unsupported declaration: {' '.join(text[pos:].split())[:100]!r}")
        pos = m.end()
        if m.group("enum") is not None:
            for item in m.group("enum").split(","):
                c = re.fullmatch(r"\s*(\w+)\s*=\s*(-?\d+)\s*", item)
                if not c:
                    raise HeaderError(f"enum constant without a literal value: {item.strip()!r}")
                h.enums[c.group(1)] = int(c.group(2))
        elif m.group("struct"):
            h.structs[m.group("struct")] = fields = []
            for decl in filter(str.strip, m.group("body").split(";")):
                t, names = decl.split(None, 1)
                if t not in SCALARS:
                    raise HeaderError(f"unknown field type {t!r} in {m.group('struct')}")
                for d in names.split(","):
                    f = re.fullmatch(r"\s*(\w+)((?:\[\w+\])*)\s*", d)
                    if not f:
                        raise HeaderError(f"unsupported field {d.strip()!r} in {m.group('struct')}")
                    dims = re.findall(r"\w+", f.group(2))
                    if any(not b.isdigit() and b not in h.defines for b in dims):
                        raise HeaderError(f"array bound of {f.group(1)} is not a literal or a known #define")
                    fields.append((f.group(1), t, tuple(int(b) if b.isdigit() else h.defines[b] for b in dims)))
        elif m.group("opaque"):
            h.structs.setdefault(m.group("opaque"), None)
        elif m.group("fn"):
            pointees = _POINTEES | set(h.structs)
            ret = m.group("ret").strip()
            args = [] if m.group("args").strip() == "void" else m.group("args").split(",")
            named = [re.fullmatch(r"\s*(.*?[\s*])\w+\s*", a) for a in args]
            if not all(named):
                raise HeaderError(f"unsupported parameter list of {m.group('fn')}")
            h.protos.append(("void" if ret == "void" else _ctype(ret, pointees), m.group("fn"),
                             [_ctype(a.group(1), pointees) for a in named]))
    return h


with open(_srchash.HEADER) as _f:
    HEADER = parse(_f.read())
