"""Reader of include/vtmc.h, the project's contract, and of the headers of its optional layers (the rows of build.ABI_LAYERS): their constants,
structs and prototypes as Python values, so that the ctypes binding (_lib.py) is the headers' by construction.  It knows the forms the header uses and nothing else, and it never skips: whatever it cannot
read raises HeaderError with the line, so a new form is taught to the reader in the pull request that first writes it."""
import collections
import ctypes
import os
import re

import numpy as np

from . import build as _build

PATH = os.path.join(_build.INCLUDE, _build.ABI_LAYERS[0][1])   # include/vtmc.h

SCALARS = {"float": (ctypes.c_float, "<f4"), "int32_t": (ctypes.c_int32, "<i4"), "uint32_t": (ctypes.c_uint32, "<u4"),
           "int64_t": (ctypes.c_int64, "<i8"), "uint64_t": (ctypes.c_uint64, "<u8"), "uint8_t": (ctypes.c_uint8, "u1")}
RETURNS = {"int32_t": ctypes.c_int32, "const char *": ctypes.c_char_p, "void": None}

# name; return type and parameter declarations as written (one space between words); what ctypes is given
Prototype = collections.namedtuple("Prototype", "name ret params restype argtypes")
Field = collections.namedtuple("Field", "name ctype format shape")   # format / shape: numpy's; None / () for a pointer


class HeaderError(ValueError):
    pass


class Header:
    def __init__(self, path=PATH, base=None):
        """base: the Header of the file this one includes; its types may be pointed to here."""
        self.path = path
        with open(path) as f:
            self.text = re.sub(r"/\*.*?\*/", lambda m: re.sub(r"[^\n]", " ", m.group()), f.read(), flags=re.S)   # comments blanked, lines kept
        self.constants, self.structs, self.prototypes = {}, {}, {}
        self.pointees = set(SCALARS) | {"void", "char", "uint8_t"}   # what a pointer may point to; structs and opaque types join below
        if base is not None:
            self.pointees |= base.pointees
        for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(VTMC_\w+)(.*)$", self.text, flags=re.M):
            if not (m.group(1).endswith("_H") and not m.group(2).strip()):   # the include guard
                self.constants[m.group(1)] = self._value(m.group(2), m.start())
        for m in re.finditer(r"\btypedef\s+struct\b", self.text):
            self._struct(m.start())
        for m in re.finditer(r"\b(vtmc_\w+)\s*\(", self.text):
            self._prototype(m)

    def _fail(self, pos, what):
        raise HeaderError("%s:%d: %s" % (self.path, self.text.count("\n", 0, pos) + 1, what))

    def _value(self, text, pos):
        v = text.strip()
        if v.startswith("(") and v.endswith(")"):
            v = v[1:-1].strip()
        if re.fullmatch(r"-?\d+[uU]?", v):
            return int(v.rstrip("uU"))
        if re.fullmatch(r"0[xX][0-9a-fA-F]+[uU]?", v):
            return int(v.rstrip("uU"), 16)
        m = re.fullmatch(r"(\d+)\s*<<\s*(\d+)", v)
        if m:
            return int(m.group(1)) << int(m.group(2))
        if re.fullmatch(r"-?(\d+\.\d*|\.\d+)([eE][-+]?\d+)?[fF]?", v):
            return float(v.rstrip("fF"))
        self._fail(pos, "cannot evaluate #define value %r" % text.strip())

    def _struct(self, pos):
        m = re.compile(r"typedef\s+struct\s+(\w+)\s+(\w+)\s*;").match(self.text, pos)
        if m and m.group(1) == m.group(2):   # an opaque handle: typedef struct vtmc_ctx vtmc_ctx;
            self.pointees.add(m.group(1))
            return
        m = re.compile(r"typedef\s+struct\s+(vtmc_\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;").match(self.text, pos)
        if not m or m.group(1) != m.group(3) or m.group(1) in self.structs:
            self._fail(pos, "cannot parse this typedef struct")
        fields, at = [], m.start(2)
        for decl in m.group(2).split(";")[:-1]:
            d = re.fullmatch(r"\s*(?:const\s+)?(\w+)\b(.*)", decl, flags=re.S)
            if not d:
                self._fail(at, "cannot parse field declaration %r" % decl.strip())
            for one in d.group(2).split(","):
                f = re.fullmatch(r"\s*(\*?)\s*(\w+)\s*(?:\[(\d+)\])?\s*", one)
                if not f or d.group(1) not in (self.pointees if f.group(1) else SCALARS) or (f.group(1) and f.group(3)):
                    self._fail(at + len(decl) - len(decl.lstrip()), "field %r: a form or base type this reader does not know" % " ".join(decl.split()))
                if f.group(1):
                    fields.append(Field(f.group(2), ctypes.c_void_p, None, ()))
                else:
                    ctype, fmt = SCALARS[d.group(1)]
                    n = int(f.group(3)) if f.group(3) else 0
                    fields.append(Field(f.group(2), ctype * n if n else ctype, fmt, (n,) if n else ()))
            at += len(decl) + 1
        if m.group(2).split(";")[-1].strip() or not fields:
            self._fail(pos, "cannot parse this typedef struct")
        self.structs[m.group(1)] = fields
        self.pointees.add(m.group(1))

    def _prototype(self, m):
        name, at = m.group(1), m.start()
        ret = self.text[max(self.text.rfind(c, 0, at) for c in ";}{") + 1:at].split("\n")   # before the name, back to the last declaration or the extern "C" {,
        ret = re.sub(r"\s*\*\s*", " *", " ".join(" ".join(l for l in ret if not l.lstrip().startswith("#")).split()))   # less preprocessor lines
        tail = re.compile(r"\(([^;{}()]*)\)\s*;").match(self.text, m.end() - 1)
        if ret not in RETURNS or not tail or name in self.prototypes:
            self._fail(at, "%s( is not a prototype this reader knows (return type %r)" % (name, ret))
        args = " ".join(tail.group(1).split())
        params = [] if args in ("", "void") else [a.strip() for a in args.split(",")]
        self.prototypes[name] = Prototype(name, ret, params, RETURNS[ret], [self._parameter(p, at, name) for p in params])

    def _parameter(self, decl, pos, name):
        d = re.fullmatch(r"(?:const )?(\w+) ?((?:\* ?(?:const ?)?)*)(\w+)? ?(\[\w*\])?", decl)
        if d and (d.group(2) or d.group(4)):   # a pointer, or an array parameter, which is one
            if d.group(1) == "char" and d.group(2).count("*") == 1 and not d.group(4):
                return ctypes.c_char_p
            if d.group(1) in self.pointees:
                return ctypes.c_void_p   # accepts byref(...), array.ctypes.data_as(c_void_p) and a bare address alike
        elif d and d.group(1) in SCALARS and d.group(3):
            return SCALARS[d.group(1)][0]
        self._fail(pos, "%s: parameter %r: a form or base type this reader does not know" % (name, decl))

    def structure(self, c_name, py_name, doc=None):
        """A ctypes.Structure class of a struct of the header: natural alignment, fields in the header's order."""
        return type(py_name, (ctypes.Structure,), {"_fields_": [(f.name, f.ctype) for f in self.structs[c_name]], "__doc__": doc})

    def dtype(self, c_name, names=None):
        """The little-endian numpy dtype of a struct without pointers, offsets and size as the C compiler's; names: other field names,
        by position."""
        fields, layout = self.structs[c_name], self.structure(c_name, c_name)
        if any(f.format is None for f in fields):
            raise HeaderError("%s holds a pointer: it has no numpy dtype" % c_name)
        return np.dtype({"names": list(names or [f.name for f in fields]), "formats": [(f.format, f.shape) for f in fields],
                         "offsets": [getattr(layout, f.name).offset for f in fields], "itemsize": ctypes.sizeof(layout)})


def read_layers(rows=_build.ABI_LAYERS, include=_build.INCLUDE):
    """name -> Header of every row, in the table's order; a row's base is an earlier row's Header."""
    layers = {}
    for name, file, base, _doc in rows:
        if base is not None and base not in layers:
            raise HeaderError("ABI layer %r: its base %r is not an earlier row of the table" % (name, base))
        layers[name] = Header(os.path.join(include, file), base=layers.get(base))
    return layers


LAYERS = read_layers()
HEADER = LAYERS["core"]
