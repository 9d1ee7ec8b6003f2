"""The contract every ABI layer keeps, written once: build.ABI_LAYERS registers a layer (name, header, the row it includes, the document
with its [DllImport] stubs), and each test here runs for every row it applies to -- the optional layers, or all rows where the core
(include/vtmc.h) keeps the same rule.  What is a layer's own (its constants' values, the prototype order and argtypes, struct offsets,
the rule words of its header and document, what it refuses) stays in that layer's test file.  CPU only."""
import ctypes
import itertools
import os
import re
import shutil
import subprocess

import pytest

import volumetricterrain_amd as vt
from volumetricterrain_amd import _header, _lib, build
import test_dllimport_stubs as stubs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = {name: (file, base, doc) for name, file, base, doc in build.ABI_LAYERS}
ALL = list(ROWS)
OPTIONAL = [name for name in ALL if ROWS[name][1] is not None]


def code_of(name):
    """The header's text without its comments."""
    return re.sub(r"/\*.*?\*/", "", open(_header.LAYERS[name].path).read(), flags=re.S)


def test_the_table_is_what_the_package_reads():
    assert ALL == list(_header.LAYERS) == list(_lib.LAYER_SYMBOLS) and ALL[0] == "core" and set(ALL) >= {"nav", "navfield", "naverode", "navsight"}
    assert _header.HEADER is _header.LAYERS["core"] and _lib.SYMBOLS is _lib.LAYER_SYMBOLS["core"]
    for name in ALL:
        assert os.path.samefile(_header.LAYERS[name].path, os.path.join(ROOT, "include", ROWS[name][0])), name
        assert _header.LAYERS[name].path in [os.path.join(build.CSRC, h) for h in build.HEADERS], name   # is_stale looks at it
    with pytest.raises(_header.HeaderError, match="'navfield'.*not an earlier row"):
        _header.read_layers([row for row in build.ABI_LAYERS if row[0] != "nav"])


@pytest.mark.parametrize("name", ALL)
def test_declared_functions_are_the_readers(name):
    found = sorted(set(re.findall(r"\b(vtmc_[a-z_0-9]+)\s*\(", code_of(name))))   # as test_abi_symbols.py finds them
    assert found == sorted(_header.LAYERS[name].prototypes) == sorted(_lib.LAYER_SYMBOLS[name])


@pytest.mark.parametrize("name", OPTIONAL)
def test_every_prototype_returns_a_status(name):
    for p in _header.LAYERS[name].prototypes.values():
        assert p.ret == "int32_t" and p.restype is ctypes.c_int32, p.name


def test_no_symbol_is_declared_by_two_headers():
    for a, b in itertools.combinations(ALL, 2):
        assert not set(_lib.LAYER_SYMBOLS[a]) & set(_lib.LAYER_SYMBOLS[b]), (a, b)


@pytest.mark.parametrize("name", OPTIONAL)
def test_header_includes_its_base(name):
    assert '#include "%s"' % ROWS[ROWS[name][1]][0] in code_of(name)


def checks_of(name):
    """C expressions, true when the compiler agrees with the reader: the size of every struct and the value of every integer constant of
    the layer's header and of the headers it includes."""
    out = []
    while name is not None:
        H = _header.LAYERS[name]
        out += ["sizeof(%s) == %d" % (s, ctypes.sizeof(H.structure(s, s))) for s in H.structs]
        out += ["%s == %d%s" % (c, v, "u" if v > 0x7fffffff else "") for c, v in H.constants.items() if isinstance(v, int)]
        name = ROWS[name][1]
    return out


@pytest.mark.parametrize("name", ALL)
def test_header_compiles_alone_as_pedantic_c_and_cpp(tmp_path, name):
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.skip("no host C compiler")
    checks = checks_of(name)
    assert len(checks) >= 3, checks
    # -fsyntax-only evaluates no return expression, so every check stands a second time as an array size the compiler has to accept
    src = tmp_path / (name + ".c")
    src.write_text('#include "%s"\nint main(void) { return %s ? 0 : 1; }\n' % (ROWS[name][0], "\n    && ".join(checks)) +
                   "".join("typedef char check_%d[(%s) ? 1 : -1];\n" % (i, c) for i, c in enumerate(checks)))
    strict = ["-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-fsyntax-only"]
    for cmd in ([cc, "-std=c99"] + strict + [str(src)], ["g++", "-std=c++11"] + strict + ["-x", "c++", str(src)]):
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("name", ALL)
def test_library_exports_every_symbol(name):
    L = vt.load()
    for symbol in _lib.LAYER_SYMBOLS[name]:
        assert hasattr(L, symbol), symbol


@pytest.mark.parametrize("name", OPTIONAL)
def test_dllimport_stubs_are_the_headers(name):
    """The stubs of the layer's document against its header, by the rules test_dllimport_stubs.py applies to INTEGRATION.md's against
    include/vtmc.h -- and exactly the layer's symbols, none missing."""
    found = stubs.cs_stubs(os.path.join(ROOT, ROWS[name][2]))
    assert sorted(found) == sorted(_lib.LAYER_SYMBOLS[name])
    for symbol, (ret, params) in found.items():
        p = _header.LAYERS[name].prototypes[symbol]
        assert ret == "int" and p.ret == "int32_t" and len(params) == len(p.params), symbol
        for cs, c in zip(params, p.params):
            assert stubs.matches(cs, c), (symbol, cs, c)


@pytest.mark.parametrize("name", OPTIONAL)
def test_document_is_linked_from_the_readme_and_the_integration_guide(name):
    for linking in ("README.md", "INTEGRATION.md"):
        assert ROWS[name][2] in open(os.path.join(ROOT, linking)).read(), linking
