"""The ctypes prototypes of bsmap_amd.methratio against include/bsx.h, and the life cycle of its Meth class, both without a device: every bsx_meth_*
declaration of the header is in methratio.PROTOTYPES with the same number of parameters, the same width of every scalar one and the same return type,
and a Meth that was never opened or has been closed raises from every public method before it reaches the library."""
import ctypes as C
import inspect
import os
import re

import pytest

import bsmap_amd as B
from bsmap_amd import methratio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALARS = {"uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "int": C.c_int32}


def declarations():
    """{name: (return type, [parameter, ..])} of the header's bsx_meth_* functions as C text, comments taken out"""
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "bsx.h")).read(), flags=re.S)
    out = {}
    for ret, name, params in re.findall(r"^((?:const\s+)?\w+\s*\*?)\s*(bsx_meth_\w+)\s*\(([^)]*)\)\s*;", hdr, flags=re.M):
        params = [" ".join(p.split()) for p in params.split(",")]
        out[name] = (" ".join(ret.split()), [] if params == ["void"] else params)
    return out


DECL = declarations()


def is_pointer(t):
    return t in (C.c_void_p, C.c_char_p) or (isinstance(t, type) and issubclass(t, C._Pointer))


def test_the_table_holds_every_export_and_nothing_else():
    exports = {n for n in B.EXPORTS if n.startswith("bsx_meth_")}
    assert set(methratio.PROTOTYPES) == exports == set(DECL) and len(exports) >= 39


def test_the_parser_reads_what_it_should():
    """declarations with a comment inside the parameter list, over two lines, without parameters and with each kind of return type"""
    assert DECL["bsx_meth_set_reference"] == ("int", ["bsx_meth *m", "uint32_t chr", "const char *upper_seq"])
    assert DECL["bsx_meth_mbias_fetch"][1] == ["bsx_meth *m", "uint64_t *cells", "uint64_t *overflow_calls"]
    assert DECL["bsx_meth_read_stats_fetch"][1] == ["bsx_meth *m", "uint64_t *cg", "uint64_t *ch", "uint64_t *totals"]
    assert len(DECL["bsx_meth_add"][1]) == 10 and len(DECL["bsx_meth_write_table"][1]) == 9
    assert DECL["bsx_meth_region_tile"] == ("uint32_t", []) and DECL["bsx_meth_destroy"][0] == "void"
    assert DECL["bsx_meth_chr_name"][0] == "const char *" and DECL["bsx_meth_n_chr"] == ("uint32_t", ["const bsx_meth *m"])


@pytest.mark.parametrize("name", sorted(DECL))
def test_prototype_agrees_with_the_header(name):
    ret, params = DECL[name]
    restype, argtypes = methratio.PROTOTYPES[name]
    assert len(argtypes) == len(params), params
    for p, t in zip(params, argtypes):
        if "*" in p:
            assert is_pointer(t), p
        else:
            assert t is SCALARS[p.rsplit(" ", 1)[0]], p
    if ret == "void":
        assert restype is None
    elif "*" in ret:
        assert ret == "const char *" and restype in (C.c_char_p, C.c_void_p)
    else:
        assert restype is SCALARS[ret]


def test_bind_applies_the_table():
    B.build()
    L = methratio._bind()
    for name, (restype, argtypes) in methratio.PROTOTYPES.items():
        f = getattr(L, name)
        assert f.restype is restype and list(f.argtypes) == argtypes, name


class Lib:
    """stands for the library: counts the destroy calls, and any other use is the failure under test"""
    destroyed = 0

    def bsx_meth_destroy(self, h):
        self.destroyed += 1

    def __getattr__(self, name):
        raise AssertionError("the library was reached: " + name)


def never_opened():
    return methratio.Meth.__new__(methratio.Meth)


def closed():
    m = never_opened()
    m.L, m.h = Lib(), C.c_void_p(1)
    m.close()
    assert m.h is None and m.L.destroyed == 1
    return m


@pytest.mark.parametrize("make", [never_opened, closed])
def test_a_closed_meth_raises_before_the_library(make):
    m = make()
    public = [n for n in vars(methratio.Meth) if not n.startswith("_") and n not in ("L", "h", "from_fasta", "from_lengths", "close")]
    assert len(public) >= 30 and {"n_chr", "add", "add_arrays", "report", "bins", "write_regions", "set_reference"} <= set(public)
    for name in public:
        member = inspect.getattr_static(methratio.Meth, name)
        with pytest.raises(ValueError, match="closed"):
            if isinstance(member, property):
                getattr(m, name)
            else:
                args = ["x.txt" if "path" in p else 0 for p, v in list(inspect.signature(member).parameters.items())[1:] if v.default is v.empty]
                getattr(m, name)(*args)
    with pytest.raises(ValueError, match="closed"):
        with m:
            pass
    m.close()   # again: nothing happens
    assert m.h is None and (m.L is None or m.L.destroyed == 1)
