"""bsmap_amd.methratio.Meth, the Python class over the bsx_meth C ABI: its two constructors give the same handle, n_chr / chr_name know the FASTA's names,
add() is add_arrays() on the same reads and nothing on no reads, and a closed object raises in Python and never enters the library.  The worked example
of test_methratio_readlevel_cpu.py on two sequences: a few dozen letters and a handful of reads."""
import ctypes as C

import numpy as np
import pytest

import meth_util as U
from bsmap_amd import _check
from bsmap_amd.methratio import Meth
from test_methratio_readlevel_cpu import ALNS as EX_ALNS, CG_C, REF as EX_REF

pytestmark = pytest.mark.gpu
NAMES, REFS = ["one", "two"], [EX_REF, EX_REF[4:]]     # two starts at the second CpG of one
ALNS = EX_ALNS + [(1, 0, st, 0, -1, s[4:]) for _, _, st, _, _, s in EX_ALNS[:5]]


@pytest.fixture(scope="module")
def fasta(tmp_path_factory):
    return U.write_fasta(tmp_path_factory.mktemp("handle") / "two.fa", NAMES, REFS)


def everything(m):
    """the table rows, the PDR rows and the valid mappings of a handle with both sequences"""
    return U.table_rows(m, 2), U.pdr_rows(m, 2), m.valid_mappings()


def filled(m):
    m.set_pdr(4)
    m.add(ALNS, 0)
    return m


def test_both_constructors_give_the_same_handle(fasta):
    with Meth.from_fasta(fasta) as a, Meth.from_lengths([len(r) for r in REFS]) as b:
        assert (a.n_chr, b.n_chr) == (2, 2)
        assert [a.chr_name(c) for c in range(2)] == NAMES and [b.chr_name(c) for c in range(2)] == ["", ""]
        for c, (ref, as_given) in enumerate(zip(REFS, (str, lambda s: np.frombuffer(s.encode(), np.uint8)))):
            b.set_reference(c, as_given(ref))
        b.set_reference(1, REFS[1].encode())
        got = everything(filled(a))
        assert got == everything(filled(b))
        rows, pdr, nmap = got
        assert nmap == len(ALNS) and len(rows[0]) > 20 and {c for c, *_ in rows[0]} == {0, 1}
        assert [i for c, i, _, _ in pdr if c == 0 and EX_REF[i] == "C"] == list(CG_C) and any(c == 1 for c, *_ in pdr)
    with Meth.from_fasta(fasta, chroms=["two"]) as only:
        assert only.n_chr == 1 and only.chr_name(0) == "two"


def test_add_is_add_arrays_and_no_reads_are_no_call(fasta):
    with Meth.from_fasta(fasta) as a, Meth.from_fasta(fasta) as b, Meth.from_fasta(fasta) as none:
        none.set_pdr(4)
        none.add([], 0)
        assert everything(none) == (([], 0, 0), [], 0)
        off = np.cumsum([0] + [len(x[5]) for x in ALNS])                       # int64: add_arrays converts what has another type ...
        seq = np.frombuffer("".join(x[5] for x in ALNS).encode(), np.uint8)    # ... and passes on what has the right one
        b.set_pdr(4)
        b.add_arrays(len(ALNS), *[[x[k] for x in ALNS] for k in range(5)], seq, off, 0)
        assert everything(filled(a)) == everything(b) and b.valid_mappings() == len(ALNS)


def test_optional_out_pointers_may_be_null(fasta, tmp_path):
    """the wrapper always asks for the counts; the ABI lets a caller leave them out"""
    nr = C.c_uint32()
    with Meth.from_fasta(fasta) as m:
        m.set_pdr(4)
        path = tmp_path / "in.bsp"
        path.write_text("".join("r%d\t%s\t%s\tUM\t%s\t%d\t%s\t0\n" % (k, s, "I" * len(s), NAMES[c], pos + 1, ("++", "-+", "+-", "--")[st], )
                                for k, (c, pos, st, _, _, s) in enumerate(ALNS)))
        _check(m.L.bsx_meth_add_file(m.h, str(path).encode(), 0, None, 0, 0, 0, None))
        assert m.valid_mappings() == len(ALNS)
        _check(m.L.bsx_meth_report_chr(m.h, 0, 1, 1, C.byref(nr), None, None))
        assert nr.value == len(m.report(0)[0]) == 15   # the ten C and G of the five CpGs, the Cs at 22, 26, 33 and the Gs at 28, 35
        _check(m.L.bsx_meth_write_pdr(m.h, str(tmp_path / "pdr").encode(), 1, None))
        _check(m.L.bsx_meth_write_table(m.h, str(tmp_path / "t.txt").encode(), 0, None, None, 1, 1, None, None))
        assert m.write_table(tmp_path / "t2.txt") == (sum(m.report(c)[3] for c in range(2)), sum(m.report(c)[4] for c in range(2)))
        assert U.read_text(tmp_path / "t.txt") == U.read_text(tmp_path / "t2.txt") and U.read_text(tmp_path / "pdr").count("\n") > 5


def test_close(fasta):
    m = Meth.from_fasta(fasta)
    m.add(ALNS, 0)
    assert m.valid_mappings() == len(ALNS)
    m.close()
    assert m.h is None
    m.close()                                            # twice: harmless
    for call in (m.valid_mappings, lambda: m.add(ALNS, 0), lambda: m.report(0), lambda: m.n_chr, lambda: m.write_table("never.txt")):
        with pytest.raises(ValueError, match="closed"):
            call()
    with pytest.raises(ValueError, match="closed"):
        with m:
            pass


def test_with_closes_on_an_exception(fasta):
    with pytest.raises(KeyError):
        with Meth.from_fasta(fasta) as m:
            assert m.h is not None
            raise KeyError("inside the block")
    assert m.h is None
    with pytest.raises(ValueError, match="closed"):
        m.combine_cpg()
