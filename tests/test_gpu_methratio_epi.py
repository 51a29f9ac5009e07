"""Epiallele patterns of bsmap_amd.methratio on the GPU (the CpG index, k_meth_epi, bsx_meth_set_epi / _n_cpg / _epi_report_chr / _epi_fetch_rows /
_write_epi; --epi) against the pure-Python model of epi_model.py, which never looks at the library's output.  Every expectation is formed from the model
before the library is touched."""
import ctypes as C
import os

import numpy as np
import pytest

from bsmap_amd import _check
from bsmap_amd.methratio import Meth

import epi_model as E
import meth_util as U
import readlevel_model as RL
from test_methratio_epi_cpu import CELLS_N0, CELLS_N3, HEADER, TEXT_N0, TEXT_N3, pat
from test_methratio_readlevel_cpu import ALNS as EX_ALNS, REF as EX_REF

pytestmark = pytest.mark.gpu
STRANDS = RL.STRANDS
BSX_ERR_ARG, BSX_ERR_STATE = -1, -5


def handle(fa, epi=True, stats=False, min_cpg=0, **kw):
    """the epiallele tally on (epi=False: off), histogram and PDR off unless asked for; kw: rm_dup, snp, mbias, trim, nonconv"""
    return U.open_meth(fa, epi=epi, stats=stats, min_cpg=min_cpg, **kw)


def n_cpg(h, n_chr):
    return [h.n_cpg(c) for c in range(n_chr)]


def written_epi(h, path, min_reads=1):
    n = h.write_epi(path, min_reads)
    return U.read_text(path), n


def make_read(rng, ref, pos, L, st, keep=None, x_rate=0.03):
    """the reference's letters under [pos, pos + L) as a read of strand code st shows them: the strand's own cytosines methylated with probability `keep`
    (default: one of 0, 1, 1/2 per read), another letter or N (an X at a CpG) with probability x_rate"""
    match, convert = ("C", "T") if st % 2 == 0 else ("G", "A")
    keep = (0.0, 1.0, 0.5)[int(rng.integers(0, 3))] if keep is None else keep
    out = []
    for x in ref[pos:pos + L]:
        if x == match:
            x = ("ANG" if match == "C" else "TNC")[int(rng.integers(0, 3))] if rng.random() < x_rate else match if rng.random() < keep else convert
        out.append(x)
    return "".join(out)


# ---- the worked example ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def example_fa(tmp_path_factory):
    return U.write_fasta(tmp_path_factory.mktemp("epi_example") / "one.fa", ["one"], [EX_REF])


@pytest.mark.parametrize("nonconv", [3, 0])
def test_worked_example(example_fa, tmp_path, nonconv):
    cells, text = (CELLS_N3, TEXT_N3) if nonconv else (CELLS_N0, TEXT_N0)
    rows = [(0, (2, 6, 10, 14), cells[0][0]), (0, (6, 10, 14, 18), cells[0][1])]
    with handle(example_fa, nonconv=nonconv) as h:
        assert n_cpg(h, 1) == [5]
        h.add(EX_ALNS, 0)
        assert U.epi_rows(h, 1) == rows
        assert U.epi_rows(h, 1, 6) == (rows if nonconv == 0 else []) and U.epi_rows(h, 1, 7) == []
        got, n = written_epi(h, tmp_path / "epi.txt")
        assert E.same_text(got, text) and n == 2, got
        assert [line.split("\t")[:7] + line.split("\t")[10:] for line in got.split("\n")] == [line.split("\t")[:7] + line.split("\t")[10:] for line in text.split("\n")]
        got, n = written_epi(h, tmp_path / "epi6.txt", 6)
        assert (E.same_text(got, text) and n == 2) if nonconv == 0 else (got == HEADER and n == 0)
        assert h.valid_mappings() == (7 if nonconv == 0 else 6)


# ---- step borders and directory borders --------------------------------------------------------------------------------------------------
class Borders:
    """Five chromosomes; none has a multiple of 64 letters, so the 64-letter blocks of the rank directory cut through them and through the reads.
      b0      191 letters of A/T with CG at 20, 30, 40, 50, 63 (its C is letter 63 of directory block 0, its G the first letter of block 1), 100, 120 and 189
              (its G is the chromosome's last letter)
      b1      130 letters, begins at letter 191 of the text; CG at 5, 15, 25, 35, 64 (letter 255 of the text: the last of block 3), 70, 80; ends in C ...
      b2      77 letters: ... and b2 begins with G: no CpG across the cut; CG at 10, 20, 30, 40, 50
      sparse  A/T with six planted groups of four CpGs, 300 letters apart: group (b, a) with b in (64, 128) and a in (1, 2, 3) has, counted from the group's
              read start, a call positions in front of letter b (b - 2a, .., b - 2) and 4 - a behind it (b, b + 2, ..); '+' reads start at the group's start,
              '-' reads one letter further, so that the G of each CpG is the same letter of the read.  Behind them a stretch with a CG every 7 to 23 letters.
      dense   "CG" x 150, then A/T: a 200-letter read holds 100 CpGs
    Reads: the whole of b0, b1, b2 and reads at their ends on all four strand codes; per group 200-letter reads on all four codes; reads of 63, 64, 65, 127,
    128, 129 and 200 letters over the dense and the sparse stretch at several starts on all four codes.  trim_fillin is 0 and every insert is 0: the window
    is the read."""
    LENGTHS = (63, 64, 65, 127, 128, 129, 200)

    def __init__(self):
        rng = np.random.default_rng(31)
        at = lambda n: rng.choice(list("AT"), n).tolist()
        def planted(n, where):
            s = at(n)
            for p in where:
                s[p:p + 2] = list("CG")
            return s
        b0 = planted(191, (20, 30, 40, 50, 63, 100, 120, 189))
        b1 = planted(130, (5, 15, 25, 35, 64, 70, 80)); b1[-1] = "C"
        b2 = planted(77, (10, 20, 30, 40, 50)); b2[0] = "G"
        self.groups = {}
        sparse = at(2901)
        for gi, (b, a) in enumerate((b, a) for b in (64, 128) for a in (1, 2, 3)):
            start = 10 + 300 * gi
            letters = [b - 2 * (a - i) for i in range(a)] + [b + 2 * i for i in range(4 - a)]
            for k in letters:
                sparse[start + k:start + k + 2] = list("CG")
            self.groups[(b, a)] = (start, letters)
        p = 1850
        while p < 2880:
            sparse[p:p + 2] = list("CG")
            p += int(rng.integers(7, 24))
        dense = list("CG" * 150) + at(103)
        self.names = ["b0", "b1", "b2", "sparse", "dense"]
        self.refs = ["".join(x) for x in (b0, b1, b2, sparse, dense)]
        assert all(len(r) % 64 for r in self.refs) and self.refs[1][-1] == "C" and self.refs[2][0] == "G"
        alns = []
        for c in range(3):
            n = len(self.refs[c])
            for st in range(4):
                for pos, L in ((0, n), (0, 64), (n - 64, 64), (n - 65, 65), (1, n - 1), (0, n - 1), (3, 70)):
                    alns.append((c, pos, st, 0, -1, make_read(rng, self.refs[c], pos, L, st, x_rate=0.0)))
                    alns.append((c, pos, st, 0, -1, make_read(rng, self.refs[c], pos, L, st)))
        self.directed = {}
        for key, (start, letters) in self.groups.items():
            for st in range(4):
                for rep in range(3):
                    aln = (3, start + (st & 1), st, 0, -1, make_read(rng, self.refs[3], start + (st & 1), 200, st, keep=0.5, x_rate=0.0))
                    self.directed.setdefault(key, []).append(aln)
                    alns.append(aln)
        for c, lo, hi in ((3, 1840, 2901), (4, 0, 403)):
            for L in self.LENGTHS:
                for st in range(4):
                    for pos in (lo, lo + 1, lo + 2, hi - L) + tuple(rng.integers(lo, hi - L + 1, 3).tolist()):
                        alns.append((c, pos, st, 0, -1, make_read(rng, self.refs[c], pos, L, st)))
        self.alns = [alns[i] for i in rng.permutation(len(alns)).tolist()]
        self.cells = E.epi_cells(self.refs, self.alns, 0)


@pytest.fixture(scope="module")
def borders(tmp_path_factory):
    b = Borders()
    b.fa = U.write_fasta(tmp_path_factory.mktemp("epi_borders") / "borders.fa", b.names, b.refs)
    return b


def test_border_set_covers_what_it_claims(borders):
    """the model's side only, no library call: the conditions without which the tests below would pass vacuously"""
    sites = E.cpgs(borders.refs)
    assert sites[0] == [20, 30, 40, 50, 63, 100, 120, 189] and sites[1] == [5, 15, 25, 35, 64, 70, 80] and sites[2] == [10, 20, 30, 40, 50]
    assert (191 + 64) % 64 == 63 and len(sites[4]) == 150
    for (b, a), alns in borders.directed.items():
        start, letters = borders.groups[(b, a)]
        assert sum(1 for k in letters if k < b) == a and len(letters) == 4 and [p for p in sites[3] if start <= p < start + 200] == [start + k for k in letters]
        o = sites[3].index(start + letters[0])
        for st in range(4):   # every strand code alone fills the group's one window, and the reads' call positions are the planned letters
            mine = [x for x in alns if x[2] == st]
            cells = E.epi_cells(borders.refs, mine, 0)[3]
            assert list(cells) == [o] and sum(cells[o]) == 3
            assert all([sites[3][oo] + (st & 1) - x[1] for oo, _ in states] == letters for x, states in zip(mine, E.states_of(borders.refs, mine, 0)))
    rows = E.epi_rows(borders.cells, borders.refs)
    assert {c for c, _, _ in rows} == {0, 1, 2, 3, 4}
    assert sum(1 for c, _, _ in rows if c == 4) == 147 and (0, (50, 63, 100, 120), borders.cells[0][3]) in rows and (0, (63, 100, 120, 189), borders.cells[0][4]) in rows
    long_ones = [st for a, st in zip(borders.alns, E.states_of(borders.refs, borders.alns, 0)) if st and len(st) > 64]
    assert len(long_ones) >= 8 and any(len(st) == 100 for st in long_ones)
    for L in Borders.LENGTHS:
        assert sum(1 for a in borders.alns if len(a[5]) == L and a[0] >= 3) >= 50


def test_n_cpg_and_borders(borders, tmp_path):
    with handle(borders.fa) as h:
        assert n_cpg(h, 5) == [len(x) for x in E.cpgs(borders.refs)]
        assert U.epi_rows(h, 5) == []
        h.add(borders.alns, 0)
        assert U.epi_rows(h, 5) == E.epi_rows(borders.cells, borders.refs)
        assert U.epi_rows(h, 5, 4) == E.epi_rows(borders.cells, borders.refs, 4) != []
        got, n = written_epi(h, tmp_path / "e.txt", 2)
        want = E.epi_text(borders.names, borders.refs, borders.cells, 2)
        assert E.same_text(got, want) and n == want.count("\n") - 1 > 100


@pytest.mark.parametrize("st", range(4))
def test_step_borders_per_strand(borders, st):
    """the reads of one strand code alone, one add: the planted windows across letters 63|64 and 127|128 and the long reads over the dense stretch"""
    mine = [a for a in borders.alns if a[2] == st and a[0] >= 3]
    want = E.epi_rows(E.epi_cells(borders.refs, mine, 0), borders.refs)
    assert len(want) > 150
    with handle(borders.fa) as h:
        h.add(mine, 0)
        assert U.epi_rows(h, 5) == want


# ---- model parity ------------------------------------------------------------------------------------------------------------------------------
class Parity:
    """Three chromosomes of 3 001, 2 050 and 1 777 random letters, each with a planted CpG island (one CG in three words of an A/C/G/T/CG mix) of 400 letters.
    About 2 000 random reads of 20 to 200 letters on all four strand codes, a third of them over an island, with inserts on both sides of the fill-in trim, cuts,
    reads that reach past the chromosome's end, and repeated fragment ends for -r; one read in eight is a non-converted one."""
    LENGTHS = (20, 50, 63, 64, 65, 100, 128, 129, 150, 200)

    def __init__(self):
        rng = np.random.default_rng(47)
        self.names, self.refs, self.island = ["p1", "p0", "p2"], [], []
        for n, isl in ((3001, 700), (2050, 1500), (1777, 60)):
            s = rng.choice(list("ACGT"), n).tolist()
            words = rng.choice(["CG", "A", "T", "C", "G", "CG", "TA"], 400).tolist()
            s[isl:isl + 400] = list("".join(words))[:400]
            s[5:9] = list("CNGC")
            self.refs.append("".join(s))
            self.island.append(isl)
        alns = []
        for k in range(2000):
            c = int(rng.integers(0, 3))
            L = int(rng.choice(self.LENGTHS))
            n = len(self.refs[c])
            pos = int(rng.integers(self.island[c] - 50, self.island[c] + 350)) if k % 3 == 0 else int(rng.integers(0, n - L + 2)) if k % 50 else n - L + 1
            pos = max(0, min(pos, n - L + 1))
            st = int(rng.integers(0, 4))
            insert = (0, L + 1, L - 3, -(L - 3), 250, L + 7, -L)[k % 7]
            cut = (-1, -1, pos + L // 2, pos + L + 5, -1, max(pos - 2, 0), -1, pos + L - 1, -1)[k % 9] if insert > 0 else -1
            ref = self.refs[c] + "A"
            read = make_read(rng, ref, pos, L, st)
            if k % 8 == 0:   # non-converted: keeps its non-CpG cytosines too
                read = "".join(r if r in "CG" and x in "TA" and rng.random() < 0.9 else x for r, x in zip(ref[pos:pos + L], read))
            alns.append((c, pos, st, insert, cut, read))
        for i in rng.integers(0, len(alns), 60).tolist():   # the same fragment with other letters
            c, pos, st, insert, cut, s = alns[i]
            alns.append((c, pos, st, insert, cut, make_read(rng, self.refs[c] + "A", pos, len(s), st)))
        for st in range(4):   # a position behind the chromosome's end: rejected by the window's bounds test, in the model and in meth_window
            alns.append((st % 3, len(self.refs[st % 3]) + 5, st, 0, -1, "ACGTCGCGCGCGTT"))
        self.alns = alns
        self._cells = {}

    def cells(self, *key):
        if key not in self._cells:
            self._cells[key] = E.epi_cells(self.refs, self.alns, *key)
        return self._cells[key]


@pytest.fixture(scope="module")
def parity(tmp_path_factory):
    p = Parity()
    p.dir = tmp_path_factory.mktemp("epi_parity")
    p.fa = U.write_fasta(p.dir / "parity.fa", p.names, p.refs)
    return p


CONFIGS = [  # trim_fillin, rm_dup, trim5, trim3, nonconv
    (0, False, 0, 0, 0),
    (2, False, 0, 0, 2),
    (2, True, 0, 0, 0),
    (0, True, 3, 2, 2),
    (2, False, 5, 0, 0),
    (2, True, 0, 7, 2),
]


@pytest.mark.parametrize("trim_fillin,rm_dup,trim5,trim3,nonconv", CONFIGS)
def test_model_parity(parity, trim_fillin, rm_dup, trim5, trim3, nonconv):
    key = (trim_fillin, rm_dup, trim5, trim3, nonconv)
    want = E.epi_rows(parity.cells(*key), parity.refs)
    # not vacuous: rows from every strand code alone, windows that a read loses to an X, reads that the filter, -r and the bounds test take away
    states = E.states_of(parity.refs, parity.alns, *key)
    for st in range(4):
        mine = [a for a in parity.alns if a[2] == st]
        assert len(E.epi_rows(E.epi_cells(parity.refs, mine, *key), parity.refs)) >= 20
    assert sum(1 for s in states if s and any("X" in [x for _, x in s[a:a + 4]] for a in range(len(s) - 3))) >= 20
    assert len(want) > 200 and sum(1 for s in states if s is None) >= 5 and any(a[4] >= 0 for a in parity.alns)
    if nonconv:
        assert sum(1 for s in E.states_of(parity.refs, parity.alns, trim_fillin, rm_dup, trim5, trim3, 0) if s is not None) > sum(1 for s in states if s is not None) + 20
    third = len(parity.alns) // 3
    for split in ((len(parity.alns),), (third, third + 1, len(parity.alns) - 2 * third - 1)):
        with handle(parity.fa, rm_dup=rm_dup, nonconv=nonconv, trim=(trim5, trim3)) as h:
            at = 0
            for part in split:
                h.add(parity.alns[at:at + part], trim_fillin)
                at += part
            assert U.epi_rows(h, 3) == want
            assert U.epi_rows(h, 3, 3) == E.epi_rows(parity.cells(*key), parity.refs, 3)


# ---- contention ------------------------------------------------------------------------------------------------------------------------------
def test_contention(example_fa):
    """5 000 identical reads on one window: one cell holds 5 000"""
    read = (0, 0, 0, 0, -1, EX_ALNS[2][5][:16])   # M U M U at 2, 6, 10, 14
    assert E.epi_cells([EX_REF], [read], 0) == [{0: pat(MUMU=1)}]
    with handle(example_fa) as h:
        h.add([read] * 5000, 0)
        assert U.epi_rows(h, 1) == [(0, (2, 6, 10, 14), pat(MUMU=5000))] and U.epi_rows(h, 1, 5000) == U.epi_rows(h, 1) and U.epi_rows(h, 1, 5001) == []


# ---- independence ----------------------------------------------------------------------------------------------------------------------------
def test_everything_else_is_unchanged(parity):
    """with the tally on, the table rows, the valid mappings, the PDR rows, the histogram, the M-bias cells and the C/T-SNP cells are those of a handle with
    it off; bsx_meth_combine_cpg leaves the epiallele rows as they are"""
    want = E.epi_rows(parity.cells(2, True, 0, 0, 2), parity.refs)
    R = RL.analyse(parity.refs, parity.alns, 2, True, 0, 0, 2, 4)
    assert R.nmap > 500 and R.dropped > 100
    kw = dict(rm_dup=True, nonconv=2, stats=True, min_cpg=4, snp=1, mbias=True)
    with handle(parity.fa, epi=True, **kw) as on, handle(parity.fa, epi=False, **kw) as off:
        on.add(parity.alns, 2)
        off.add(parity.alns, 2)
        assert U.epi_rows(on, 3) == want
        for fold in (False, True):
            if fold:
                on.combine_cpg(); off.combine_cpg()
            rows = U.rows_and_rev(on, 3, 1)
            assert rows == U.rows_and_rev(off, 3, 1) and len(rows[0]) > 1000 and len(rows[1]) == len(rows[0])
            assert on.valid_mappings() == off.valid_mappings() == R.nmap and on.nonconv_dropped() == off.nonconv_dropped() == R.dropped
            assert U.pdr_rows(on, 3) == U.pdr_rows(off, 3) != [] and U.read_hist(on) == U.read_hist(off) and U.mbias_cells(on) == U.mbias_cells(off) and len(U.mbias_cells(on)[0]) > 100
            assert U.epi_rows(on, 3) == want


# ---- state and errors --------------------------------------------------------------------------------------------------------------------------
def test_state_and_errors(example_fa, tmp_path):
    buf = np.zeros(4096, np.uint32)
    p = buf.ctypes.data
    n64, nr = C.c_uint64(), C.c_uint32()
    with handle(example_fa, epi=False) as h:
        L = h.L
        assert L.bsx_meth_n_cpg(h.h, 0, C.byref(n64)) == BSX_ERR_STATE and L.bsx_meth_epi_report_chr(h.h, 0, 1, C.byref(nr)) == BSX_ERR_STATE
        assert L.bsx_meth_epi_fetch_rows(h.h, p, p) == BSX_ERR_STATE
        assert L.bsx_meth_write_epi(h.h, str(tmp_path / "e").encode(), 1, None) == BSX_ERR_STATE and not os.path.exists(tmp_path / "e")
        assert b"bsx_meth_set_epi" in L.bsx_last_error_detail()
        assert L.bsx_meth_set_epi(h.h, 1) == 0 and L.bsx_meth_n_cpg(h.h, 0, C.byref(n64)) == 0 and n64.value == 5
        assert L.bsx_meth_n_cpg(h.h, 1, C.byref(n64)) == BSX_ERR_ARG and L.bsx_meth_n_cpg(h.h, 0, None) == BSX_ERR_ARG
        assert L.bsx_meth_epi_report_chr(h.h, 0, 0, C.byref(nr)) == BSX_ERR_ARG and L.bsx_meth_epi_report_chr(h.h, 1, 1, C.byref(nr)) == BSX_ERR_ARG
        assert L.bsx_meth_epi_report_chr(h.h, 0, 1, None) == BSX_ERR_ARG and L.bsx_meth_epi_fetch_rows(h.h, None, p) == BSX_ERR_ARG
        assert L.bsx_meth_epi_fetch_rows(h.h, p, None) == BSX_ERR_ARG and L.bsx_meth_write_epi(h.h, None, 1, None) == BSX_ERR_ARG
        assert L.bsx_meth_write_epi(h.h, str(tmp_path / "e").encode(), 0, None) == BSX_ERR_ARG
        assert L.bsx_meth_set_epi(h.h, 0) == 0 and L.bsx_meth_epi_report_chr(h.h, 0, 1, C.byref(nr)) == BSX_ERR_STATE       # off again before any add
        h.add(EX_ALNS, 0)
        assert L.bsx_meth_set_epi(h.h, 1) == BSX_ERR_STATE and L.bsx_meth_set_epi(h.h, 0) == 0                                # no change is no error
    with handle(example_fa) as h:
        h.add(EX_ALNS, 0)
        assert h.L.bsx_meth_set_epi(h.h, 0) == BSX_ERR_STATE and h.L.bsx_meth_set_epi(h.h, 1) == 0
        # an epiallele report between a table report and its fetch, and between a PDR report and its fetch, disturbs neither
    with handle(example_fa, min_cpg=4) as h, handle(example_fa, epi=False, min_cpg=4) as plain:
        h.add(EX_ALNS, 0)
        plain.add(EX_ALNS, 0)
        want_rows, want_pdr = U.rows_and_rev(plain, 1), U.pdr_rows(plain, 1)
        assert len(want_rows[0]) > 10 and len(want_pdr) == 10
        _check(h.L.bsx_meth_report_chr(h.h, 0, 1, 1, C.byref(nr), None, None))
        n_table = nr.value
        _check(h.L.bsx_meth_pdr_report_chr(h.h, 0, 1, C.byref(nr)))
        n_pdr = nr.value
        assert U.epi_rows(h, 1) == E.epi_rows(CELLS_N0, [EX_REF])
        pos, dep, met = (np.zeros(n_table, np.uint32) for _ in range(3))
        _check(h.L.bsx_meth_fetch_rows(h.h, pos.ctypes.data, dep.ctypes.data, met.ctypes.data))
        assert [(0,) + t for t in zip(pos.tolist(), dep.tolist(), met.tolist())] == want_rows[0]
        pos, reads, disc = (np.zeros(n_pdr, np.uint32) for _ in range(3))
        _check(h.L.bsx_meth_pdr_fetch_rows(h.h, pos.ctypes.data, reads.ctypes.data, disc.ctypes.data))
        assert [(0,) + t for t in zip(pos.tolist(), reads.tolist(), disc.tolist())] == want_pdr


def test_set_reference_rebuilds_the_index():
    """through bsx_meth_create: the index built for one text is discarded when the text changes"""
    with Meth.from_lengths([70, 9]) as h:
        first, second = ["AT" * 31 + "ACGCGCGC", "GCGACGTCG"], ["CG" * 35, "GCGCATATA"]
        h.set_epi()
        for refs in (first, second):
            for c, s in enumerate(refs):
                h.set_reference(c, s)
            assert n_cpg(h, 2) == [len(x) for x in E.cpgs(refs)]
        assert [len(x) for x in E.cpgs(first)] == [3, 3] and [len(x) for x in E.cpgs(second)] == [35, 1]


# ---- command line ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["bsp", "sam"])
def test_command_line(fmt, parity, tmp_path, capsys):
    from bsmap_amd import methratio
    path = str(tmp_path / ("in." + fmt))
    with open(path, "w") as f:
        if fmt == "sam":
            f.write("".join("@SQ\tSN:%s\tLN:%d\n" % (n, len(r)) for n, r in zip(parity.names, parity.refs)))
        for k, (c, pos, st, insert, cut, s) in enumerate(parity.alns):
            if fmt == "sam":  # PNEXT = cut_at + 1; 0 (with a positive insert: "no cut" in the C ABI) where the set has none
                f.write("r%d\t0\t%s\t%d\t255\t%dM\t=\t%d\t%d\t%s\t%s\tNM:i:0\tZS:Z:%s\n" % (k, parity.names[c], pos + 1, len(s), cut + 1, insert, s, "I" * len(s), STRANDS[st]))
            else:
                f.write("r%d\t%s\t%s\tUM\t%s\t%d\t%s\t%d\n" % (k, s, "I" * len(s), parity.names[c], pos + 1, STRANDS[st], insert))
    alns = parity.alns if fmt == "sam" else [(c, pos, st, insert, -1, s) for c, pos, st, insert, cut, s in parity.alns]  # a BSP line carries no mate position
    cells = E.epi_cells(parity.refs, alns, 2, True, 0, 0, 2)
    want = E.epi_text(parity.names, parity.refs, cells, 2)
    assert 100 < want.count("\n") < E.epi_text(parity.names, parity.refs, cells).count("\n") and want.split("\n")[1].startswith("p0\t")   # sorted by name
    out, out2, epi = (str(tmp_path / x) for x in ("t.txt", "t2.txt", "epi.txt"))
    methratio.main(["-q", "-z", "-r", "-g", "--nonconv-filter", "2", "--epi", epi, "--epi-min-reads", "2", "-o", out, "-d", parity.fa, path])
    summary = capsys.readouterr().out
    assert E.same_text(open(epi).read(), want)
    methratio.main(["-q", "-z", "-r", "-g", "--nonconv-filter", "2", "-o", out2, "-d", parity.fa, path])
    assert capsys.readouterr().out == summary and open(out, "rb").read() == open(out2, "rb").read() and open(out).read().count("\n") > 1000
