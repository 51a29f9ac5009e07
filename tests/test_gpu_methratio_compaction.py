"""The three reports of bsmap_amd.methratio that list their rows by ordered compaction (compact_count / compact_emit of bsx_meth.hip under the table's, the
PDR's and the epiallele rule; bsx_meth_report_chr, bsx_meth_pdr_report_chr, bsx_meth_epi_report_chr) through every cut of the shared loop: rows at the
first and the last lane of a wave, of a round of 256 items and of a block of 1 024, a last block of 4 items, a sequence of one item and one of none, all
behind a first sequence, so that the base offsets (g0, the first CpG's ordinal) are not 0.  Every expectation comes from ctsnp_model.py, readlevel_model.py
and epi_model.py, which never look at the library, and is formed before the library is touched; a test without a GPU checks that the expected sets are the
ones this text names, so that no comparison on the GPU is one of two empty lists.

  a   ACGCGCGCGT        four CpGs, one window; one read on it
  b   "CG" x 2055, A    2 055 CpGs: 2 052 windows in three blocks, the last block holds 4; 4 111 positions in five blocks
  c   C                 one position, no CpG, no read
Reads are 8 letters on '++' at position 2w of b: such a read covers exactly window w and makes its calls at the four Cs; the Gs between them carry the
opposite-strand calls of the C/T-SNP mode."""
import ctypes as C
import functools

import pytest

from bsmap_amd import _check

import ctsnp_model as M
import epi_model as E
import readlevel_model as RL
import meth_util as U

NAMES = ["a", "b", "c"]
REFS = ["ACGCGCGCGT", "CG" * 2055 + "A", "C"]
N_WIN = 2052
SPARSE = (0, 63, 64, 255, 256, 1023, 1024, 1025, 2047, 2048, 2051)
TWICE = (64, 1024)   # the windows of the sparse set with a second read
NEVER = 3            # a threshold no cell of a meets: it has one read


def read_at(w, salt=0):
    """the read of window w: C or T at the four Cs by the bits of a pattern that changes with w, G or A at the four Gs likewise"""
    meth, rev = (w * 7 + 3 + salt) & 15, (w * 5 + 1 + salt) & 15
    return "".join(("C" if (meth >> j) & 1 else "T") + ("G" if (rev >> j) & 1 else "A") for j in range(4))


def alignments(kind):
    alns = [(0, 1, 0, 0, -1, "CGTGCGTG")]   # a: Cs at 1, 3, 5, 7
    for w in (SPARSE if kind == "sparse" else range(N_WIN)):
        alns.append((1, 2 * w, 0, 0, -1, read_at(w)))
        if kind == "sparse" and w in TWICE:
            alns.append((1, 2 * w, 0, 0, -1, read_at(w, salt=9)))
    return alns


@functools.lru_cache(maxsize=None)
def expected(kind):
    """the models' results for one read set, computed once"""
    alns = alignments(kind)
    K = M.pileup(REFS, alns, trim_fillin=0)
    X = {"alns": alns}
    # The C/T-SNP table is taken behind the CpG fold: a '+' read makes its opposite-strand calls at the Gs, and the fold brings them to the Cs the table lists
    for mode, Km in ((0, K), (1, M.combine_cpg(K))):
        for min_depth in (1, 2):
            for meth0 in (True, False):
                X["table", mode, min_depth, meth0] = M.rows(Km, min_depth, meth0, mode)
                X["text", mode, min_depth, meth0] = M.table(NAMES, Km, min_depth, meth0, mode)[0]
    X["table", 0, NEVER, True] = M.rows(K, NEVER, True, 0)
    R = RL.analyse(REFS, alns, trim_fillin=0, min_cpg=4)
    cells = E.epi_cells(REFS, alns, trim_fillin=0)
    for min_reads in (1, 2, NEVER):
        X["pdr", min_reads] = RL.pdr_rows(R.pdr, min_reads)
        X["epi", min_reads] = E.epi_rows(cells, REFS, min_reads)
    return X


def window_of(row):
    """the window of an epiallele row of b"""
    c, pos, _ = row
    assert c == 1 and pos == (pos[0], pos[0] + 2, pos[0] + 4, pos[0] + 6)
    return pos[0] // 2


def test_expected_sets_are_the_ones_named():
    for kind, windows in (("sparse", SPARSE), ("dense", tuple(range(N_WIN)))):
        X = expected(kind)
        on_b = [r for r in X["epi", 1] if r[0] == 1]
        assert tuple(window_of(r) for r in on_b) == windows and all(sum(r[2]) == (2 if kind == "sparse" and window_of(r) in TWICE else 1) for r in on_b)
        assert [window_of(r) for r in X["epi", 2] if r[0] == 1] == (list(TWICE) if kind == "sparse" else [])
        assert [r[:2] for r in X["epi", 1] if r[0] == 0] == [(0, (1, 3, 5, 7))] and all(r[0] != 2 for r in X["epi", 1]) and X["epi", NEVER] == []
        cs = sorted({2 * w + 2 * j for w in windows for j in range(4)})   # every C under a read has a PDR cell and a table row
        assert [i for c, i, _, _ in X["pdr", 1] if c == 1] == cs and [i for c, i, _, _ in X["pdr", 1] if c == 0] == [1, 3, 5, 7]
        assert 0 < len([r for r in X["pdr", 2] if r[0] == 1]) < len(cs) and all(r[0] == 1 for r in X["pdr", 2]) and all(r[0] == 1 for r in X["pdr", NEVER])
        for mode in (0, 1):
            listed = X["table", mode, 1, True][0]
            on_b = [i for c, i, *_ in listed if c == 1]   # mode 1 drops the Cs whose opposite-strand calls all show A
            assert (on_b == cs if mode == 0 else 0 < len(on_b) < len(cs) and set(on_b) < set(cs)) and [i for c, i, *_ in listed if c == 0] == [1, 3, 5, 7]
            assert all(c != 2 for c, *_ in listed)
            assert 0 < len(X["table", mode, 1, False][0]) < len(listed) and 0 < len(X["table", mode, 2, True][0]) < len(listed)
            assert all(c == 1 for c, *_ in X["table", mode, 2, True][0])
        snp_rows = X["table", 1, 1, True][0]
        assert any(0 < g < ga for *_, g, ga in snp_rows) and any(0 < g == ga for *_, g, ga in snp_rows) and all(c == 1 for c, *_ in X["table", 0, NEVER, True][0])
    assert len(REFS[1]) == 4111 and E.cpgs(REFS)[1][-1] == 4108 and len(E.cpgs(REFS)[1]) - 3 == N_WIN == 2 * 1024 + 4
    # rows at both ends of a wave, a round and a block of the epiallele report, and of the position reports (position 2w)
    assert {0, 63, 64, 255, 256, 1023, 1024, 2047, 2048, 2051} <= set(SPARSE) and {0, 512, 2048, 4096, 4108} <= {i for c, i, _, _ in expected("sparse")["pdr", 1] if c == 1}


@pytest.fixture(scope="module")
def fasta(tmp_path_factory):
    return U.write_fasta(tmp_path_factory.mktemp("compaction") / "three.fa", NAMES, REFS)


def row_counts(h, report, *args):
    """the number of rows every sequence's report call sets, with the counts it fills preset to a value no report here gives: an empty report has to write its 0"""
    per_chr = []
    for c in range(len(REFS)):
        out = [C.c_uint32(0xFFFFFFFF)] + [C.c_uint64(0xFFFFFFFFFFFFFFFF) for _ in range(2 if report == "bsx_meth_report_chr" else 0)]
        _check(getattr(h.L, report)(h.h, c, *args, *[C.byref(x) for x in out]))
        assert all(x.value < 0xFFFFFFFF for x in out)
        per_chr.append(out[0].value)
    return per_chr


def table_rows(h, min_depth, meth0, snp):
    """([(chr id, pos, depth, meth, rev_g, rev_ga)], n_covered, sum_depth, rows per sequence) over all sequences; rev_g = rev_ga = 0 with the mode off"""
    got, nc, nd = U.table_rows(h, len(REFS), min_depth, meth0, bool(snp), pad=True)
    per_chr = row_counts(h, "bsx_meth_report_chr", min_depth, 1 if meth0 else 0)
    assert per_chr == [sum(1 for r in got if r[0] == c) for c in range(len(REFS))]
    return got, nc, nd, per_chr


def table_text(h, path, min_depth, meth0):
    nc, nd = h.write_table(path, min_depth, meth0)
    return open(path).read(), nc, nd


def pdr_rows(h, min_reads):
    got, per_chr = U.pdr_rows(h, len(REFS), min_reads), row_counts(h, "bsx_meth_pdr_report_chr", min_reads)
    assert per_chr == [sum(1 for r in got if r[0] == c) for c in range(len(REFS))]
    return got, per_chr


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["sparse", "dense"])
def test_reports_equal_the_models(fasta, tmp_path, kind):
    X = expected(kind)
    for mode in (0, 1):   # the table without and with its two extra columns
        with U.open_meth(fasta, snp=mode) as h:
            h.add(X["alns"], 0)
            if mode:
                h.combine_cpg()
            for min_depth in (1, 2):
                for meth0 in (True, False):
                    want, nc, nd = X["table", mode, min_depth, meth0]
                    want = [(c, i, dd, m) + ((g, ga) if mode else (0, 0)) for c, i, dd, m, g, ga in want]
                    got, gnc, gnd, per_chr = table_rows(h, min_depth, meth0, mode)
                    assert len(got) == len(want) > 0 and got == want and (gnc, gnd) == (nc, nd) and per_chr[2] == 0
                    assert table_text(h, tmp_path / ("t%d%d%d.txt" % (mode, min_depth, meth0)), min_depth, meth0) == (X["text", mode, min_depth, meth0], nc, nd)
            if mode == 0:
                got, _, _, per_chr = table_rows(h, NEVER, True, 0)
                assert got == [(c, i, dd, m, 0, 0) for c, i, dd, m, _, _ in X["table", 0, NEVER, True][0]] and per_chr[0] == 0 and per_chr[2] == 0
    with U.open_meth(fasta, min_cpg=4, epi=True) as h:   # PDR and the epiallele tally
        h.add(X["alns"], 0)
        for min_reads in (1, 2, NEVER):
            got, per_chr = pdr_rows(h, min_reads)
            assert got == X["pdr", min_reads] and per_chr[2] == 0 and (min_reads == 1 or per_chr[0] == 0)
            assert U.epi_rows(h, len(REFS), min_reads) == X["epi", min_reads]
        assert len(pdr_rows(h, 1)[0]) > 0 and len(U.epi_rows(h, len(REFS), 1)) == len(X["epi", 1]) > 0
        assert [h.n_cpg(c) for c in range(len(REFS))] == [4, 2055, 0] and U.epi_rows(h, len(REFS), NEVER) == []
