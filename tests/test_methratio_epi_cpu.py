"""Epiallele patterns of bsmap_amd.methratio (--epi) without a GPU: the model of epi_model.py pinned to a worked example that is written out
literally here, the model's edge cases, the option parser, the argument checks of the new C ABI entry points (a null handle needs no device), and the
host formatter of bsmap_amd/csrc/bsx_meth_epi.h under AddressSanitizer + UndefinedBehaviorSanitizer through tests/harness/epi_check.cpp."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import epi_model as E
from conftest import HOST_SAN_FLAGS
from test_methratio_readlevel_cpu import ALNS, READS, REF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BSX_ERR_ARG = -1


def pat(**kw):
    """sixteen counts from pattern = count; patterns are written as in the file's header, leftmost CpG first: pat(MUMU=1) is index 5"""
    out = [0] * 16
    for name, n in kw.items():
        out[E.PATTERNS.index(name)] = n
    return out


# ---- the worked example: REF has its five CpGs at 2, 6, 10, 14, 18; reads 1-7 of READS, trim_fillin 0 ----
# states of the five CpGs per read: 1 MMMMM, 2 UUUUU, 3 MUMUM, 4 MMMMM (dropped at N = 3), 5 ('-+', A over the G at 11) MMUMM, 6 MUM (three CpGs only),
# 7 ('--', A over every G) UUUUU
HEADER = ("chr\tpos1\tpos2\tpos3\tpos4\treads\tmeth\tmean\tepipoly\tentropy\tUUUU\tMUUU\tUMUU\tMMUU\tUUMU\tMUMU\tUMMU\tMMMU\tUUUM\tMUUM\tUMUM\tMMUM\tUUMM\tMUMM\tUMMM\t"
          "MMMM\n")
CELLS_N3 = [{0: pat(UUUU=2, MUMU=1, MMUM=1, MMMM=1), 1: pat(UUUU=2, UMUM=1, MUMM=1, MMMM=1)}]
CELLS_N0 = [{0: pat(UUUU=2, MUMU=1, MMUM=1, MMMM=2), 1: pat(UUUU=2, UMUM=1, MUMM=1, MMMM=2)}]
TEXT_N3 = (HEADER + "one\t3\t7\t11\t15\t5\t9\t0.450\t0.7200\t0.4805\t2\t0\t0\t0\t0\t1\t0\t0\t0\t0\t0\t1\t0\t0\t0\t1\n"
           + "one\t7\t11\t15\t19\t5\t9\t0.450\t0.7200\t0.4805\t2\t0\t0\t0\t0\t0\t0\t0\t0\t0\t1\t0\t0\t1\t0\t1\n")
TEXT_N0 = (HEADER + "one\t3\t7\t11\t15\t6\t13\t0.542\t0.7222\t0.4796\t2\t0\t0\t0\t0\t1\t0\t0\t0\t0\t0\t1\t0\t0\t0\t2\n"
           + "one\t7\t11\t15\t19\t6\t13\t0.542\t0.7222\t0.4796\t2\t0\t0\t0\t0\t0\t0\t0\t0\t0\t1\t0\t0\t1\t0\t2\n")


def test_worked_example_cells_and_rows():
    assert E.EPI_HEADER == HEADER and E.cpgs([REF]) == [[2, 6, 10, 14, 18]]
    assert CELLS_N3[0][0] == [2, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 0, 1] and CELLS_N3[0][1] == [2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 1, 0, 1]   # {0:2, 5:1, 11:1, 15:1}, {0:2, 10:1, 13:1, 15:1}
    states = E.states_of([REF], ALNS, trim_fillin=0, nonconv=3)
    assert ["".join(s for _, s in st) if st is not None else None for st in states] == ["MMMMM", "UUUUU", "MUMUM", None, "MMUMM", "MUM", "UUUUU"]
    cells = E.epi_cells([REF], ALNS, trim_fillin=0, nonconv=3)
    assert cells == CELLS_N3
    assert E.epi_rows(cells, [REF]) == [(0, (2, 6, 10, 14), CELLS_N3[0][0]), (0, (6, 10, 14, 18), CELLS_N3[0][1])]
    assert E.epi_rows(cells, [REF], 5) == E.epi_rows(cells, [REF]) and E.epi_rows(cells, [REF], 6) == []
    for counts in cells[0].values():
        reads, meth, mean, epipoly, entropy = E.scores(counts)
        assert (reads, meth) == (5, 9) and "%.4f %.4f" % (epipoly, entropy) == "0.7200 0.4805"
    cells0 = E.epi_cells([REF], ALNS, trim_fillin=0, nonconv=0)    # read 4 is kept: MMMM becomes 2 in both windows
    assert cells0 == CELLS_N0 and len(E.epi_rows(cells0, [REF], 6)) == 2 and E.epi_rows(cells0, [REF], 7) == []
    for counts in cells0[0].values():
        reads, meth, mean, epipoly, entropy = E.scores(counts)
        assert (reads, meth) == (6, 13) and "%.4f %.4f" % (epipoly, entropy) == "0.7222 0.4796"
    assert E.epi_cells([REF], [ALNS[5]], trim_fillin=0) == [{}]   # read 6 has three CpGs: in no window


def test_worked_example_files():
    assert E.epi_text(["one"], [REF], CELLS_N3) == TEXT_N3 and E.epi_text(["one"], [REF], CELLS_N0) == TEXT_N0
    assert E.epi_text(["one"], [REF], CELLS_N3, 6) == HEADER and E.epi_text(["one"], [REF], [{}]) == HEADER
    assert E.same_text(TEXT_N3, TEXT_N3) and not E.same_text(TEXT_N3, TEXT_N0) and not E.same_text(TEXT_N3, HEADER)
    assert E.same_text(TEXT_N3.replace("0.4805", "0.4806"), TEXT_N3) and not E.same_text(TEXT_N3.replace("0.4805", "0.4807"), TEXT_N3)
    assert not E.same_text(TEXT_N3.replace("\t5\t9\t", "\t5\t8\t"), TEXT_N3)


METH = READS[0][1]   # '++', every CpG methylated, 40 letters
MINUS = REF          # under '-+' the reference's own letters: every G shown, every CpG methylated


def one(aln, **kw):
    return E.epi_cells([REF], [aln], **dict(dict(trim_fillin=0), **kw))[0]


def test_model_three_and_four_cpgs():
    assert one((0, 0, 0, 0, -1, METH[:14])) == {}                                   # exactly three CpGs (C at 2, 6, 10): in no window
    assert one((0, 0, 0, 0, -1, METH[:16])) == {0: pat(MMMM=1)}                     # exactly four: one window
    assert one((0, 4, 0, 0, -1, METH[4:20])) == {1: pat(MMMM=1)}
    assert one((0, 4, 0, 0, -1, READS[2][1][4:20])) == {1: pat(UMUM=1)}             # read 3 shows M U M U M


def test_model_plus_read_ending_on_a_c_and_minus_read_starting_on_a_g():
    assert one((0, 0, 0, 0, -1, METH[:15])) == {0: pat(MMMM=1)}                     # '+' read whose last letter is the C at 14: that CpG is covered
    assert one((0, 0, 0, 0, -1, METH[:14])) == {}
    assert one((0, 0, 0, 0, -1, METH[:19])) == {0: pat(MMMM=1), 1: pat(MMMM=1)}     # ... and the C at 18
    assert one((0, 0, 0, 0, -1, METH[:18])) == {0: pat(MMMM=1)}
    assert one((0, 3, 1, 0, -1, MINUS[3:20])) == {0: pat(MMMM=1), 1: pat(MMMM=1)}   # '-' read whose first letter is the G at 3: the CpG at 2 is covered
    assert one((0, 4, 1, 0, -1, MINUS[4:20])) == {1: pat(MMMM=1)}
    assert one((0, 3, 1, 0, -1, MINUS[3:19])) == {0: pat(MMMM=1)}                   # ends in front of the G at 19
    assert one((0, 2, 0, 0, -1, METH[2:19])) == one((0, 3, 1, 0, -1, MINUS[3:20]))  # both strands feed the same cells


def test_model_x_in_the_middle():
    sub = lambda s, at, x: s[:at] + x + s[at + 1:]
    assert one((0, 0, 0, 0, -1, sub(METH, 10, "A"))) == {}                          # a mismatch at the third CpG: it is in both windows
    assert one((0, 0, 0, 0, -1, sub(METH, 10, "N"))) == {}
    assert one((0, 0, 0, 0, -1, sub(METH, 2, "N"))) == {1: pat(MMMM=1)}             # at the first: window 1 is intact
    assert one((0, 0, 0, 0, -1, sub(METH, 18, "G"))) == {0: pat(MMMM=1)}
    assert one((0, 0, 0, 0, -1, sub(METH, 10, "T"))) == {0: pat(MMUM=1), 1: pat(MUMM=1)}   # converted: U, not X
    assert one((0, 0, 1, 0, -1, sub(MINUS, 11, "T"))) == {}                         # '-' read: the call is at the G


def test_model_masked_cycles():
    plus, minus = (0, 0, 0, 0, -1, METH[:20]), (0, 0, 1, 0, -1, MINUS[:20])          # 20 letters: '++' cycle = letter, '-+' cycle = 19 - letter
    both = {0: pat(MMMM=1), 1: pat(MMMM=1)}
    assert one(plus) == one(minus) == both
    assert one(plus, trim5=2) == both and one(plus, trim5=3) == {1: pat(MMMM=1)}     # the C at 2 is cycle 2
    assert one(plus, trim3=1) == both and one(plus, trim3=2) == {0: pat(MMMM=1)}     # the C at 18 is cycle 18 of 20
    assert one(minus, trim5=1) == {0: pat(MMMM=1)}                                   # the G at 19 is cycle 0
    assert one(minus, trim3=3) == both and one(minus, trim3=4) == {1: pat(MMMM=1)}   # the G at 3 is cycle 16 of 20
    assert one(plus, trim5=3, trim3=2) == {} and one(minus, trim5=1, trim3=4) == {}
    assert one((0, 0, 0, 20, -1, METH[:20]), trim_fillin=2) == {0: pat(MMMM=1)}      # the fill-in trim takes the last two letters: not X, not covered
    assert one((0, 0, 0, 30, 18, METH[:20])) == {0: pat(MMMM=1)}                     # cut_at likewise


TWO = ["ACGTCGTCGTC", "GTCGTCGTCGTCGT"]   # the first ends in C, the second starts with G


def test_model_cg_across_two_sequences_and_small_chromosomes():
    assert E.cpgs(TWO) == [[1, 4, 7], [2, 5, 8, 11]]                                  # the C at 10 of the first is no CpG
    assert E.cpgs(["ATATAT", "C", "G", "", "CG", "GC"]) == [[], [], [], [], [0], []]
    full = [(0, 0, 0, 0, -1, TWO[0]), (1, 0, 0, 0, -1, TWO[1]), (1, 0, 1, 0, -1, TWO[1])]
    assert E.epi_cells(TWO, full, trim_fillin=0) == [{}, {0: pat(MMMM=2)}]            # three CpGs: no window; four: one, from both strands
    assert E.epi_rows(E.epi_cells(TWO, full, trim_fillin=0), TWO) == [(1, (2, 5, 8, 11), pat(MMMM=2))]
    refs = ["ATATATAT", TWO[0], TWO[1]]                                                # 0, 3 and 4 CpGs
    cells = E.epi_cells(refs, [(0, 0, 0, 0, -1, refs[0]), (1, 0, 0, 0, -1, refs[1]), (2, 0, 3, 0, -1, "GTCATCATCATCAT")], trim_fillin=0)
    assert cells == [{}, {}, {0: pat(UUUU=1)}]
    assert E.epi_text(["n", "a", "b"], refs, cells) == HEADER + "b\t3\t6\t9\t12\t1\t0\t0.000\t0.0000\t0.0000\t1" + "\t0" * 15 + "\n"


def test_model_duplicates_and_invalid_reads():
    a = (0, 0, 0, 0, -1, METH)
    assert one(a) == {0: pat(MMMM=1), 1: pat(MMMM=1)}
    assert E.epi_cells([REF], [a, (0, 0, 0, 0, -1, READS[1][1])], trim_fillin=0, rm_dup=True) == [{0: pat(MMMM=1), 1: pat(MMMM=1)}]   # -r keeps the first
    assert E.epi_cells([REF], [a, (0, 0, 0, 0, -1, READS[1][1])], trim_fillin=0) == [{0: pat(MMMM=1, UUUU=1), 1: pat(MMMM=1, UUUU=1)}]
    assert E.epi_cells([REF], [ALNS[3], a], trim_fillin=0, rm_dup=True, nonconv=3) == [{}]   # the dropped owner still suppresses its duplicate
    assert one((0, 1, 0, 0, -1, METH)) == {} and one((0, 41, 0, 0, -1, "CG")) == {}            # past the end: not a valid mapping


# ---- the option surface ----
def test_option_parser():
    from bsmap_amd import methratio
    ap = methratio.build_parser()
    base = ["-o", "t", "-d", "r.fa", "in.bsp"]
    o = ap.parse_args(base)
    assert (o.epi, o.epi_min_reads) == (None, None)
    o = ap.parse_args(["--epi", "e.txt"] + base)
    assert (o.epi, o.epi_min_reads) == ("e.txt", None)
    o = ap.parse_args(["--epi", "e.txt", "--epi-min-reads", "10"] + base)
    assert (o.epi, o.epi_min_reads) == ("e.txt", 10)
    for bad in (["--epi-min-reads", "1"], ["--epi", "e", "--epi-min-reads", "0"], ["--epi", "e", "--epi-min-reads", "x"], ["--epi"]):
        with pytest.raises(SystemExit):
            ap.parse_args(bad + base)


def test_run_rejects_before_it_touches_the_library():
    from bsmap_amd import methratio
    for kw in (dict(epi_min_reads=1), dict(epi="e", epi_min_reads=0), dict(epi="e", epi_min_reads=-2)):
        with pytest.raises(ValueError):
            methratio.run("no-such.fa", ["no-such.bsp"], "no-such.txt", **kw)


def test_null_handle_is_an_argument_error():
    """every new entry point, with a null handle and (where it has one) a null out pointer: BSX_ERR_ARG before any device call"""
    from bsmap_amd import methratio
    L = methratio._bind()
    buf = (C.c_uint64 * 1024)()
    p = C.addressof(buf)
    assert L.bsx_meth_set_epi(None, 1) == BSX_ERR_ARG
    assert L.bsx_meth_n_cpg(None, 0, p) == BSX_ERR_ARG
    assert L.bsx_meth_epi_report_chr(None, 0, 1, p) == BSX_ERR_ARG
    assert L.bsx_meth_epi_fetch_rows(None, p, p) == BSX_ERR_ARG
    assert L.bsx_meth_write_epi(None, b"x", 1, None) == BSX_ERR_ARG


# ---- the formatter, compiled on its own under the host sanitizers ----
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("epi") / "epi_check")
    subprocess.run(["g++"] + HOST_SAN_FLAGS + ["-o", exe, os.path.join(ROOT, "tests", "harness", "epi_check.cpp")], check=True)   # (ASan + UBSan: conftest.py)
    return exe


def formatted(exe, rows):
    """rows: [(name, four 0-based positions, sixteen counts)] -> the harness's text"""
    text = "".join("%s %s %s\n" % (name, " ".join(map(str, pos)), " ".join(map(str, counts))) for name, pos, counts in rows)
    r = subprocess.run([exe], input=text.encode(), capture_output=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr.decode(errors="replace")[-3000:])
    return r.stdout.decode()


def test_formatter_equals_the_model(harness):
    rng = np.random.default_rng(11)
    rows = [("one", (2, 6, 10, 14), CELLS_N3[0][0]), ("one", (6, 10, 14, 18), CELLS_N3[0][1]), ("one", (2, 6, 10, 14), CELLS_N0[0][0]),
            ("chr1", (0, 2, 4, 6), pat(UMUM=1)),                              # one read
            ("chr1", (9, 99, 999, 9999), pat(MMMM=12345)),                    # one pattern: both scores 0
            ("a_long_sequence_name.1", (4294967291, 4294967292, 4294967293, 4294967294), [3] * 16),   # all sixteen equal: both at their maxima
            ("x", (1, 2, 3, 4), [4294967295] * 16),                           # the sum does not fit 32 bits
            ("x", (1, 2, 3, 4), pat(UUUU=1, MMMM=1)), ("x", (1, 2, 3, 4), pat(UUUU=999999, MUUU=1))]
    for _ in range(200):
        counts = (rng.integers(0, 50, 16) * (rng.random(16) < rng.random())).tolist()
        if sum(counts):
            rows.append(("r", tuple(sorted(rng.integers(0, 1 << 31, 4).tolist())), counts))
    want = E.EPI_HEADER + "".join(E.row_text(*r) for r in rows)
    got = formatted(harness, rows)
    assert E.same_text(got, want), (got[:2000], want[:2000])
    lines = got.split("\n")
    assert lines[0] + "\n" == HEADER and lines[1] + "\n" + lines[2] + "\n" == TEXT_N3[len(HEADER):]   # the worked example, byte for byte
    assert lines[4].split("\t")[5:10] == ["1", "2", "0.500", "0.0000", "0.0000"]
    assert lines[5].split("\t")[5:10] == ["12345", "49380", "1.000", "0.0000", "0.0000"]
    assert lines[6].split("\t")[:10] == ["a_long_sequence_name.1", "4294967292", "4294967293", "4294967294", "4294967295", "48", "96", "0.500", "0.9375", "1.0000"]
    assert lines[7].split("\t")[5:10] == [str(16 * 4294967295), str(32 * 4294967295), "0.500", "0.9375", "1.0000"]
    assert lines[8].split("\t")[5:10] == ["2", "4", "0.500", "0.5000", "0.2500"]
    assert formatted(harness, []) == HEADER
