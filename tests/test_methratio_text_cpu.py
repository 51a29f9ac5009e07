"""The row formatters of bsmap_amd/csrc/bsx_meth_text.h (the table with 9 and 12 columns, the region file, the wiggle track, the PDR file) without a GPU:
tests/harness/meth_text_check.cpp compiles the header on its own under AddressSanitizer + UndefinedBehaviorSanitizer, reads counters on stdin and prints the
rows, and the rows are compared byte for byte (the rule of the GPU tests of these files) with the text of ctsnp_model.py, regions_model.py and
readlevel_model.py, which never look at the library."""
import os
import subprocess

import numpy as np
import pytest

import ctsnp_model as M
import readlevel_model as RL
import regions_model as RG
from conftest import HOST_SAN_FLAGS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LONG = "a_long_sequence_name." + "x" * 400 + ".1"   # longer than any fixed line buffer
LAST = (1 << 32) - 2                                 # the last position a 32-bit 0-based position can name with its 1-based form


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("meth_text") / "meth_text_check")
    subprocess.run(["g++"] + HOST_SAN_FLAGS + ["-o", exe, os.path.join(ROOT, "tests", "harness", "meth_text_check.cpp")], check=True)   # (ASan + UBSan: conftest.py)
    return exe


def formatted(exe, lines):
    r = subprocess.run([exe], input="".join(x + "\n" for x in lines).encode(), capture_output=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr.decode(errors="replace")[-3000:])
    return r.stdout.decode()


def packed(ref, i):
    """the packed context k_meth_emit writes for position i of `ref`: the letters of ref[i-2:i+3] (Python's slice) from byte 0 on, the letter at i in byte 7"""
    return sum(ord(ch) << (8 * k) for k, ch in enumerate(ref[i - 2:i + 3])) | (ord(ref[i]) << 56)


def table_case(names, refs, cells, mode):
    """cells: {(chr id, pos): (depth, meth, rev_g, rev_ga)} -> (the harness's input, the model's table without its header)"""
    K = M.Counters(refs)
    for (c, i), (dd, m, g, ga) in cells.items():
        K.depth[c][i], K.meth[c][i], K.rev_g[c][i], K.rev_ga[c][i] = dd, m, g, ga
    text, _, _ = M.table(names, K, min_depth=1, meth0=True, mode=mode)
    listed, _, _ = M.rows(K, 1, True, mode)
    assert len(listed) == len(cells)   # every case is a row of the model's table
    by_name = sorted(listed, key=lambda r: (names[r[0]], r[1]))
    kind = "table12" if mode else "table9"
    lines = ["%s %s %d %d %d %d" % (kind, names[c], i, dd, m, packed(refs[c], i)) + (" %d %d" % (g, ga) if mode else "") for c, i, dd, m, g, ga in by_name]
    return lines, text[len(M.HEADER12 if mode else M.HEADER9):]


REFS = ["ACGTCCGGTTAGC", "C", "CCGG", "GATTACAG"]
NAMES = ["chr2", LONG, "chr10", "b"]   # sorted order: LONG, b, chr10, chr2


def test_table_rows_equal_the_model(harness):
    plain = {(0, 1): (1, 1, 0, 0), (0, 2): (1, 0, 0, 0),                # depth 1, methylated and not
             (0, 4): (7, 3, 0, 0), (0, 5): (4294967295, 4294967295, 0, 0), (0, 12): (12, 12, 0, 0),
             (1, 0): (3, 2, 0, 0),                                      # a one-letter sequence with a long name: its context is "C"
             (2, 0): (5, 1, 0, 0), (2, 1): (9, 9, 0, 0), (2, 3): (2, 0, 0, 0),   # below five letters the slice start is negative ("CCGG": position 1 -> "G")
             (3, 0): (10, 4, 0, 0), (3, 7): (1, 1, 0, 0)}
    lines, want = table_case(NAMES, REFS, plain, 0)
    assert formatted(harness, lines) == want and want.count("\n") == len(plain)
    snp = {(0, 1): (1, 1, 0, 0),                                        # depth 1, no opposite-strand call
           (0, 2): (10, 4, 3, 5),                                       # g != ga: eff = 6.0
           (0, 4): (10, 8, 1, 4),                                       # m > effective depth (2.5): the clip, ratio 1.000
           (0, 5): (3, 3, 1, 3), (0, 12): (7, 0, 2, 3), (1, 0): (20, 5, 6, 6), (2, 1): (4294967295, 4294967295, 1, 4294967295),
           (3, 0): (9, 2, 4294967295, 4294967294), (3, 7): (1, 0, 1, 2)}
    for mode in (1, 2):
        cells = {k: v for k, v in snp.items() if mode == 1 or v[2] == v[3]}   # mode 2 lists only g == ga
        lines, want = table_case(NAMES, REFS, cells, mode)
        got = formatted(harness, lines)
        assert got == want and want.count("\n") == len(cells)
    rows = {tuple(x.split("\t")[:2]): x.split("\t") for x in formatted(harness, table_case(NAMES, REFS, snp, 1)[0]).split("\n") if x}
    assert rows[("chr2", "3")][4:8] == ["0.667", "6.00", "4", "10"] and rows[("chr2", "5")][4:6] == ["1.000", "2.50"]
    assert rows[(LONG, "1")][2:4] == ["+", "C"] and len(rows[(LONG, "1")]) == 12


def test_table_row_at_the_last_position_and_random_rows(harness):
    rng = np.random.default_rng(5)
    lines, want = [], []
    cases = [(LAST, 1, 1, 0, 0, 0), (LAST, 17, 5, 0, 0, 0), (LAST, 17, 5, 1, 2, 3), (LAST, 4, 4, 1, 1, 5)]
    for _ in range(300):
        dd = int(rng.integers(1, 200))
        mode = int(rng.integers(0, 3))
        ga = int(rng.integers(0, 50)) if mode else 0
        g = (int(rng.integers(1, ga + 1)) if ga else 0) if mode == 1 else ga
        cases.append((int(rng.integers(0, 1 << 32) - 1) % (LAST + 1), dd, int(rng.integers(0, dd + 1)), mode, g, ga))
    for k, (pos, dd, m, mode, g, ga) in enumerate(cases):
        ref = "TACGT" if k % 2 == 0 else "AACGA"   # the C at 2 ('+') or the G at 3 ('-')
        i = 2 if k % 2 == 0 else 3
        name = LONG if k % 7 == 0 else "chr%d" % k
        lines.append("%s %s %d %d %d %d" % ("table12" if mode else "table9", name, pos, dd, m, packed(ref, i)) + (" %d %d" % (g, ga) if mode else ""))
        want.append("%s\t%d\t%s\t%s\t%s\n" % (name, pos + 1, "+" if ref[i] == "C" else "-", ref[i - 2:i + 3], M.row_fields(dd, m, g, ga, mode)))
    got = formatted(harness, lines)
    assert got == "".join(want)
    assert got.split("\n")[0].split("\t")[:4] == [LONG, "4294967295", "+", "TACGT"]


def region_line(name, start, end, label, s):
    return "%s\t%d\t%d\t%s\t%s\n" % (name, start, end, label, RG.region_fields(s))


def test_region_and_wig_rows_equal_the_model(harness):
    rng = np.random.default_rng(6)
    one = 1 << 16
    sums = [[1, 1, 1, one, one],                      # one site of depth 1
            [1, 0, 1, one, 0],
            [3, 12, 30, 1179648, 655360],             # g != ga at a site: E = 18.0, MC = 10.0
            [2, 9, 10, 5 * one // 2, 5 * one // 2],   # the clip: MC == E below M
            [1, 3, 7, 0, 0],                          # E == 0 with a site: the NA row, no wig line
            [0, 0, 0, 0, 0],                          # no site: NA
            [4294967295, 1 << 40, 1 << 41, (1 << 41) * one, (1 << 40) * one]]
    for _ in range(200):
        n = int(rng.integers(1, 1000))
        d = int(rng.integers(n, 50 * n))
        e = int(rng.integers(1, d * one + 1))
        sums.append([n, int(rng.integers(0, d + 1)), d, e, int(rng.integers(0, e + 1))])
    lines, want = [], []
    for k, s in enumerate(sums):
        name, label = (LONG, "label_" + "y" * 300) if k % 5 == 0 else ("chr%d" % k, ".")
        start, end = (LAST, LAST + 1) if k % 3 == 0 else (k, 10 * k + 7)
        lines.append("region %s %d %d %s %d %d %d %d %d" % ((name, start, end, label) + tuple(s)))
        want.append(region_line(name, start, end, label, s))
    got = formatted(harness, lines)
    assert got == "".join(want)
    assert got.split("\n")[4].split("\t")[4:] == ["1", "3", "7", "0.00", "NA", "NA", "NA"] and got.split("\n")[0].split("\t")[:3] == [LONG, "4294967294", "4294967295"]
    # the wiggle lines of the same sums as the bins of two widths; the last bin of a 2^32 - 1 letter sequence at width 1 starts at 2^32 - 1
    for B, j0 in ((1, LAST - len(sums) + 1), (1000, 0)):
        lines = ["wig %d %d %d %d %d %d %d" % ((j0 + j, B) + tuple(s)) for j, s in enumerate(sums)]
        want = "".join("%d\t%.3f\n" % ((j0 + j) * B + 1, RG.ratio(s)) for j, s in enumerate(sums) if s[0] > 0 and s[3] > 0)
        got = formatted(harness, lines)
        assert got == want and got.count("\n") == len(sums) - 2
    assert formatted(harness, ["wig %d 1 1 1 1 65536 65536" % LAST]) == "4294967295\t1.000\n"


def test_pdr_rows_equal_the_model(harness):
    rng = np.random.default_rng(7)
    refs = ["ACGTCGACGG", "CG"]
    names = ["chr1", LONG]
    pdr = [[[0, 0] for _ in r] for r in refs]
    for c, i, r, d in ((0, 1, 1, 0), (0, 2, 1, 1), (0, 4, 7, 3), (0, 5, 4294967295, 4294967295), (0, 8, 1000, 1), (1, 0, 3, 2), (1, 1, 9, 0)):
        pdr[c][i] = [r, d]
    want = RL.pdr_text(names, refs, pdr)[len(RL.PDR_HEADER):]
    order = sorted(RL.pdr_rows(pdr), key=lambda t: (names[t[0]], t[1]))
    lines = ["pdr %s %d %s %d %d" % (names[c], i, refs[c][i], r, d) for c, i, r, d in order]
    assert formatted(harness, lines) == want and want.count("\n") == 7
    lines, want = ["pdr %s %d C 1 1" % (LONG, LAST)], ["%s\t%d\t+\t1\t1\t1.000\n" % (LONG, LAST + 1)]
    for _ in range(200):
        r = int(rng.integers(1, 500))
        d, pos, letter = int(rng.integers(0, r + 1)), int(rng.integers(0, LAST + 1)), "CG"[int(rng.integers(0, 2))]
        lines.append("pdr c %d %s %d %d" % (pos, letter, r, d))
        want.append("c\t%d\t%s\t%d\t%d\t%.3f\n" % (pos + 1, "+" if letter == "C" else "-", r, d, float(d) / r))
    assert formatted(harness, lines) == "".join(want)


def test_nothing_in_nothing_out_and_a_bad_line(harness):
    assert formatted(harness, []) == ""
    r = subprocess.run([harness], input=b"table9 chr1 1 2\n", capture_output=True, timeout=600)
    assert r.returncode == 2
