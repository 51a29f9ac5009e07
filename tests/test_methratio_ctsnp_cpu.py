"""What the C/T-SNP correction (-i) and the context filter (-x) of bsmap_amd.methratio can be held to without a GPU: the model the GPU
tests compare against (ctsnp_model.py) on rows and a case written out by hand, the command line, and the signature of run()."""
import os
import re

import pytest

import bsmap_amd as B
import ctsnp_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the worked rows of the specification: dd, m, g, ga -> the columns from `ratio` on -------------------------------------
@pytest.mark.parametrize("counters,columns", [
    ((10, 8, 3, 6), "1.000 5.00 8 10 3 6 0.566 1.000"),   # the opposite strand halves the depth; min() caps the ratio
    ((7, 2, 2, 3), "0.429 4.67 2 7 2 3 0.127 0.795"),
    ((4, 1, 5, 5), "0.250 4.00 1 4 5 5 0.046 0.699"),     # no converted opposite-strand call: the plain ratio
    ((3, 0, 0, 0), "0.000 3.00 0 3 0 0 0.000 0.562"),     # no opposite-strand call at all
])
def test_worked_rows(counters, columns):
    assert M.row_fields(*counters, mode=1) == columns.replace(" ", "\t")
    assert M.row_fields(*counters, mode=2) == columns.replace(" ", "\t")


def test_row_rule_order():
    ref = "ACGTT"
    assert M.covered(ref, 1, 3, 0, 2, 1, 0, 0) and not M.covered(ref, 1, 3, 0, 2, 1, 1, 0) and not M.covered(ref, 1, 3, 0, 2, 1, 2, 0)
    assert M.covered(ref, 1, 3, 1, 2, 1, 1, 0) and not M.covered(ref, 1, 3, 1, 2, 1, 2, 0)
    assert M.covered(ref, 1, 0, 0, 0, 0, 0, 0) and not M.covered(ref, 1, 0, 0, 0, 0, 1, 0)   # depth 0 is never covered with the mode on
    assert M.covered(ref, 1, 3, 2, 2, 1, 2, 1) and not M.covered(ref, 1, 3, 2, 2, 1, 2, 6)   # position 1 is a CG
    assert M.covered(ref, 2, 3, 2, 2, 1, 0, 1) and M.covered(ref, 2, 3, 2, 2, 1, 0, 0xF) and not M.covered(ref, 2, 3, 2, 2, 4, 0, 0xF)


# ---- 2. a case by hand -----------------------------------------------------------------------------------------------------------
# position       0123456789..
HAND_REF = "ACGTCCGATCGA"
HAND_ALNS = [  # -t 0, no -r; the SNP is planted at position 4: the '-' read that spans it whole shows T over the C
    (0, 0, 0, 0, -1, "ATGTCTGATCGA"),   # '++'  C1 T, C4 C, C5 T, C9 C;   G2, G6, G10 show G
    (0, 0, 1, 0, -1, "ACATTCGATCAA"),   # '-+'  G2 A, G6 G, G10 A;        C1 C, C4 T (the SNP), C5 C, C9 C
    (0, 2, 2, 0, -1, "GTTCGATC"),       # '+-'  C4 T, C5 C, C9 C;         G2, G6 show G
    (0, 3, 3, 0, -1, "TCCGAT"),         # '--'  G6 G;                     C4 C, C5 C
    (0, 4, 0, 0, -1, "CTGAT"),          # '++'  C4 C, C5 T;               G6 shows G
]
HAND_DEPTH = [0, 1, 1, 0, 3, 3, 2, 0, 0, 2, 1, 0]
HAND_METH = [0, 0, 0, 0, 2, 1, 2, 0, 0, 2, 0, 0]
HAND_REV_G = [0, 1, 2, 0, 1, 2, 3, 0, 0, 1, 1, 0]
HAND_REV_GA = [0, 1, 2, 0, 2, 2, 3, 0, 0, 1, 1, 0]
HAND_ROWS = {  # by 1-based position; position 5 (depth 3, rev 1 of 2: eff 1.50 < 2 methylated) is the SNP
    2: "h\t2\t+\t\t0.000\t1.00\t0\t1\t1\t1\t0.000\t0.793\n",
    3: "h\t3\t-\tACGTC\t0.000\t1.00\t0\t1\t2\t2\t0.000\t0.793\n",
    5: "h\t5\t+\tGTCCG\t1.000\t1.50\t2\t3\t1\t2\t0.281\t1.000\n",
    6: "h\t6\t+\tTCCGA\t0.333\t3.00\t1\t3\t2\t2\t0.061\t0.792\n",
    7: "h\t7\t-\tCCGAT\t1.000\t2.00\t2\t2\t3\t3\t0.342\t1.000\n",
    10: "h\t10\t+\tATCGA\t1.000\t2.00\t2\t2\t1\t1\t0.342\t1.000\n",
    11: "h\t11\t-\tTCGA\t0.000\t1.00\t0\t1\t1\t1\t0.000\t0.793\n",
}


def test_hand_written_case():
    K = M.pileup([HAND_REF], HAND_ALNS, trim_fillin=0)
    assert K.nmap == 5 and sorted(a[2] for a in HAND_ALNS) == [0, 0, 1, 2, 3]
    assert (K.depth, K.meth, K.rev_g, K.rev_ga) == ([HAND_DEPTH], [HAND_METH], [HAND_REV_G], [HAND_REV_GA])
    text, nc, nd = M.table(["h"], K, 1, True, mode=1)
    assert text == M.HEADER12 + "".join(HAND_ROWS[p] for p in (2, 3, 5, 6, 7, 10, 11)) and (nc, nd) == (7, 13)
    text, nc, nd = M.table(["h"], K, 1, True, mode=2)
    assert text == M.HEADER12 + "".join(HAND_ROWS[p] for p in (2, 3, 6, 7, 10, 11)) and (nc, nd) == (6, 10)
    assert M.summary(5, 6, 10) == "total 5 valid mappings, 6 covered cytosines, average coverage: 1.67 fold.\n"
    # -z off drops the rows without a methylated call, not what counts as covered
    text, nc, nd = M.table(["h"], K, 1, False, mode=1)
    assert text == M.HEADER12 + "".join(HAND_ROWS[p] for p in (5, 6, 7, 10)) and (nc, nd) == (7, 13)
    # the fold: G3 onto C2, G7 onto C6, G11 onto C10
    F = M.combine_cpg(K)
    assert F.depth == [[0, 2, 0, 0, 3, 5, 0, 0, 0, 3, 0, 0]] and F.rev_g == [[0, 3, 0, 0, 1, 5, 0, 0, 0, 2, 0, 0]] and F.rev_ga == [[0, 3, 0, 0, 2, 5, 0, 0, 0, 2, 0, 0]]
    assert K.depth == [HAND_DEPTH]   # a copy was folded


# ---- 3. the command line ---------------------------------------------------------------------------------------------------------------
BASE = ["-o", "t.txt", "-d", "g.fa"]


def test_build_parser_takes_the_options():
    from bsmap_amd import methratio
    ap = methratio.build_parser()
    o = ap.parse_args(BASE + ["a.bsp"])
    assert o.ct_snp == "no-action" and o.context is None
    assert ap.parse_args(BASE + ["-i", "correct", "a.bsp"]).ct_snp == "correct"
    assert ap.parse_args(BASE + ["--ct-snp=skip", "a.bsp"]).ct_snp == "skip"
    assert ap.parse_args(BASE + ["-i", "no-action", "a.bsp"]).ct_snp == "no-action"
    assert ap.parse_args(BASE + ["-x", "CG,CHH", "a.bsp"]).context == ["CG", "CHH"]
    assert ap.parse_args(BASE + ["--context", "CHG", "a.bsp"]).context == ["CHG"]


@pytest.mark.parametrize("bad", [["-i", "fix"], ["-x", "CGG"], ["-x", ""], ["-x", "cg"], ["-x", "CG,"], ["-i", "Correct"]])
def test_build_parser_rejects(bad, capsys):
    from bsmap_amd import methratio
    with pytest.raises(SystemExit) as e:
        methratio.build_parser().parse_args(BASE + bad + ["a.bsp"])
    assert e.value.code == 2 and bad[0] in capsys.readouterr().err


def test_main_hands_the_options_to_run(monkeypatch):
    from bsmap_amd import methratio
    seen = {}
    monkeypatch.setattr(methratio, "run", lambda reffile, infiles, outfile, **kw: seen.update(kw) or "")
    methratio.main(BASE + ["-i", "skip", "-x", "CHG,CG", "a.sam"])
    assert (seen["ct_snp"], seen["context"]) == ("skip", ["CHG", "CG"])
    methratio.main(BASE + ["a.sam"])
    assert (seen["ct_snp"], seen["context"]) == ("no-action", None)


# ---- 4. run() -----------------------------------------------------------------------------------------------------------------------------
def test_run_signature_and_no_device_error(tmp_path):
    import inspect
    from bsmap_amd import methratio
    p = inspect.signature(methratio.run).parameters
    assert (p["ct_snp"].default, p["context"].default) == ("no-action", None)
    B.build()
    fa = tmp_path / "g.fa"
    fa.write_text(">h\n" + HAND_REF + "\n")
    if B.lib().bsx_device_count() > 0:  # with a device the call goes through: an empty mapping file, the 12-column header only
        bsp = tmp_path / "e.bsp"
        bsp.write_text("")
        assert methratio.run(str(fa), [str(bsp)], str(tmp_path / "t.txt"), ct_snp="correct", context=["CG"]).startswith("total 0 valid mappings")
        assert (tmp_path / "t.txt").read_text() == M.HEADER12
    else:
        with pytest.raises(B.BsxError) as e:
            methratio.run(str(fa), [str(tmp_path / "none.bsp")], str(tmp_path / "t.txt"), ct_snp="correct", context=["CG"])
        assert "no HIP device" in str(e.value)
    with pytest.raises(ValueError):
        methratio.run(str(fa), [], str(tmp_path / "t.txt"), ct_snp="fix")


@pytest.mark.parametrize("name", ["bsx_meth_set_ct_snp", "bsx_meth_set_contexts", "bsx_meth_fetch_rows_snp"])
def test_declared_exported_and_bound(name):
    from bsmap_amd import methratio
    B.build()
    header = open(os.path.join(ROOT, "include", "bsx.h")).read()
    assert re.search(r"\bint\s+%s\s*\(\s*bsx_meth\s*\*" % name, header), f"{name} is not declared in include/bsx.h"
    assert name in B.EXPORTS and hasattr(B.lib(), name)
    assert getattr(methratio._bind(), name).argtypes
