"""Two-sample differential methylation (bsmap_amd.methdiff) without a GPU: the exact model of diff_model.py on cases that are known in closed
form, the Fisher test and the row formatters of bsmap_amd/csrc/bsx_meth_diff.h — the text the kernel k_meth_fisher compiles — under AddressSanitizer +
UndefinedBehaviorSanitizer through tests/harness/diff_check.cpp against that model, the option parser, and the argument checks of the new C ABI entry
points (a null handle needs no device).

The tolerance is derived, not measured: rtol = 64 (s + 16) 2^-53 for a support of s tables (diff_model.rtol says why), for an exact p of 1e-290 or more; below
that the result must lie in [0, 1e-289].  A case is left out of the comparison if some w(x) / w(mA) lies within 1e-8 of the selection limit 1 + 1e-7 without
being equal to it; at most 1 % of the cases may be left out."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import pytest

import diff_model as D
from conftest import HOST_SAN_FLAGS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BSX_ERR_ARG = -1


# ---- the model ----
def test_model_closed_forms():
    assert D.fisher(3, 3, 0, 3) == Fraction(1, 10)                 # [[3, 0], [0, 3]]: two of the twenty tables
    for m, d in ((0, 1), (1, 1), (3, 7), (5, 10), (0, 40), (17, 300)):
        assert D.fisher(m, d, m, d) == 1
    for quad in ((0, 5, 0, 9), (4, 4, 6, 6), (0, 1, 0, 1)):         # one table in the support
        assert D.support(*quad)[0] == D.support(*quad)[1] and D.fisher(*quad) == 1
    assert D.fisher(5, 10, 5, 10) == 1
    assert D.fisher(2, 10, 8, 10) == D.fisher(8, 10, 2, 10) == Fraction(2 * (1 + 100 + 45 * 45), sum(D.weights(2, 10, 8, 10)))   # both tails: x = 0, 1, 2 and 8, 9, 10
    assert D.fisher(1, 1, 0, 1) == 1 and D.fisher(3, 6, 30, 60) == 1


def test_model_case_set_and_filters():
    cases = D.cases()
    assert len(cases) == 3006 and len(set(cases[-14:])) == 14 and all(0 <= mA <= dA and 0 <= mB <= dB for mA, dA, mB, dB in cases)
    assert max(hi - lo + 1 for lo, hi in (D.support(*q) for q in cases)) == 2501
    assert D.delta_keeps(1, 2, 3, 4, 250) and not D.delta_keeps(1, 2, 3, 4, 251) and D.delta_keeps(1, 2, 1, 2, 0) and not D.delta_keeps(1, 2, 1, 2, 1)
    assert D.delta_keeps(0, 7, 7, 7, 1000) and not D.delta_keeps(1, 7, 7, 7, 1000)
    assert not D.near_boundary(5, 10, 5, 10) and not D.near_boundary(2, 10, 8, 10)
    assert D.rtol(0, 4000, 2500, 2500) == Fraction(64 * (2501 + 16), 2 ** 53)
    assert D.p_error(0.1, (3, 3, 0, 3)) is None and D.p_error(0.1000001, (3, 3, 0, 3)) is not None and D.p_error(float("nan"), (3, 3, 0, 3)) is not None
    assert D.p_error(0.0, (0, 4000, 2500, 2500)) is None and D.p_error(1e-280, (0, 4000, 2500, 2500)) is not None
    assert [D.context_class("ACGTCAGCATCNC", i) for i in (1, 2, 4, 6, 7, 10, 12)] == [0, 0, 1, 1, 2, 3, 3]   # the G at 6 looks left: A, then C


# ---- the header, compiled on its own under the host sanitizers ----
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("diff") / "diff_check")
    subprocess.run(["g++"] + HOST_SAN_FLAGS + ["-o", exe, os.path.join(ROOT, "tests", "harness", "diff_check.cpp")], check=True)   # (ASan + UBSan: conftest.py)
    return exe


def ask(exe, lines):
    r = subprocess.run([exe], input="".join(x + "\n" for x in lines).encode(), capture_output=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr.decode(errors="replace")[-3000:])
    return r.stdout.decode()


def test_fisher_keeps_the_bound_over_the_case_set(harness):
    cases = D.cases()
    got = [float.fromhex(x) for x in ask(harness, ["q %d %d %d %d" % q for q in cases]).split()]
    assert len(got) == len(cases)
    left_out = [q for q in cases if D.near_boundary(*q)]
    assert len(left_out) * 100 <= len(cases)
    errors = [e for e in (D.p_error(p, q) for p, q in zip(got, cases) if q not in left_out) if e]
    assert not errors, errors[:10]
    by_case = dict(zip(cases, got))
    assert by_case[(3, 3, 0, 3)] == pytest.approx(0.1, rel=1e-14) and by_case[(0, 1, 0, 1)] == 1.0 and by_case[(5, 10, 5, 10)] == 1.0
    assert by_case[(2, 10, 8, 10)] == float.fromhex(ask(harness, ["q 8 10 2 10"]).strip())
    assert all(by_case[q] == 1.0 for q in cases if D.support(*q)[0] == D.support(*q)[1])   # a support of one table: exactly 1


def test_formatters_equal_python_formatting(harness):
    ps = [1.0, 0.1, 0.05, 1.05e-306, 0.0, 4.9e-324, 0.999949999, 1.23456789e-5, 9.99995e-100]
    quads = [(0, 1, 0, 1), (1, 2, 3, 4), (3, 4, 1, 2), (5, 10, 5, 10), (4000, 4000, 0, 2500), (1, 3, 2, 3), (4294967295, 4294967295, 1, 4294967295), (1, 8, 1, 9), (2, 3, 2, 3)]
    lines, want = [], ""
    for k, (q, p) in enumerate(zip(quads, ps)):
        lines.append("pos chr%d %d %d %d %d %d %d %s" % (k, k * 1000003, k % 8, *q, p.hex()))
        want += D.pos_row_text("chr%d" % k, k * 1000003, "G" if k % 8 >= 4 else "C", k % 4, q, p)
    big = (2 ** 40, 2 ** 50, 2 ** 51 + 1, 2 ** 52 - 1, 2 ** 52)
    for k, (sums, p) in enumerate([((3, 1, 6, 5, 9), 0.25), (big, 1e-300), ((0, 0, 0, 0, 0), float("nan")), ((1, 1, 1, 0, 1), 1.0)]):
        ptxt = "nan" if p != p else p.hex()
        lines.append("reg a_long_sequence_name.1 %d %d label%d %d %d %d %d %d %s" % (k, 4294967295 - k, k, *sums, ptxt))
        want += D.interval_row_text("a_long_sequence_name.1", k, 4294967295 - k, "label%d" % k, sums, p)
        lines.append("bin x %d %d %d %d %d %d %d %s" % (k * 100, k * 100 + 100, *sums, ptxt))
        want += D.interval_row_text("x", k * 100, k * 100 + 100, None, sums, p)
    got = ask(harness, lines)
    assert got == want
    assert got.split("\n")[1] == "chr1\t1000004\t+\tCHG\t1\t2\t0.500\t3\t4\t0.750\t+0.250\t1.0000e-01"
    assert got.split("\n")[2] == "chr2\t2000007\t+\tCHH\t3\t4\t0.750\t1\t2\t0.500\t-0.250\t5.0000e-02"
    assert "a_long_sequence_name.1\t2\t4294967293\tlabel2\t0\t0\t0\tNA\t0\t0\tNA\tNA\tNA\n" in got and "x\t200\t300\t0\t0\t0\tNA\t0\t0\tNA\tNA\tNA\n" in got
    assert ask(harness, []) == ""


def test_headers_agree():
    hdr = open(os.path.join(ROOT, "bsmap_amd", "csrc", "bsx_meth_diff.h")).read()
    for text in (D.POS_HEADER, D.REGION_HEADER, D.BIN_HEADER):
        assert '"%s"' % text.replace("\t", "\\t").replace("\n", "\\n") in hdr


# ---- the option surface ----
BASE = ["-o", "t", "-d", "r.fa", "--a", "a1.sam", "a2.bam", "--b", "b.sam"]


def test_option_parser():
    from bsmap_amd import methdiff
    ap = methdiff.build_parser()
    o = ap.parse_args(BASE)
    assert (o.a_files, o.b_files, o.min_delta, o.max_p, o.regions, o.bin, o.min_depth) == (["a1.sam", "a2.bam"], ["b.sam"], 0.0, None, None, None, 1)
    o = ap.parse_args(BASE + ["--min-delta", "0.25", "--max-p", "0.01", "--regions", "r.bed", "--region-out", "r.txt", "--bin", "100", "--bin-out", "b.txt", "-g", "-m", "3",
                              "-x", "CG", "--trim-5p", "2", "--nonconv-filter", "3", "-r", "-u", "-p", "-t", "0", "-c", "one,two", "-G", "1"])
    assert (o.min_delta, o.max_p, o.regions, o.region_out, o.bin, o.bin_out) == (0.25, 0.01, "r.bed", "r.txt", 100, "b.txt")
    assert (o.combine_CpG, o.min_depth, o.context, o.trim5, o.trim3, o.nonconv_filter, o.rm_dup, o.unique, o.pair, o.trim_fillin, o.chroms, o.device) == \
        (True, 3, ["CG"], 2, 0, 3, True, True, True, 0, "one,two", 1)
    for bad in (["--min-delta", "1.5"], ["--min-delta", "-0.1"], ["--min-delta", "x"], ["--max-p", "2"], ["--regions", "r.bed"], ["--region-out", "r.txt"], ["--bin", "0"],
                ["--bin", "10"], ["--bin-out", "b.txt"], ["-i", "correct"], ["-m", "-1"], ["-x", "CC"]):
        with pytest.raises(SystemExit):
            ap.parse_args(BASE + bad)
    for missing in ("--a", "--b", "-o", "-d"):
        k = BASE.index(missing)
        with pytest.raises(SystemExit):
            ap.parse_args(BASE[:k] + BASE[k + (3 if missing == "--a" else 2):])


def test_run_rejects_before_it_touches_the_library():
    from bsmap_amd import methdiff
    for kw in (dict(min_delta=1.5), dict(min_delta=-0.001), dict(min_delta=float("nan")), dict(max_p=1.5), dict(regions="r.bed"), dict(region_out="r.txt"), dict(bin=0, bin_out="b"),
               dict(bin=10), dict(bin_out="b"), dict(context=[]), dict(context=["CC"]), dict(nonconv_filter=-1)):
        with pytest.raises(ValueError):
            methdiff.run("no-such.fa", ["no-such.sam"], ["no-such.sam"], "no-such.txt", **kw)
    for a, b in (([], ["x"]), (["x"], [])):
        with pytest.raises(ValueError):
            methdiff.run("no-such.fa", a, b, "no-such.txt")


def test_null_handles_are_argument_errors():
    """every new entry point with a null handle in either place: BSX_ERR_ARG before any device call"""
    from bsmap_amd import methratio
    L = methratio._bind()
    buf = (C.c_uint64 * 64)()
    p, some = C.addressof(buf), C.c_void_p(C.addressof(buf))   # `some` stands for a handle: the null one is tested first
    for a, b in ((None, None), (None, some), (some, None)):
        assert L.bsx_meth_diff_report_chr(a, b, 0, 1, 0, p) == BSX_ERR_ARG
        assert L.bsx_meth_write_diff(a, b, b"x", 1, 0, None, None) == BSX_ERR_ARG
        assert L.bsx_meth_diff_regions(a, b, 1, p, p, p, 1, p, p) == BSX_ERR_ARG
        assert L.bsx_meth_write_diff_regions(a, b, b"x.bed", b"x", 1, None, None) == BSX_ERR_ARG
        assert L.bsx_meth_write_diff_bins(a, b, b"x", 100, 1, None) == BSX_ERR_ARG
    assert L.bsx_meth_diff_fetch_rows(None, p, p, p) == BSX_ERR_ARG
    assert not os.path.exists("x")
