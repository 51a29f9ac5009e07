"""q-values over all rows and de novo DMRs of the two-sample report without a GPU: the numpy model of Benjamini-Hochberg on cases known in
closed form, the run model on hand-written row lists, the new formatters, the host form of the delta rule and the run filter of
bsmap_amd/csrc/bsx_meth_diff.h under AddressSanitizer + UndefinedBehaviorSanitizer through tests/harness/fdr_check.cpp, the option parser, and the argument
checks of the new C ABI entry points (a null handle needs no device)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import diff_model as D
import fdr_model as F
from conftest import HOST_SAN_FLAGS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BSX_ERR_ARG = -1
A_ROW, B_ROW, NEUTRAL, WEAK = (8, 8, 0, 8), (0, 8, 8, 8), (4, 8, 4, 8), (12, 40, 30, 40)   # A higher (sign -1), B higher (+1), equal, delta 0.45 towards B


# ---- the q model ----
def bits(x):
    return np.asarray(x, np.float64).view(np.uint64).tolist()


def test_bh_closed_forms():
    assert F.bh([]).shape == (0,)
    for p in (0.0, 0.3, 1.0, 5e-324):
        assert bits(F.bh([p])) == bits([p])                       # n = 1: q = p
    for p in (0.0, 0.25, 0.5, 1.0):                               # (values whose product with 7 is exact)
        assert bits(F.bh([p] * 7)) == bits([p] * 7)               # all equal: the last of the tie block has r = p n / n
    # five values by hand: r = .05, .05, .035, .0275, .9; the suffix minimum makes the first four .0275
    got = F.bh([0.021, 0.9, 0.01, 0.022, 0.02])
    small = (0.022 * 5.0) / 4.0
    assert bits(got) == bits([small, (0.9 * 5.0) / 5.0, small, small, small])
    assert bits(F.bh([0.5, 0.9])) == bits([0.9, 0.9]) and bits(F.bh([0.6, 0.9])) == bits([0.9, 0.9])   # 0.6 * 2 = 1.2, the suffix minimum 0.9 is below it
    assert bits(F.bh([0.6, 1.0])) == bits([1.0, 1.0])             # clipped at 1


def test_bh_properties():
    rng = np.random.default_rng(5)
    p = rng.choice(np.append(rng.random(20), [0.0, 1.0, 5e-324]), 500)
    p[rng.random(500) < 0.1] = np.nan
    q = F.bh(p)
    inside = ~np.isnan(p)
    assert np.array_equal(np.isnan(q), ~inside) and 0 < (~inside).sum() < 500
    assert np.all(q[inside] >= p[inside]) and np.all(q[inside] <= 1.0)
    order = np.argsort(p[inside], kind="stable")
    assert np.all(np.diff(q[inside][order]) >= 0)                 # monotone in p
    for v in np.unique(p[inside]):
        assert len(set(bits(q[p == v]))) == 1                     # equal p, equal q
    assert bits(F.bh(p[inside])) == bits(q[inside])               # a NaN does not count in n


# ---- the run model on hand-written rows ----
def rows_of(*sites):
    """sites: (sequence, pos, counts); q = 0.001 for every site but the NEUTRAL ones, 1.0 for those"""
    return [(s, x) + c for s, x, c in sites], [1.0 if c == NEUTRAL else 0.001 for _, _, c in sites]


def model(sites, max_q=0.01, permille=500, max_gap=30, min_sites=3):
    rows, q = rows_of(*sites)
    return F.dmrs(rows, q, max_q, permille, max_gap, min_sites)


def test_dmr_model_directed():
    a = lambda s, *xs: [(s, x, A_ROW) for x in xs]
    b = lambda s, *xs: [(s, x, B_ROW) for x in xs]
    assert F.sign(*A_ROW) == -1 and F.sign(*B_ROW) == 1 and F.sign(*NEUTRAL) == 0 and F.sign(*WEAK) == 1 and F.sign(1, 2, 2, 4) == 0
    assert model(a(0, 0, 10, 40)) == [(0, 0, 41, 3)]                                              # a gap of exactly max_gap joins
    assert model(a(0, 0, 10, 20, 51, 61, 71)) == [(0, 0, 21, 3), (0, 51, 72, 3)]                  # max_gap + 1 splits
    assert model(a(0, 0, 10, 20) + b(0, 30, 40, 50)) == [(0, 0, 21, 3), (0, 30, 51, 3)]           # a sign flip inside a gap splits
    assert model(a(0, 40, 50, 60) + a(1, 70, 80, 90)) == [(0, 40, 61, 3), (1, 70, 91, 3)]         # another sequence splits, whatever the positions
    assert model(a(0, 0, 10) + [(0, 20, NEUTRAL)] + a(0, 30)) == [(0, 0, 31, 3)]                  # a common site that is no candidate breaks nothing
    assert model(a(0, 0, 10)) == [] and model(a(0, 0, 10), min_sites=1) == [(0, 0, 11, 2)]        # a run below min_sites is dropped
    assert model(a(0, 0, 10, 20), max_q=0.0001) == [] and model([]) == []                         # no candidate, no run
    weak = [(0, x, WEAK) for x in (0, 10, 20)]
    assert model(weak) == [] and model(weak, permille=450) == [(0, 0, 21, 3)] and model(weak, permille=451) == []   # the delta rule, at its limit
    assert model([(0, 0, (1, 2, 2, 4)), (0, 10, (3, 6, 1, 2)), (0, 20, (5, 10, 1, 2))], permille=0) == []            # equal ratios: sign 0, never a candidate
    runs = F.candidate_runs(*rows_of(*(a(0, 0, 10) + [(0, 20, NEUTRAL)] + a(0, 30) + b(0, 40))), 0.01, 500, 30)
    assert runs == [[0, 1, 3], [4]]


# ---- the header, compiled on its own under the host sanitizers ----
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fdr") / "fdr_check")
    subprocess.run(["g++"] + HOST_SAN_FLAGS + ["-o", exe, os.path.join(ROOT, "tests", "harness", "fdr_check.cpp")], check=True)   # (ASan + UBSan: conftest.py)
    return exe


def ask(exe, lines):
    r = subprocess.run([exe], input="".join(x + "\n" for x in lines).encode(), capture_output=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr.decode(errors="replace")[-3000:])
    return r.stdout.decode()


def test_formatters_equal_python_formatting(harness):
    nan = float("nan")
    qs = [1.0, 0.05, 3.3e-4, 0.0, 5e-324, 0.99995, nan, 9.99995e-100]
    quads = [(0, 1, 0, 1), (1, 2, 3, 4), (8, 8, 0, 8), (4000, 4000, 0, 2500), (1, 3, 2, 3), (4294967295, 4294967295, 1, 4294967295), (2, 3, 2, 3), (1, 8, 1, 9)]
    lines, want = [], ""
    for k, (quad, q) in enumerate(zip(quads, qs)):
        p = min(1.0, 0.5 ** k)
        lines.append("posq chr%d %d %d %d %d %d %d %s %s" % (k, k * 1000003, k % 8, *quad, p.hex(), "nan" if q != q else q.hex()))
        want += F.with_q(D.pos_row_text("chr%d" % k, k * 1000003, "G" if k % 8 >= 4 else "C", k % 4, quad, p), q)
    big = (2 ** 40, 2 ** 50, 2 ** 51 + 1, 2 ** 52 - 1, 2 ** 52)
    for k, (sums, p, q) in enumerate([((3, 1, 6, 5, 9), 0.25, 0.5), (big, 1e-300, 2e-300), ((0, 0, 0, 0, 0), nan, nan), ((1, 1, 1, 0, 1), 1.0, 1.0)]):
        txt = lambda x: "nan" if x != x else x.hex()
        lines.append("regq a_long_sequence_name.1 %d %d label%d %d %d %d %d %d %s %s" % (k, 4294967295 - k, k, *sums, txt(p), txt(q)))
        want += F.with_q(D.interval_row_text("a_long_sequence_name.1", k, 4294967295 - k, "label%d" % k, sums, p), q)
        if sums[0]:
            lines.append("dmr x %d %d %d %d %d %d %d %d %s" % (k * 100, k * 100 + 77, k + 1, *sums, txt(p)))
            want += F.dmr_row_text("x", k * 100, k * 100 + 77, k + 1, sums, p)
    got = ask(harness, lines)
    assert got == want
    assert "chr2\t2000007\t+\tCHH\t8\t8\t1.000\t0\t8\t0.000\t-1.000\t2.5000e-01\t3.3000e-04\n" in got
    assert "a_long_sequence_name.1\t2\t4294967293\tlabel2\t0\t0\t0\tNA\t0\t0\tNA\tNA\tNA\tNA\n" in got and got.count("\tNA\n") == 2
    assert "x\t0\t77\t1\t3\t1\t6\t0.167\t5\t9\t0.556\t+0.389\t2.5000e-01\n" in got


def test_headers_agree(harness):
    assert ask(harness, ["hdr"]) == F.POS_FDR_HEADER + F.REGION_FDR_HEADER + F.DMR_HEADER
    assert F.POS_FDR_HEADER.split("\t")[:12] == D.POS_HEADER[:-1].split("\t") and F.POS_FDR_HEADER.endswith("\tp\tq\n")
    assert F.DMR_HEADER == "chr\tstart\tend\tn_sig\t" + D.BIN_HEADER.split("\t", 3)[3]


def test_host_delta_rule_and_run_filter(harness):
    cases = [(250, 1, 2, 3, 4), (251, 1, 2, 3, 4), (0, 1, 2, 1, 2), (1, 1, 2, 1, 2), (1000, 0, 7, 7, 7), (1000, 1, 7, 7, 7), (450, *WEAK), (451, *WEAK), (500, *A_ROW),
             (999, 4294967295, 4294967295, 1, 4294967295), (1000, 4294967295, 4294967295, 0, 4294967295), (1, 4294967294, 4294967295, 4294967295, 4294967295),
             (0, 3, 6, 30, 60), (1000, 0, 4294967295, 4294967295, 4294967295)]
    got = ask(harness, ["keep %d %d %d %d %d" % c for c in cases]).split("\n")[:-1]
    assert got == ["%d %d" % (D.delta_keeps(*c[1:], c[0]), F.sign(*c[1:])) for c in cases]
    assert got[0] == "1 1" and got[1] == "0 1" and got[8] == "1 -1" and got[12] == "1 0"
    runs = [(2, 0, 21, 3), (2, 100, 111, 2), (0, 5, 6, 1), (0, 50, 500, 40), (1, 7, 30, 3)]
    flat = " ".join("%d %d %d %d" % r for r in runs)
    text = lambda kept: "".join("%d %d %d %d\n" % r for r in kept) + "-\n"
    for k in (1, 2, 3, 4, 41):
        assert ask(harness, ["runs %d %d %s" % (k, len(runs), flat)]) == text([r for r in runs if r[3] >= k])
    assert ask(harness, ["runs 3 0"]) == "-\n"


# ---- the option surface ----
BASE = ["-o", "t", "-d", "r.fa", "--a", "a.sam", "--b", "b.sam"]


def test_option_parser():
    from bsmap_amd import methdiff
    ap = methdiff.build_parser()
    o = ap.parse_args(BASE)
    assert (o.fdr, o.max_q, o.dmr_out, o.dmr_max_q, o.dmr_max_gap, o.dmr_min_sites) == (False, None, None, None, None, None)
    assert ap.parse_args(BASE + ["--fdr"]).fdr is True
    o = ap.parse_args(BASE + ["--max-q", "0.05"])
    assert o.fdr is True and o.max_q == 0.05                       # --max-q implies --fdr
    o = ap.parse_args(BASE + ["--dmr-out", "d.txt"])
    assert (o.fdr, o.dmr_out, o.dmr_max_q, o.dmr_max_gap, o.dmr_min_sites) == (False, "d.txt", None, None, None)   # run() fills 0.05, 300 and 3 in
    o = ap.parse_args(BASE + ["--dmr-out", "d.txt", "--dmr-max-q", "0.1", "--dmr-max-gap", "0", "--dmr-min-sites", "1", "--min-delta", "0.2"])
    assert (o.dmr_max_q, o.dmr_max_gap, o.dmr_min_sites, o.min_delta) == (0.1, 0, 1, 0.2)
    for bad in (["--dmr-max-q", "0.1"], ["--dmr-max-gap", "100"], ["--dmr-min-sites", "2"], ["--max-q", "1.5"], ["--max-q", "-0.1"], ["--max-q", "x"],
                ["--dmr-out", "d", "--dmr-max-q", "2"], ["--dmr-out", "d", "--dmr-max-gap", "-1"], ["--dmr-out", "d", "--dmr-min-sites", "0"], ["--dmr-out"]):
        with pytest.raises(SystemExit):
            ap.parse_args(BASE + bad)


def test_run_rejects_before_it_touches_the_library():
    from bsmap_amd import methdiff
    for kw in (dict(max_q=1.5), dict(max_q=-0.1), dict(max_q=float("nan")), dict(dmr_max_q=0.1), dict(dmr_max_gap=100), dict(dmr_min_sites=2),
               dict(dmr_out="d", dmr_max_q=1.5), dict(dmr_out="d", dmr_max_q=float("nan")), dict(dmr_out="d", dmr_max_gap=-1), dict(dmr_out="d", dmr_min_sites=0),
               dict(dmr_out="d", dmr_max_gap=2 ** 32), dict(max_q="0.05"), dict(dmr_out="d", dmr_max_q="0.05"), dict(dmr_out="d", dmr_max_gap="300"),
               dict(dmr_out="d", dmr_min_sites="3"), dict(dmr_out="d", dmr_max_gap=1.5)):   # a value of another type is a ValueError too
        with pytest.raises(ValueError):
            methdiff.run("no-such.fa", ["no-such.sam"], ["no-such.sam"], "no-such.txt", **kw)


def test_null_handles_and_null_counts_are_argument_errors():
    """every new entry point with a null handle in either place, and with a null place for its count: BSX_ERR_ARG before any device call"""
    from bsmap_amd import methratio
    L = methratio._bind()
    buf = (C.c_uint64 * 64)()
    p, some = C.addressof(buf), C.c_void_p(C.addressof(buf))   # `some` stands for a handle: the null one is tested first
    q05 = C.byref(C.c_double(0.05))
    for a, b in ((None, None), (None, some), (some, None)):
        assert L.bsx_meth_diff_report_all(a, b, 1, p) == BSX_ERR_ARG
        assert L.bsx_meth_diff_dmrs(a, b, 1, q05, 0, 300, 3, p) == BSX_ERR_ARG
        assert L.bsx_meth_write_diff_fdr(a, b, b"x", 1, 0, None, None, p) == BSX_ERR_ARG
        assert L.bsx_meth_write_diff_regions_fdr(a, b, b"x.bed", b"x", 1, None, None) == BSX_ERR_ARG
        assert L.bsx_meth_write_dmrs(a, b, b"x", 1, q05, 0, 300, 3, p) == BSX_ERR_ARG
    assert L.bsx_meth_diff_fetch_all(None, p, p, p, p, p, p) == BSX_ERR_ARG
    assert L.bsx_meth_diff_fetch_dmrs(None, p, p, p, p, p, p) == BSX_ERR_ARG
    assert L.bsx_meth_bh(0, None, 1, p) == BSX_ERR_ARG and L.bsx_meth_bh(0, p, 1, None) == BSX_ERR_ARG
    # a null place for the count, ahead of any look at the handles
    assert L.bsx_meth_diff_report_all(some, some, 1, None) == BSX_ERR_ARG
    assert L.bsx_meth_diff_dmrs(some, some, 1, q05, 0, 300, 3, None) == BSX_ERR_ARG
    assert L.bsx_meth_write_diff_fdr(some, some, b"x", 1, 0, None, None, None) == BSX_ERR_ARG
    assert L.bsx_meth_write_dmrs(some, some, b"x", 1, q05, 0, 300, 3, None) == BSX_ERR_ARG
    assert L.bsx_meth_diff_dmrs(some, some, 1, None, 0, 300, 3, p) == BSX_ERR_ARG
    assert L.bsx_meth_bh(0, None, 0, None) == 0                # nothing to do, and no device asked for
    assert not os.path.exists("x")
