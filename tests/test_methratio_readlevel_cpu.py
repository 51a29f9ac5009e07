"""Per-read calls of bsmap_amd.methratio (--nonconv-filter, --read-stats, --pdr) without a GPU: the model of readlevel_model.py pinned to a worked example
that is written out literally here, the option parser, and the argument checks of the new C ABI entry points (a null handle needs no device)."""
import ctypes as C

import pytest

import readlevel_model as RL

BSX_ERR_ARG = -1

# One chromosome: CG at 2, 6, 10, 14, 18; non-CpG cytosines C at 22 (CHH), 26 and 33 (CHG), G at 28 and 35 (CHG)
REF = "ATCGATCGTTCGAACGTTCGATCATTCTGATTACAGTATT"
READS = [  # (strand code, letters), all at position 0, insert 0, no cut
    (0, "ATCGATCGTTCGAACGTTCGATTATTTTGATTATAGTATT"),   # 1  '++'  5, 5, 3, 0  eligible, concordant
    (0, "ATTGATTGTTTGAATGTTTGATTATTTTGATTATAGTATT"),   # 2  '++'  5, 0, 3, 0  eligible, concordant
    (0, "ATCGATTGTTCGAATGTTCGATTATTTTGATTATAGTATT"),   # 3  '++'  5, 3, 3, 0  eligible, discordant
    (0, "ATCGATCGTTCGAACGTTCGATCATTCTGATTACAGTATT"),   # 4  '++'  5, 5, 3, 3  dropped
    (1, "ATCGATCGTTCAAACGTTCGATCATTCTAATTACAATATT"),   # 5  '-+'  5, 4, 2, 0  eligible, discordant
    (0, "ATCGATTGTTCGA"),                              # 6  '++'  3, 2, 0, 0  not eligible
    (3, "ATCAATCATTCAAACATTCAATCATTCTAATTACAATATT"),   # 7  '--'  5, 0, 2, 0  eligible, concordant
]
ALNS = [(0, 0, st, 0, -1, s) for st, s in READS]
CG_C, CG_G = (2, 6, 10, 14, 18), (3, 7, 11, 15, 19)


def test_worked_example_contexts():
    assert [i for i in range(len(REF)) if REF[i:i + 2] == "CG"] == list(CG_C)
    assert [(i, RL.context_class(REF, i, True)) for i, x in enumerate(REF) if x == "C" and i not in CG_C] == [(22, 2), (26, 1), (33, 1)]
    assert [(i, RL.context_class(REF, i, False)) for i, x in enumerate(REF) if x == "G" and i not in CG_G] == [(28, 1), (35, 1)]


def test_worked_example_counts_and_verdicts():
    R = RL.analyse([REF], ALNS, trim_fillin=0, nonconv=3, min_cpg=4)
    assert R.counts == [(5, 5, 3, 0), (5, 0, 3, 0), (5, 3, 3, 0), (5, 5, 3, 3), (5, 4, 2, 0), (3, 2, 0, 0), (5, 0, 2, 0)]
    assert R.verdict == ["concordant", "concordant", "discordant", "dropped", "discordant", "plain", "concordant"]
    assert R.dropped == 1 and R.nmap == 6 and R.kept == [0, 1, 2, 4, 5, 6]


def test_worked_example_pdr_cells():
    R = RL.analyse([REF], ALNS, trim_fillin=0, nonconv=3, min_cpg=4)
    want = [[0, 0] for _ in REF]
    for i in CG_C:
        want[i] = [3, 1]
    for i in CG_G:
        want[i] = [2, 1]
    assert R.pdr == [want]
    assert RL.pdr_rows(R.pdr) == sorted([(0, i, 3, 1) for i in CG_C] + [(0, i, 2, 1) for i in CG_G])
    folded = RL.fold([REF], R.pdr)
    assert RL.pdr_rows(folded) == [(0, i, 5, 2) for i in CG_C]
    assert RL.pdr_rows(folded, 6) == [] and RL.pdr_rows(R.pdr, 3) == [(0, i, 3, 1) for i in CG_C]
    assert RL.pdr_rows(RL.analyse([REF], ALNS, trim_fillin=0, nonconv=3, min_cpg=6).pdr) == []           # K = 6: no read is eligible
    R0 = RL.analyse([REF], ALNS, trim_fillin=0, nonconv=0, min_cpg=4)                                       # N = 0: read 4 is eligible and concordant
    assert R0.verdict[3] == "concordant" and R0.dropped == 0 and R0.nmap == 7
    assert RL.pdr_rows(R0.pdr) == sorted([(0, i, 4, 1) for i in CG_C] + [(0, i, 2, 1) for i in CG_G])
    assert RL.pdr_rows(RL.analyse([REF], ALNS, trim_fillin=0, nonconv=3, min_cpg=0).pdr) == []           # K = 0: off


def test_worked_example_histogram():
    for n in (0, 1, 3):  # the histogram does not depend on the threshold
        R = RL.analyse([REF], ALNS, trim_fillin=0, nonconv=n, min_cpg=4)
        assert (R.reads, R.cg_over, R.ch_calls, R.ch_meth) == (7, 0, 16, 3)
        assert R.ch == [6, 0, 0, 1] + [0] * 60
        cells = {(a, b): v for a, row in enumerate(R.cg) for b, v in enumerate(row) if v}
        assert cells == {(5, 5): 2, (5, 0): 2, (5, 3): 1, (5, 4): 1, (3, 2): 1}


def test_worked_example_counters_after_the_filter():
    R = RL.analyse([REF], ALNS, trim_fillin=0, nonconv=3, min_cpg=4)
    assert [R.depth[0][i] for i in CG_C] == [4, 4, 4, 3, 3] and [R.meth[0][i] for i in CG_C] == [3, 1, 3, 1, 2]   # reads 1, 2, 3, 6 ('++', not dropped)
    assert [R.depth[0][i] for i in CG_G] == [2] * 5 and [R.meth[0][i] for i in CG_G] == [1, 1, 0, 1, 1]            # reads 5, 7
    assert [R.depth[0][i] for i in (22, 26, 33)] == [3, 3, 3] and [R.meth[0][i] for i in (22, 26, 33)] == [0, 0, 0]
    R0 = RL.analyse([REF], ALNS, trim_fillin=0)
    assert [R0.depth[0][i] for i in (22, 26, 33)] == [4, 4, 4] and [R0.meth[0][i] for i in (22, 26, 33)] == [1, 1, 1]
    assert R0.rev_ga[0][3] == 5 and R0.rev_g[0][3] == 5 and R.rev_ga[0][3] == 4                                     # '+' reads over the G of the first CG


PDR_TEXT = RL.PDR_HEADER + "".join("one\t%d\t%s\t%d\t1\t%s\n" % (i + 1, "+" if i in CG_C else "-", 3 if i in CG_C else 2, "0.333" if i in CG_C else "0.500")
                                   for i in sorted(CG_C + CG_G))
PDR_TEXT_FOLDED = RL.PDR_HEADER + "".join("one\t%d\t+\t5\t2\t0.400\n" % (i + 1) for i in CG_C)
STATS_TEXT = (RL.STATS_HEADER + "CG\t3\t2\t1\nCG\t5\t0\t2\nCG\t5\t3\t1\nCG\t5\t4\t1\nCG\t5\t5\t2\nCG\t>31\t.\t0\n" + "CH\t.\t0\t6\nCH\t.\t1\t0\nCH\t.\t2\t0\nCH\t.\t3\t1\n"
              + "".join("CH\t.\t%d\t0\n" % k for k in range(4, 63)) + "CH\t.\t63+\t0\n" + "# reads\t7\n# CH calls\t16\n# CH methylated\t3\n# CH ratio\t0.18750\n")


def test_worked_example_files():
    R = RL.analyse([REF], ALNS, trim_fillin=0, nonconv=3, min_cpg=4)
    assert RL.pdr_text(["one"], [REF], R.pdr) == PDR_TEXT
    assert RL.pdr_text(["one"], [REF], RL.fold([REF], R.pdr)) == PDR_TEXT_FOLDED
    assert RL.read_stats_text(R) == STATS_TEXT
    empty = RL.analyse([REF], [], trim_fillin=0)
    assert RL.read_stats_text(empty).endswith("# reads\t0\n# CH calls\t0\n# CH methylated\t0\n# CH ratio\tNA\n") and RL.pdr_text(["one"], [REF], empty.pdr) == RL.PDR_HEADER


def test_model_windows_and_masks():
    """what takes a read below K: a masked cycle, a cut, the fill-in trim; and the duplicate filter runs before the read is looked at"""
    read = READS[0][1][:16]   # CG calls at 2, 6, 10, 14
    K = lambda **kw: RL.analyse([REF], [(0, 0, 0, kw.pop("insert", 0), kw.pop("cut", -1), read)], **dict(dict(trim_fillin=0), **kw))
    assert K().counts == [(4, 4, 0, 0)] and K().verdict == ["concordant"]
    assert K(trim5=3).counts == [(3, 3, 0, 0)] and K(trim5=3).verdict == ["plain"]          # cycle 2 masked
    assert K(trim3=2).counts == [(3, 3, 0, 0)] and K(trim3=1).counts == [(4, 4, 0, 0)]      # cycle 14 masked
    assert K(cut=14, insert=30).counts == [(3, 3, 0, 0)] and K(cut=15, insert=30).counts == [(4, 4, 0, 0)]
    assert K(trim_fillin=2, insert=16).counts == [(3, 3, 0, 0)]                            # '++' loses its last two letters
    minus = (0, 0, 1, 0, -1, READS[4][1])   # '-+': cycle of letter j is n0 - 1 - j
    assert RL.analyse([REF], [minus], trim_fillin=0, trim3=4).counts == [(4, 3, 2, 0)]      # the methylated G at 3 is cycle 36 of 40: masked
    assert RL.analyse([REF], [minus], trim_fillin=0, trim3=3).counts == [(5, 4, 2, 0)]
    dup = [ALNS[3], ALNS[0]]                 # read 4 owns the fragment end, is dropped, and still suppresses read 1
    R = RL.analyse([REF], dup, trim_fillin=0, rm_dup=True, nonconv=3)
    assert R.verdict == ["dropped", "invalid"] and R.reads == 1 and R.nmap == 0 and RL.table_rows(R) == []
    assert RL.analyse([REF], [(0, 1, 0, 0, -1, REF)], trim_fillin=0).reads == 0             # one letter past the end: in nothing


def test_option_parser():
    from bsmap_amd import methratio
    ap = methratio.build_parser()
    base = ["-o", "t", "-d", "r.fa", "in.bsp"]
    o = ap.parse_args(base)
    assert (o.nonconv_filter, o.read_stats, o.pdr, o.pdr_min_cpg, o.pdr_min_reads) == (0, None, None, 4, 1)
    o = ap.parse_args(["--nonconv-filter", "3", "--read-stats", "s.txt", "--pdr", "p.txt", "--pdr-min-cpg", "5", "--pdr-min-reads", "10"] + base)
    assert (o.nonconv_filter, o.read_stats, o.pdr, o.pdr_min_cpg, o.pdr_min_reads) == (3, "s.txt", "p.txt", 5, 10)
    o = ap.parse_args(["--pdr", "p.txt"] + base)
    assert (o.pdr_min_cpg, o.pdr_min_reads) == (4, 1)
    for bad in (["--pdr-min-cpg", "4"], ["--pdr-min-reads", "1"], ["--pdr", "p", "--pdr-min-cpg", "0"], ["--pdr", "p", "--pdr-min-reads", "0"],
                ["--nonconv-filter", "-1"], ["--nonconv-filter", "x"], ["--pdr"], ["--read-stats"]):
        with pytest.raises(SystemExit):
            ap.parse_args(bad + base)


def test_run_rejects_before_it_touches_the_library():
    from bsmap_amd import methratio
    for kw in (dict(pdr_min_cpg=4), dict(pdr_min_reads=1), dict(pdr="p", pdr_min_cpg=0), dict(pdr="p", pdr_min_reads=0), dict(nonconv_filter=-1)):
        with pytest.raises(ValueError):
            methratio.run("no-such.fa", ["no-such.bsp"], "no-such.txt", **kw)


def test_null_handle_is_an_argument_error():
    """every new entry point, with a null handle and (where it has one) a null out pointer: BSX_ERR_ARG before any device call"""
    from bsmap_amd import methratio
    L = methratio._bind()
    buf = (C.c_uint64 * 1024)()
    p = C.addressof(buf)
    assert L.bsx_meth_set_nonconv(None, 3) == BSX_ERR_ARG
    assert L.bsx_meth_nonconv_dropped(None, p) == BSX_ERR_ARG
    assert L.bsx_meth_set_read_stats(None, 1) == BSX_ERR_ARG
    assert L.bsx_meth_read_stats_fetch(None, p, p, p) == BSX_ERR_ARG
    assert L.bsx_meth_write_read_stats(None, b"x") == BSX_ERR_ARG
    assert L.bsx_meth_set_pdr(None, 4) == BSX_ERR_ARG
    assert L.bsx_meth_pdr_report_chr(None, 0, 1, p) == BSX_ERR_ARG
    assert L.bsx_meth_pdr_fetch_rows(None, p, p, p) == BSX_ERR_ARG
    assert L.bsx_meth_write_pdr(None, b"x", 1, None) == BSX_ERR_ARG
    assert (methratio.RS_CG, methratio.RS_CH) == (RL.CG_MAX + 1, RL.CH_MAX + 1)
