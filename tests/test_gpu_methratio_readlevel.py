"""Per-read calls of bsmap_amd.methratio on the GPU (k_meth_reads: non-conversion filter, read histogram, PDR; bsx_meth_set_nonconv / _set_read_stats /
_set_pdr and their fetch / write calls; --nonconv-filter, --read-stats, --pdr) against the pure-Python model of readlevel_model.py, which never looks at
the library's output.  Every expectation is formed from the model before the library is touched."""
import ctypes as C
import gzip
import json
import os

import numpy as np
import pytest

import golden_util as G
import meth_util as U
import readlevel_model as RL
from test_methratio_readlevel_cpu import ALNS as EX_ALNS, PDR_TEXT, PDR_TEXT_FOLDED, REF as EX_REF, STATS_TEXT, CG_C, CG_G

pytestmark = pytest.mark.gpu
STRANDS = RL.STRANDS
BSX_ERR_ARG, BSX_ERR_STATE = -1, -5


# ---- the library through bsmap_amd.methratio.Meth ---------------------------------------------------------------------------
def handle(fa, rm_dup=False, nonconv=0, stats=True, min_cpg=4, snp=0, mbias=False, trim=None):
    return U.open_meth(fa, rm_dup, snp, mbias, trim, nonconv, stats, min_cpg)


def written_pdr(h, path, min_reads=1):
    n = h.write_pdr(path, min_reads)
    return U.read_text(path), n


def written_stats(h, path):
    h.write_read_stats(path)
    return U.read_text(path)


def model_hist(R):
    return R.cg, R.ch, (R.reads, R.cg_over, R.ch_calls, R.ch_meth)


def model_rows_snp1(R):
    """the rows of the C/T-SNP mode 1 with min_depth 1 and meth0 (depth > 0 and not rev_g == 0 < rev_ga), and their rev cells"""
    keep = [(c, i, d, m) for c, i, d, m in RL.table_rows(R) if not (R.rev_g[c][i] == 0 and R.rev_ga[c][i] > 0)]
    return keep, [(c, i, R.rev_g[c][i], R.rev_ga[c][i]) for c, i, _, _ in keep]


def compare(h, R, refs, snp=0, mbias=False):
    """everything a handle holds against the model's result, before and after the CpG fold"""
    n = len(refs)
    assert h.nonconv_dropped() == R.dropped and h.valid_mappings() == R.nmap
    if R.has_stats:
        assert U.read_hist(h) == model_hist(R)
    if R.min_cpg:
        assert U.pdr_rows(h, n) == RL.pdr_rows(R.pdr) and U.pdr_rows(h, n, 3) == RL.pdr_rows(R.pdr, 3)
    assert U.rows_and_rev(h, n, snp) == (model_rows_snp1(R) if snp else (RL.table_rows(R), []))
    if mbias:
        assert U.mbias_cells(h) == (R.mbias, 0)
    h.combine_cpg()
    if R.min_cpg:
        folded = RL.fold(refs, R.pdr)
        assert U.pdr_rows(h, n) == RL.pdr_rows(folded) and U.pdr_rows(h, n, 2) == RL.pdr_rows(folded, 2)
    if not snp:
        assert U.rows_and_rev(h, n)[0] == RL.table_rows(R, RL.fold(refs, R.depth), RL.fold(refs, R.meth))


# ---- the worked example ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def example_fa(tmp_path_factory):
    fa = str(tmp_path_factory.mktemp("readlevel_example") / "one.fa")
    open(fa, "w").write(">one worked example\n%s\n" % EX_REF)
    return fa


def test_worked_example(example_fa, tmp_path):
    with handle(example_fa, nonconv=3, min_cpg=4) as h:
        h.add(EX_ALNS, 0)
        assert U.pdr_rows(h, 1) == sorted([(0, i, 3, 1) for i in CG_C] + [(0, i, 2, 1) for i in CG_G])
        assert h.nonconv_dropped() == 1 and h.valid_mappings() == 6
        cg, ch, tot = U.read_hist(h)
        assert tot == (7, 0, 16, 3) and ch == [6, 0, 0, 1] + [0] * 60
        assert {(a, b): v for a, row in enumerate(cg) for b, v in enumerate(row) if v} == {(5, 5): 2, (5, 0): 2, (5, 3): 1, (5, 4): 1, (3, 2): 1}
        assert written_pdr(h, tmp_path / "pdr.txt") == (PDR_TEXT, 10) and written_stats(h, tmp_path / "stats.txt") == STATS_TEXT
        h.combine_cpg()
        assert U.pdr_rows(h, 1) == [(0, i, 5, 2) for i in CG_C] and U.pdr_rows(h, 1, 6) == []
        assert written_pdr(h, tmp_path / "pdr_g.txt") == (PDR_TEXT_FOLDED, 5) and written_stats(h, tmp_path / "stats_g.txt") == STATS_TEXT
    with handle(example_fa, nonconv=3, min_cpg=6) as h:   # K = 6: no read is eligible
        h.add(EX_ALNS, 0)
        assert U.pdr_rows(h, 1) == [] and written_pdr(h, tmp_path / "none.txt") == (RL.PDR_HEADER, 0) and h.nonconv_dropped() == 1
    with handle(example_fa, nonconv=0, min_cpg=4) as h:   # N = 0: read 4 is eligible and concordant
        h.add(EX_ALNS, 0)
        assert U.pdr_rows(h, 1) == sorted([(0, i, 4, 1) for i in CG_C] + [(0, i, 2, 1) for i in CG_G]) and h.nonconv_dropped() == 0 and h.valid_mappings() == 7


def test_dropped_owner_still_suppresses_its_duplicate(example_fa):
    """-r: read 4 comes first and owns the fragment end; the filter drops it; read 1 at the same end is a duplicate all the same: neither tallied nor piled"""
    dup = [EX_ALNS[3], EX_ALNS[0]]
    R = RL.analyse([EX_REF], dup, trim_fillin=0, rm_dup=True, nonconv=3)
    assert R.verdict == ["dropped", "invalid"] and R.reads == 1
    with handle(example_fa, rm_dup=True, nonconv=3) as h:
        h.add(dup, 0)
        assert U.read_hist(h)[2] == (1, 0, 3, 3) and h.nonconv_dropped() == 1 and h.valid_mappings() == 0 and U.rows_and_rev(h, 1) == ([], []) and U.pdr_rows(h, 1) == []
    with handle(example_fa, rm_dup=True, nonconv=0) as h:   # without the filter the owner is piled, the duplicate is not
        h.add(dup, 0)
        assert U.read_hist(h)[2] == (1, 0, 3, 3) and h.valid_mappings() == 1 and U.pdr_rows(h, 1) == [(0, i, 1, 0) for i in CG_C]


# ---- the edge set ------------------------------------------------------------------------------------------------------------
N0, K0 = 3, 4   # the thresholds the directed reads are built around


class Edges:
    """Four chromosomes.  edgeA (301 letters) ends in C and edgeB (97) begins with G: no CG across the cut.  edgeP (200) is poly-CA: every C is CHH, for reads with
    62, 63 and 64 methylated non-CpG calls.  edgeC (2 100) crosses the report's 1 024-position blocks and holds, in this order: a CpG-rich stretch "ACG" x 70 at
    [200, 410); an A/T stretch at [600, 720) with CG at 610, 630, 650 and 670 (three CpG calls in the first 64 letters of a read at 600, one behind); an A/T
    stretch at [740, 860) with CHH cytosines at 760, 780 and 820 (two in the first 64 letters of a read at 740, one behind); "ACG" x 8 across the cut at 1 024,
    in front of the cut at 2 048 and in the partial last block.  An N beside a C and beside a G, CCGG, lower case in the FASTA.
    Random reads on all four strands, lengths 1, 2, 63, 64, 65, 128, 129, 144, at position 0, at clen - len, one letter further (invalid unless a trim takes
    it off) and in between, with inserts on both sides of the fill-in trim, cuts, and repeated fragments for -r.  A read is all-methylated, all-unmethylated or
    mixed at its CpGs, and converted at its other cytosines except for a few stray ones; one read in ten is a non-converted one."""
    LENGTHS = (1, 2, 63, 64, 65, 128, 129, 144)
    SEED = 20

    def __init__(self):
        rng = np.random.default_rng(self.SEED)
        self.names, self.refs = ["edgeA", "edgeB", "edgeP", "edgeC"], []
        for n, first, last in ((301, "C", "C"), (97, "G", "G"), (200, "C", "A"), (2100, "A", "T")):
            s = rng.choice(list("ACGT"), n).tolist()
            if n == 200:
                s = list("CA" * 100)
            else:
                s[0], s[-1] = first, last
                s[20:25] = list("ACNCG")    # an N behind a C ('+' context) ...
                s[40:45] = list("TGNGA")    # ... and in front of a G ('-' context)
                s[60:64] = list("CCGG")
            if n == 2100:
                s[200:410] = list("ACG" * 70)
                s[600:720] = rng.choice(list("AT"), 120).tolist()
                for at in (610, 630, 650, 670):
                    s[at:at + 2] = list("CG")
                s[740:860] = rng.choice(list("AT"), 120).tolist()
                for at in (760, 780, 820):
                    s[at:at + 3] = list("CAT")
                for at in (1010, 2022, 2070):
                    s[at:at + 24] = list("ACG" * 8)
            self.refs.append("".join(s))
        assert self.refs[0][-1] == "C" and self.refs[1][0] == "G"
        low = lambda s: s[:10] + s[10:50].lower() + s[50:]
        self.fasta = "".join(">%s some text\n%s" % (n, "".join(low(s)[i:i + 50] + "\n" for i in range(0, len(s), 50))) for n, s in zip(self.names, self.refs))
        alns, k = [], 0
        for rep in range(2):
            for c, ref in enumerate(self.refs):
                for L in self.LENGTHS:
                    if L > len(ref):
                        continue
                    for st in range(4):
                        for pos in (0, len(ref) - L, len(ref) - L + 1) + tuple(rng.integers(0, len(ref) - L + 1, (4 if c == 3 else 2) - rep).tolist()):
                            k += 1
                            insert = (0, L + 1, L - 3, -(L - 3), 250, L + 7, -L)[k % 7]
                            cut = (-1, -1, pos + L // 2, pos + L + 5, -1, max(pos - 2, 0), -1, pos + L - 1, -1)[k % 9] if insert > 0 else -1
                            alns.append((c, pos, st, insert, cut, self.read(rng, c, pos, L, st)))
        for st in range(4):  # over the CpG-rich stretch and across both block cuts
            for pos in rng.integers(150, 420 - 144, 12).tolist() + [1024 - 70, 2048 - 64, 2100 - 64]:
                L = int(rng.choice((64, 65, 128, 144))) if pos < 950 else 144 if pos < 1024 else 64
                alns.append((3, pos, st, 0, -1, self.read(rng, 3, pos, L, st, noise=False)))
        # the directed reads, '++' with insert 0 (no fill-in trim, window letter k = read letter k) unless said otherwise
        ref = self.refs[3]
        meth = lambda a, b, keep=(): "".join(x if x != "C" or i in keep else "T" for i, x in enumerate(ref[a:b], a))
        self.directed = {}
        def directed(name, aln):
            self.directed[name] = aln
            alns.append(aln)
        for n_cg in (K0 - 1, K0, K0 + 1, 10, 31, 32):                                          # exactly that many CpG calls, one of them unmethylated
            directed("cg%d" % n_cg, (3, 200, 0, 0, -1, meth(200, 200 + 3 * n_cg, keep=range(204, 410))))
        directed("split_cg", (3, 600, 0, 0, -1, meth(600, 700, keep=(610, 650, 670))))     # 3 + 1 CpG calls around letter 64, discordant
        directed("split_ch_n", (3, 740, 0, 0, -1, meth(740, 840, keep=(760, 780, 820))))   # m_ch = 2 + 1 = N
        directed("split_ch_n1", (3, 740, 0, 0, -1, meth(740, 840, keep=(760, 820))))       # m_ch = 1 + 1 = N - 1
        directed("split_ch_first", (3, 740, 0, 0, -1, meth(740, 840, keep=(760, 780))))    # m_ch = 2 + 0 = N - 1
        for m_ch in (62, 63, 64):
            directed("ch%d" % m_ch, (2, 0, 0, 0, -1, self.refs[2][:2 * m_ch]))
        directed("trim5", (3, 200, 0, 0, -1, meth(200, 212, keep=range(200, 212))))        # K calls at cycles 1, 4, 7, 10: --trim-5p 2 leaves K - 1
        directed("trim5_minus", (3, 200, 1, 0, -1, ref[200:212]))                           # '-+': the G calls at letters 2, 5, 8, 11 are cycles 9, 6, 3, 0
        directed("cut", (3, 203, 0, 250, 203 + 10, meth(203, 215, keep=range(203, 215))))  # K calls; cut behind letter 10 of 12: K - 1
        for i in rng.integers(0, len(alns), 40).tolist():  # the same fragment with other letters: -r has to keep the first
            c, pos, st, insert, cut, s = alns[i]
            alns.append((c, pos, st, insert, cut, self.read(rng, c, pos, len(s), st)))
        order = rng.permutation(len(alns)).tolist()
        self.alns = [alns[i] for i in order]
        self.where = {name: self.alns.index(a) for name, a in self.directed.items()}
        self._res = {}

    def read(self, rng, c, pos, L, st, noise=True):
        ref = self.refs[c]
        match, convert = ("C", "T") if st % 2 == 0 else ("G", "A")
        cg_keep = (0.0, 1.0, 0.5)[int(rng.integers(0, 3))]
        ch_keep = 0.9 if rng.random() < 0.1 else 0.01
        out = []
        for i in range(L):
            g = min(pos + i, len(ref) - 1)
            x = ref[g]
            if x == "N":
                x = "ACGT"[int(rng.integers(0, 4))]
            if x == match:
                in_cg = RL.context_class(ref, g, st % 2 == 0) == 0
                if rng.random() >= (cg_keep if in_cg else ch_keep):
                    x = convert
            elif noise and rng.random() > 0.97:
                x = "ACGTN"[int(rng.integers(0, 5))]
            out.append(x)
        return "".join(out)

    def result(self, trim_fillin=2, rm_dup=False, trim5=0, trim3=0, nonconv=N0, min_cpg=K0, stats=True):
        key = (trim_fillin, rm_dup, trim5, trim3, nonconv, min_cpg)
        if key not in self._res:
            self._res[key] = RL.analyse(self.refs, self.alns, *key)
        R = self._res[key]
        R.has_stats, R.min_cpg = stats, min_cpg
        return R


@pytest.fixture(scope="module")
def edges(tmp_path_factory):
    e = Edges()
    e.dir = tmp_path_factory.mktemp("readlevel_edges")
    e.fa = str(e.dir / "edges.fa")
    open(e.fa, "w").write(e.fasta)
    return e


def test_edge_set_covers_what_it_claims(edges):
    """the model's side only, no library call: the conditions without which the tests below would pass vacuously"""
    R = edges.result()
    count = lambda what: sum(1 for v in R.verdict if v == what)
    assert count("concordant") >= 10 and count("discordant") >= 10 and count("concordant") + count("discordant") >= 50
    assert R.dropped == count("dropped") >= 10 and count("invalid") >= 20 and R.cg_over >= 1
    long_rows = [i for c, i, _, _ in RL.pdr_rows(R.pdr) if c == 3]
    assert all(any(i // 1024 == b for i in long_rows) for b in range(3))
    assert 1023 in long_rows and 1024 in long_rows and max(long_rows) > 2090   # a CG on the first block cut: its C and its G are rows of two blocks
    folded_rows = [i for c, i, _, _ in RL.pdr_rows(RL.fold(edges.refs, R.pdr)) if c == 3]
    assert folded_rows != long_rows and all(edges.refs[3][i] == "C" for i in folded_rows)
    assert {edges.refs[c][i] for c, i, _, _ in RL.pdr_rows(R.pdr)} == {"C", "G"}
    counts = {name: R.counts[i] for name, i in edges.where.items()}
    verdict = {name: R.verdict[i] for name, i in edges.where.items()}
    assert [counts["cg%d" % n][:2] for n in (3, 4, 5, 31, 32)] == [(3, 2), (4, 3), (5, 4), (31, 30), (32, 31)]
    assert [verdict["cg%d" % n] for n in (3, 4, 5, 31, 32)] == ["plain"] + ["discordant"] * 4
    assert counts["split_cg"] == (4, 3, 0, 0) and verdict["split_cg"] == "discordant"
    assert counts["split_ch_n"] == (0, 0, 3, 3) and verdict["split_ch_n"] == "dropped"
    assert counts["split_ch_n1"] == (0, 0, 3, 2) and counts["split_ch_first"] == (0, 0, 3, 2) and verdict["split_ch_n1"] == verdict["split_ch_first"] == "plain"
    assert [counts["ch%d" % n] for n in (62, 63, 64)] == [(0, 0, n, n) for n in (62, 63, 64)] and R.ch[62] >= 1 and R.ch[63] >= 2
    assert counts["trim5"] == counts["trim5_minus"] == (4, 4, 0, 0) and counts["cut"] == (3, 3, 0, 0) and verdict["cut"] == "plain"
    T = edges.result(2, False, 2, 0)
    assert T.counts[edges.where["trim5"]] == T.counts[edges.where["trim5_minus"]] == (3, 3, 0, 0) and T.verdict[edges.where["trim5"]] == "plain"
    D = edges.result(2, True)
    assert D.nmap < R.nmap and D.reads < R.reads and D.dropped <= R.dropped
    assert R.ch_meth > 0 and sum(R.ch[N0:]) == R.dropped and R.cg[0][0] > 0 and sum(map(sum, R.cg)) + R.cg_over == R.reads == sum(R.ch)


# ---- model parity: histogram, dropped, PDR cells, and what the filter leaves in the pile-up ------------------------------------------------
CONFIGS = [  # trim_fillin, rm_dup, trim5, trim3, N, K, histogram, C/T-SNP mode, M-bias
    (2, False, 0, 0, 3, 4, True, 1, False),    # k_meth_pile<SNP> behind the filter
    (2, False, 0, 0, 3, 4, True, 1, True),     # k_meth_pile_mbias<SNP> behind the filter
    (2, True, 0, 0, 3, 4, True, 0, False),
    (0, True, 2, 3, 1, 5, True, 0, True),
    (5, False, 2, 0, 0, 4, True, 0, False),    # no filter: no drop flags
    (2, False, 0, 0, 3, 0, False, 0, False),   # the filter alone
    (2, False, 0, 0, 0, 0, True, 0, True),     # the histogram alone
    (2, True, 0, 0, 0, 1, False, 0, False),    # PDR alone, every read with a CpG call eligible
]


@pytest.mark.parametrize("trim_fillin,rm_dup,trim5,trim3,nonconv,min_cpg,stats,snp,mbias", CONFIGS)
def test_model_parity(edges, trim_fillin, rm_dup, trim5, trim3, nonconv, min_cpg, stats, snp, mbias):
    R = edges.result(trim_fillin, rm_dup, trim5, trim3, nonconv, min_cpg, stats)
    assert R.reads > 500 and (not nonconv or R.dropped >= 10) and (not min_cpg or len(RL.pdr_rows(R.pdr)) > 50)
    with handle(edges.fa, rm_dup, nonconv, stats, min_cpg, snp, mbias, (trim5, trim3)) as h:
        h.add(edges.alns, trim_fillin)
        compare(h, R, edges.refs, snp, mbias)


def test_directed_cut(edges):
    """a cut_at that takes a read from K to K - 1 CpG calls: eligible without the cut, not with it"""
    c, pos, st, insert, cut, s = edges.directed["cut"]
    for aln, want in (((c, pos, st, insert, cut, s), (3, 3, 0, 0)), ((c, pos, st, insert, -1, s), (4, 4, 0, 0))):
        R = RL.analyse(edges.refs, [aln], 2, False, 0, 0, N0, K0)
        assert R.counts == [want] and R.verdict == ["plain" if want[0] < K0 else "concordant"]
        R.has_stats, R.min_cpg = True, K0
        with handle(edges.fa, nonconv=N0, min_cpg=K0) as h:
            h.add([aln], 2)
            compare(h, R, edges.refs)


@pytest.mark.parametrize("mbias", [False, True])
def test_filter_equals_feeding_the_kept_reads(edges, mbias):
    """with the filter on, the pile-up holds what a handle without the filter holds that was fed the non-dropped reads only"""
    R = edges.result(2, False)
    kept = [edges.alns[i] for i in R.kept]
    assert 0 < R.dropped and len(kept) == R.nmap < R.reads
    with handle(edges.fa, nonconv=N0, snp=1, mbias=mbias) as h, handle(edges.fa, nonconv=0, snp=1, mbias=mbias) as plain:
        h.add(edges.alns, 2)
        plain.add(kept, 2)
        assert U.rows_and_rev(h, 4, 1) == U.rows_and_rev(plain, 4, 1) == model_rows_snp1(R) and h.valid_mappings() == plain.valid_mappings() == R.nmap
        assert U.pdr_rows(h, 4) == U.pdr_rows(plain, 4) == RL.pdr_rows(R.pdr)
        assert (h.nonconv_dropped(), plain.nonconv_dropped()) == (R.dropped, 0)
        if mbias:
            assert U.mbias_cells(h) == U.mbias_cells(plain) == (R.mbias, 0)


def test_histogram_does_not_depend_on_the_threshold(edges):
    want = model_hist(edges.result(2, False, 0, 0, 0))
    for n in (0, 1, 3):
        R = edges.result(2, False, 0, 0, n)
        assert model_hist(R) == want and R.dropped == sum(R.ch[n:]) * (n > 0)
        with handle(edges.fa, nonconv=n) as h:
            h.add(edges.alns, 2)
            cg, ch, tot = U.read_hist(h)
            assert (cg, ch, tot) == want and h.nonconv_dropped() == (sum(ch[n:]) if n else 0) == R.dropped and h.valid_mappings() == R.nmap


# ---- accumulation and contention ------------------------------------------------------------------------------------------------------------
def test_accumulation_and_contention(edges):
    """20 000 copies of one eligible discordant read among 20 000 random ones in one bsx_meth_add: more reads than a block's waves and more blocks than one;
    one histogram cell and ten PDR cells receive 20 000 each.  The same reads in two adds give the same."""
    rng = np.random.default_rng(5)
    n = 20_000
    hot = edges.directed["cg10"]
    pool = [a for a, v in zip(edges.alns, edges.result().verdict) if v != "invalid"]
    rand = [pool[i] for i in rng.integers(0, len(pool), n).tolist()]
    alns = [x for pair in zip([hot] * n, rand) for x in pair]
    # the model on the distinct alignments, weighted (no -r: an alignment's calls do not depend on the others)
    uniq = sorted(set(alns))
    weight = {a: 0 for a in uniq}
    for a in alns:
        weight[a] += 1
    one = RL.analyse(edges.refs, [hot], 2, False, 0, 0, N0, K0)
    assert one.counts == [(10, 9, 0, 0)] and one.verdict == ["discordant"]
    cg = np.zeros((32, 32), np.int64); ch = np.zeros(64, np.int64); tot = np.zeros(4, np.int64)
    pdr = [np.zeros((len(r), 2), np.int64) for r in edges.refs]
    dropped = nmap = 0
    for a in uniq:
        R = RL.analyse(edges.refs, [a], 2, False, 0, 0, N0, K0)
        w = weight[a]
        cg += w * np.array(R.cg); ch += w * np.array(R.ch); tot += w * np.array([R.reads, R.cg_over, R.ch_calls, R.ch_meth])
        dropped += w * R.dropped; nmap += w * R.nmap
        for c in range(4):
            pdr[c] += w * np.array(R.pdr[c])
    want_rows = RL.pdr_rows([p.tolist() for p in pdr])
    assert cg[10][9] >= n and sum(1 for c, i, r, d in want_rows if r >= n and d >= n) == 10 and dropped > 100 and tot[0] == 2 * n
    for split in ((2 * n,), (n + 1, n - 1)):
        with handle(edges.fa, nonconv=N0, min_cpg=K0) as h:
            at = 0
            for part in split:
                h.add(alns[at:at + part], 2)
                at += part
            assert U.read_hist(h) == (cg.tolist(), ch.tolist(), tuple(tot.tolist()))
            assert U.pdr_rows(h, 4) == want_rows and h.nonconv_dropped() == dropped and h.valid_mappings() == nmap
            h.combine_cpg()
            folded = RL.pdr_rows(RL.fold(edges.refs, [p.tolist() for p in pdr]))
            assert U.pdr_rows(h, 4) == folded and sum(1 for c, i, r, d in folded if r >= n and d >= n) == 10


# ---- state and errors ----------------------------------------------------------------------------------------------------------------------------
def test_state_and_errors(edges, tmp_path):
    buf = np.zeros(4096, np.uint64)
    p = buf.ctypes.data
    with handle(edges.fa, stats=False, min_cpg=0) as h:
        L = h.L
        nr = C.c_uint32()
        assert L.bsx_meth_read_stats_fetch(h.h, p, p, p) == BSX_ERR_STATE and L.bsx_meth_write_read_stats(h.h, str(tmp_path / "s").encode()) == BSX_ERR_STATE
        assert L.bsx_meth_pdr_report_chr(h.h, 0, 1, C.byref(nr)) == BSX_ERR_STATE and L.bsx_meth_pdr_fetch_rows(h.h, p, p, p) == BSX_ERR_STATE
        assert L.bsx_meth_write_pdr(h.h, str(tmp_path / "p").encode(), 1, None) == BSX_ERR_STATE and not os.path.exists(tmp_path / "p")
        assert L.bsx_meth_set_read_stats(h.h, 1) == 0 and L.bsx_meth_read_stats_fetch(h.h, p, p, p) == 0 and not buf.any()
        assert L.bsx_meth_read_stats_fetch(h.h, None, p, p) == BSX_ERR_ARG and L.bsx_meth_read_stats_fetch(h.h, p, p, None) == BSX_ERR_ARG
        assert L.bsx_meth_set_read_stats(h.h, 0) == 0 and L.bsx_meth_read_stats_fetch(h.h, p, p, p) == BSX_ERR_STATE       # off again before any add
        assert L.bsx_meth_set_pdr(h.h, 4) == 0 and L.bsx_meth_pdr_report_chr(h.h, 0, 1, C.byref(nr)) == 0 and nr.value == 0
        assert L.bsx_meth_pdr_report_chr(h.h, 0, 0, C.byref(nr)) == BSX_ERR_ARG and L.bsx_meth_pdr_report_chr(h.h, 4, 1, C.byref(nr)) == BSX_ERR_ARG
        assert L.bsx_meth_pdr_report_chr(h.h, 0, 1, None) == BSX_ERR_ARG and L.bsx_meth_nonconv_dropped(h.h, None) == BSX_ERR_ARG
        assert L.bsx_meth_set_pdr(h.h, 0) == 0 and L.bsx_meth_pdr_fetch_rows(h.h, p, p, p) == BSX_ERR_STATE
        h.add(edges.alns[:50], 2)
        assert L.bsx_meth_set_read_stats(h.h, 1) == BSX_ERR_STATE and L.bsx_meth_set_pdr(h.h, 4) == BSX_ERR_STATE
        assert L.bsx_meth_set_pdr(h.h, 0) == 0 and L.bsx_meth_set_nonconv(h.h, 3) == 0                                      # no change; the filter at any time
    with handle(edges.fa) as h:
        h.add(edges.alns[:50], 2)
        assert h.L.bsx_meth_set_read_stats(h.h, 0) == BSX_ERR_STATE and h.L.bsx_meth_set_pdr(h.h, 0) == BSX_ERR_STATE
        assert h.L.bsx_meth_set_pdr(h.h, 2) == 0                                                                             # another threshold: later adds


def test_set_nonconv_between_two_adds(edges):
    """the threshold applies to later adds: the first half is piled unfiltered, the second filtered (no -r: the halves do not depend on each other)"""
    half = len(edges.alns) // 2
    a, b = edges.alns[:half], edges.alns[half:]
    A, B = RL.analyse(edges.refs, a, 2, False, 0, 0, 0, K0), RL.analyse(edges.refs, b, 2, False, 0, 0, N0, K0)
    plus = lambda x, y: [[p + q for p, q in zip(u, v)] for u, v in zip(x, y)]
    assert A.dropped == 0 < B.dropped and sum(A.ch[N0:]) > 0
    with handle(edges.fa) as h:
        h.add(a, 2)
        assert h.L.bsx_meth_set_nonconv(h.h, N0) == 0
        h.add(b, 2)
        assert h.nonconv_dropped() == B.dropped and h.valid_mappings() == A.nmap + B.nmap
        assert U.read_hist(h) == (plus(A.cg, B.cg), [p + q for p, q in zip(A.ch, B.ch)], tuple(p + q for p, q in zip(model_hist(A)[2], model_hist(B)[2])))
        both = [[[p + q for p, q in zip(u, v)] for u, v in zip(x, y)] for x, y in zip(A.pdr, B.pdr)]
        assert U.pdr_rows(h, 4) == RL.pdr_rows(both)
        assert U.rows_and_rev(h, 4)[0] == RL.table_rows(A, plus(A.depth, B.depth), plus(A.meth, B.meth))


# ---- command line -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["bsp", "sam"])
def test_command_line(fmt, edges, tmp_path, capsys):
    from bsmap_amd import methratio
    import ctsnp_model
    path = str(tmp_path / ("in." + fmt))
    with open(path, "w") as f:
        if fmt == "sam":
            f.write("".join("@SQ\tSN:%s\tLN:%d\n" % (n, len(r)) for n, r in zip(edges.names, edges.refs)))
        for k, (c, pos, st, insert, cut, s) in enumerate(edges.alns):
            if fmt == "sam":  # PNEXT = cut_at + 1; 0 (with a positive insert: "no cut" in the C ABI) where the set has none
                f.write("r%d\t0\t%s\t%d\t255\t%dM\t=\t%d\t%d\t%s\t%s\tNM:i:0\tZS:Z:%s\n" % (k, edges.names[c], pos + 1, len(s), cut + 1, insert, s, "I" * len(s), STRANDS[st]))
            else:
                f.write("r%d\t%s\t%s\tUM\t%s\t%d\t%s\t%d\n" % (k, s, "I" * len(s), edges.names[c], pos + 1, STRANDS[st], insert))
    alns = edges.alns if fmt == "sam" else [(c, pos, st, insert, -1, s) for c, pos, st, insert, cut, s in edges.alns]  # a BSP line carries no mate position
    R = RL.analyse(edges.refs, alns, 2, True, 0, 0, 2, 5)
    folded = RL.fold(edges.refs, R.pdr)
    want_pdr, want_stats = RL.pdr_text(edges.names, edges.refs, folded, 2), RL.read_stats_text(R)
    K = ctsnp_model.Counters(edges.refs)
    K.depth, K.meth, K.nmap = RL.fold(edges.refs, R.depth), RL.fold(edges.refs, R.meth), R.nmap
    want_table, nc, nd = ctsnp_model.table(edges.names, K, 1, True, 0)
    assert R.dropped >= 10 and want_pdr.count("\n") > 30 and want_pdr != RL.pdr_text(edges.names, edges.refs, R.pdr, 2)
    out, pdr, stats = (str(tmp_path / x) for x in ("t.txt", "pdr.txt", "stats.txt"))
    methratio.main(["-q", "-z", "-r", "-g", "--nonconv-filter", "2", "--read-stats", stats, "--pdr", pdr, "--pdr-min-cpg", "5", "--pdr-min-reads", "2",
                    "-o", out, "-d", edges.fa, path])
    assert capsys.readouterr().out == ctsnp_model.summary(R.nmap, nc, nd)
    assert open(pdr).read() == want_pdr and open(stats).read() == want_stats and open(out).read() == want_table
    # the dropped count goes to stderr with the progress lines
    methratio.run(edges.fa, [path], out, rm_dup=True, meth0=True, quiet=False, nonconv_filter=2)
    assert "%d reads with 2 or more methylated non-CpG calls dropped" % R.dropped in capsys.readouterr().err


GOLD = json.load(gzip.open(os.path.join(G.GOLDEN, "methratio.json.gz"), "rt"))


def test_command_line_without_the_options_is_unchanged(tmp_path, capsys):
    """run() with none of the three options on a pinned input: the pinned table and summary, byte for byte"""
    import base64
    from bsmap_amd import methratio
    case = sorted(c for c in GOLD["cases"] if "same_as" not in GOLD["cases"][c]["runs"][0] and not GOLD["cases"][c]["runs"][0]["crashed"])[0]
    fa = str(tmp_path / "g.fa")
    open(fa, "w").write(GOLD["fasta"])
    for fn, txt in GOLD["cases"][case]["files"].items():
        open(str(tmp_path / fn), "w").write(txt)
    for fn, b64 in GOLD["cases"][case].get("files_b64", {}).items():
        open(str(tmp_path / fn), "wb").write(base64.b64decode(b64))
    run = GOLD["cases"][case]["runs"][0]
    out = str(tmp_path / "t.txt")
    methratio.main(["-q", "-o", out, "-d", fa] + list(run["options"]) + [str(tmp_path / fn) for fn in GOLD["cases"][case]["infiles"]])
    assert open(out).read() == run["table"] and capsys.readouterr().out == run["stdout"] and run["table"].count("\n") > 10
