"""C/T-SNP correction and context filter of bsmap_amd.methratio (bsx_meth_set_ct_snp / _set_contexts / _fetch_rows_snp, -i / -x)
against the pure-Python model of ctsnp_model.py, which never looks at the library's output.

The v2.6 script the project mirrors has neither option, so there is no reference table for them: the model is the yardstick, and test 9
ties the corrected table back to the pinned v2.6 tables where the two must agree."""
import gzip
import json
import os

import numpy as np
import pytest

import ctsnp_model as M
import golden_util as G
import meth_util as U

pytestmark = pytest.mark.gpu
STRANDS = M.STRANDS
BSX_ERR_ARG, BSX_ERR_STATE = -1, -5


# ---- the library through bsmap_amd.methratio.Meth ---------------------------------------------------------------------------
def rows(h, n_chr, min_depth=1, meth0=1, snp=True):
    """[(chr id, pos, dd, m, g, ga)] (g = ga = 0 with snp=False: the mode is off), n_covered, sum_depth"""
    return U.table_rows(h, n_chr, min_depth, meth0, snp, pad=True)


# ---- the edge set ------------------------------------------------------------------------------------------------------------
class Edges:
    """Three chromosomes of 301, 97 and 2 100 letters.  The first ends in C, the second begins with G; an N beside a C and beside a G, CCGG, lower case in
    the FASTA.  The third crosses the 1 024-position block cuts of the report at 1 024 and 2 048 and has a partial tail; its middle block holds C/G only in
    [1510, 1550), each of them a planted SNP that the opposite strand always shows converted, under reads of all four strands: mode 2 removes every
    candidate row of that block.  Alignments as in the M-bias edge set: four strands, lengths 1, 2, 63, 64, 65, 128, 129, 144, at position 0, at clen - len,
    one letter further (invalid) and in between, inserts on both sides of the '++' / '-+' trim, cut_at inside, behind and in front of the read, repeated
    fragments for -r.  Planted SNPs: at about 5 % of the reference C/G positions the reads of the other strand show the converted letter with
    probability 0.5, at a few more always."""
    LENGTHS = (1, 2, 63, 64, 65, 128, 129, 144)
    SEED = 31

    def __init__(self):
        rng = np.random.default_rng(self.SEED)
        self.names, self.refs = ["edgeA", "edgeB", "edgeC"], []
        for n, first, last in ((301, "C", "C"), (97, "G", "G"), (2100, "A", "T")):
            s = rng.choice(list("ACGT"), n).tolist()
            s[0], s[-1] = first, last
            s[20:25] = list("ACNCG")    # an N behind a C ('+' context) ...
            s[40:45] = list("TGNGA")    # ... and in front of a G ('-' context)
            s[60:64] = list("CCGG")
            if n == 2100:
                s[1024:2048] = rng.choice(list("AT"), 1024).tolist()
                s[1510:1550] = rng.choice(list("ACGT"), 40).tolist()
                s[1021:1024] = list("CGC")   # rows just in front of the first cut and just behind the second one
                s[2048:2051] = list("GCG")
            self.refs.append("".join(s))
        assert self.refs[0][-1] == "C" and self.refs[1][0] == "G"
        low = lambda s: s[:10] + s[10:50].lower() + s[50:]
        self.fasta = "".join(">%s some text\n%s" % (n, "".join(low(s)[i:i + 50] + "\n" for i in range(0, len(s), 50))) for n, s in zip(self.names, self.refs))
        assert self.fasta != self.fasta.upper()
        self.snp = []  # per chromosome {position: probability that a read of the other strand shows the converted letter}
        for c, ref in enumerate(self.refs):
            cg = [i for i, ch in enumerate(ref) if ch in "CG"]
            p = {i: 0.5 for i in cg if rng.random() < 0.05}
            p.update({int(i): 1.0 for i in rng.choice(cg, 4, replace=False)})
            if c == 2:
                p.update({i: 1.0 for i in range(1024, 2048) if ref[i] in "CG"})
            self.snp.append(p)
        alns = []
        k = 0
        for rep in range(2):
            for c, ref in enumerate(self.refs):
                for L in self.LENGTHS:
                    if L > len(ref):
                        continue
                    for st in range(4):
                        for pos in (0, len(ref) - L) + tuple(rng.integers(0, len(ref) - L + 1, (4 if c == 2 else 2) - rep).tolist()):
                            k += 1
                            insert = (0, L + 1, L - 3, -(L - 3), 250, L + 7, -L)[k % 7]
                            cut = (-1, -1, pos + L // 2, pos + L + 5, -1, max(pos - 2, 0), -1, pos + L - 1, -1)[k % 9] if insert > 0 else -1
                            alns.append((c, pos, st, insert, cut, self.read(rng, c, pos, L, st)))
        for c, ref in enumerate(self.refs):  # 64 letters from clen - 63: one letter past the end unless a trim takes it off
            for st in (0, 3, 1, 2):
                alns.append((c, len(ref) - 63, st, 0, -1, self.read(rng, c, len(ref) - 64, 64, st)))
        for st in range(4):  # across both block cuts of the long chromosome, and all four strands over the SNP window of its middle block
            alns.append((2, 1024 - 70, st, 0, -1, self.read(rng, 2, 1024 - 70, 144, st)))
            alns.append((2, 2048 - 64, st, 0, -1, self.read(rng, 2, 2048 - 64, 116, st)))
            for rep in range(2):
                alns.append((2, 1490 + st + 4 * rep, st, 0, -1, self.read(rng, 2, 1490 + st + 4 * rep, 80, st, noise=False)))
        for i in rng.integers(0, len(alns), 40).tolist():  # the same fragment with other letters: -r has to keep the first
            c, pos, st, insert, cut, s = alns[i]
            alns.append((c, pos, st, insert, cut, self.read(rng, c, pos, len(s), st)))
        order = rng.permutation(len(alns)).tolist()
        self.alns = [alns[i] for i in order]
        self._pile = {}

    def read(self, rng, c, pos, L, st, noise=True):
        ref = self.refs[c]
        out = []
        match, convert, rc_match, rc_convert = ("C", "T", "G", "A") if st % 2 == 0 else ("G", "A", "C", "T")
        for i in range(L):
            g = min(pos + i, len(ref) - 1)
            x, r = ref[g], rng.random()
            if x == "N":
                x = "ACGT"[int(rng.integers(0, 4))]
            if x == match and r < 0.5:
                x = convert
            elif x == rc_match and g in self.snp[c] and rng.random() < self.snp[c][g]:
                x = rc_convert
            elif noise and r > 0.96:
                x = "ACGTN"[int(rng.integers(0, 5))]
            out.append(x)
        return "".join(out)

    def pile(self, trim_fillin=2, rm_dup=False, trim5=0, trim3=0, cpg=False):
        key = (trim_fillin, rm_dup, trim5, trim3)
        if key not in self._pile:
            self._pile[key] = M.pileup(self.refs, self.alns, trim_fillin, rm_dup, trim5, trim3)
        if cpg:
            if key + (1,) not in self._pile:
                self._pile[key + (1,)] = M.combine_cpg(self._pile[key])
            return self._pile[key + (1,)]
        return self._pile[key]


@pytest.fixture(scope="module")
def edges(tmp_path_factory):
    e = Edges()
    e.dir = tmp_path_factory.mktemp("ctsnp_edges")
    e.fa = str(e.dir / "edges.fa")
    open(e.fa, "w").write(e.fasta)
    return e


def test_edge_set_covers_what_it_claims(edges):
    """the generated set holds what the other tests rely on (the model's side only; no library call)"""
    K = edges.pile(2, False)
    assert 0 < K.nmap < len(edges.alns) and edges.pile(2, True).nmap < K.nmap   # some alignments are invalid, and -r removes some more
    all_rows = M.rows(K, 1, True, 0)[0]
    assert any(g != ga and g > 0 for _, _, dd, m, g, ga in all_rows)
    assert any(g == 0 < ga for _, _, dd, m, g, ga in all_rows)
    assert any(g != ga and g > 0 and m > M.effective(dd, m, g, ga)[0] for _, _, dd, m, g, ga in all_rows)  # the min() of the ratio matters
    assert any(g != ga and g > 0 and 0 < m < M.effective(dd, m, g, ga)[0] for _, _, dd, m, g, ga in all_rows)
    assert any(g == ga > 0 for _, _, dd, m, g, ga in all_rows)
    assert any(ga > 0 and dd == 0 for c in range(3) for dd, ga in zip(K.depth[c], K.rev_ga[c]))   # reverse calls alone make no row
    # the long chromosome: mode 2 removes every candidate of the middle 1 024-block, and rows sit on both sides of both cuts' neighbours
    blocks = lambda rr: [sorted(i for c, i, *_ in rr if c == 2 and i // 1024 == b) for b in range(3)]
    b0, b1 = blocks(all_rows), blocks(M.rows(K, 1, True, 1)[0])
    b2, b3 = blocks(M.rows(K, 1, True, 2)[0]), blocks(M.rows(K, 3, True, 2)[0])
    assert len(b0[1]) >= 10 and b1[1] == [] and b2[1] == [] and b3[1] == []
    assert 1023 in b2[0] and 2048 in b2[2] and 1021 in b2[0] and b2[2][-1] > 2090 and b3[0] and b3[2]
    seen = {(edges.refs[c][i], M.context_class(edges.refs[c], i, edges.refs[c][i] == "C")) for c, i, *_ in M.rows(K, 1, True, 1)[0]}
    assert seen == {(l, x) for l in "CG" for x in range(4)}                                        # every context class on both strands
    F = edges.pile(2, False, cpg=True)
    assert F.rev_ga != K.rev_ga and sum(map(sum, F.rev_ga)) == sum(map(sum, K.rev_ga))


# ---- 1. counter parity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("rm_dup", [0, 1])
@pytest.mark.parametrize("trim_fillin", [0, 2, 5])
def test_counter_parity(edges, trim_fillin, rm_dup, mode):
    K = edges.pile(trim_fillin, bool(rm_dup))
    with U.open_meth(edges.fa, rm_dup, mode) as h:
        h.add(edges.alns, trim_fillin)
        assert rows(h, 3) == M.rows(K, 1, True, mode)
        assert h.valid_mappings() == K.nmap
    # with the M-bias twin: the same rows, and the tally of a handle that has the mode off
    with U.open_meth(edges.fa, rm_dup, mode, mbias=True) as h, U.open_meth(edges.fa, rm_dup, 0, mbias=True) as plain:
        h.add(edges.alns, trim_fillin)
        plain.add(edges.alns, trim_fillin)
        assert rows(h, 3) == M.rows(K, 1, True, mode) and h.valid_mappings() == K.nmap
        (cells, over), (cells0, over0) = h.mbias(), plain.mbias()
        assert over == over0 == 0 and cells.sum() > 0 and np.array_equal(cells, cells0)
        assert [r[:4] for r in rows(plain, 3, snp=False)[0]] == [r[:4] for r in M.rows(K, 1, True, 0)[0]]


# ---- 2. table bytes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cpg", [0, 1])
@pytest.mark.parametrize("min_depth", [1, 3])
@pytest.mark.parametrize("meth0", [0, 1])
@pytest.mark.parametrize("mode", [1, 2])
def test_table_bytes(edges, mode, meth0, min_depth, cpg):
    K = edges.pile(2, False, cpg=bool(cpg))
    with U.open_meth(edges.fa, 0, mode) as h:
        h.add(edges.alns, 2)
        if cpg:
            h.combine_cpg()
        got = U.written_table(h, edges.dir / "t.txt", min_depth, meth0)
    want = M.table(edges.names, K, min_depth, bool(meth0), mode)
    assert got[1:] == want[1:] and got[0] == want[0]
    assert got[0].count("\n") > (20 if meth0 else 5)


def test_two_tables_from_one_pileup(edges):
    with U.open_meth(edges.fa, 0, 1) as h:
        h.add(edges.alns, 2)
        t1 = U.written_table(h, edges.dir / "m1.txt")
        h.set_ct_snp(2)
        t2 = U.written_table(h, edges.dir / "m2.txt")
        h.set_ct_snp(1)
        assert U.written_table(h, edges.dir / "m1b.txt") == t1
    with U.open_meth(edges.fa, 0, 2) as h:
        h.add(edges.alns, 2)
        fresh = U.written_table(h, edges.dir / "m2f.txt")
    assert t2 == fresh == M.table(edges.names, edges.pile(2, False), 1, True, 2) and t1 != t2
    assert t1 == M.table(edges.names, edges.pile(2, False), 1, True, 1)


# ---- 3. the CpG fold at a chromosome boundary --------------------------------------------------------------------------------------------
def test_cpg_fold_at_a_chromosome_boundary(tmp_path):
    """the first chromosome ends in C, the second begins with G: in the concatenated text they read CG, and neither the forward nor the reverse
    counters of that G may move onto that C"""
    refs = ["TTACGTTAC", "GTTACGTT"]
    fa = str(tmp_path / "two.fa")
    open(fa, "w").write(">x1\nTTACGTTAC\n>x2\nGTTACGTT\n")
    alns = [(0, 0, 0, 0, -1, "TTACGTTAC"),    # x1: '++' shows C over the last C
            (0, 0, 1, 0, -1, "TTACGTTAC"),    #     '-+' shows C there ...
            (0, 1, 3, 0, -1, "TACGTTAT"),     #     ... and '--' shows T: rev_G 1, rev_GA 2
            (1, 0, 1, 0, -1, "GTTACGTT"),     # x2: '-+' shows G over the first G
            (1, 0, 0, 0, -1, "GTTACGTT"), (1, 0, 2, 0, -1, "GTTAC"), (1, 0, 0, 0, -1, "ATT")]   # two '+' reads show G there, one shows A: 2, 3
    K = M.pileup(refs, alns, 0)
    assert (K.depth[0][8], K.meth[0][8], K.rev_g[0][8], K.rev_ga[0][8]) == (1, 1, 1, 2)
    assert (K.depth[1][0], K.meth[1][0], K.rev_g[1][0], K.rev_ga[1][0]) == (1, 1, 2, 3)
    F = M.combine_cpg(K)
    assert F.depth[0][3] == K.depth[0][3] + K.depth[0][4] > K.depth[0][3] and F.rev_ga[0][3] == K.rev_ga[0][3] + K.rev_ga[0][4] > K.rev_ga[0][3]
    with U.open_meth(fa, 0, 1) as h:
        h.add(alns, 0)
        assert rows(h, 2) == M.rows(K, 1, True, 1)
        h.combine_cpg()
        got = rows(h, 2)
    assert got == M.rows(F, 1, True, 1)
    assert (0, 8, 1, 1, 1, 2) in got[0] and (1, 0, 1, 1, 2, 3) in got[0]


# ---- 4. contention ------------------------------------------------------------------------------------------------------------------------
def test_contention(tmp_path):
    """2^16 copies each of one '++' and one '-+' alignment over the same 300 letters: the forward adds of the one and the reverse adds of the other
    hit the same positions.  One bsx_meth_add call and three: every counter is 65 536 x the model's for the two alignments."""
    rng = np.random.default_rng(7)
    ref = "".join(rng.choice(list("ACGT"), 400).tolist())
    fa = str(tmp_path / "one.fa")
    open(fa, "w").write(">one\n" + ref + "\n")
    body = ref[50:350]
    plus = "".join(("T" if (ch == "C" and i % 3 == 0) else "A" if (ch == "G" and i % 5 == 0) else ch) for i, ch in enumerate(body))
    minus = "".join(("A" if (ch == "G" and i % 2 == 0) else "T" if (ch == "C" and i % 7 == 0) else ch) for i, ch in enumerate(body))
    pair = [(0, 50, 0, 0, -1, plus), (0, 50, 1, 0, -1, minus)]
    K = M.pileup([ref], pair, 2)
    want, nc, nd = M.rows(K, 1, True, 1)
    assert K.nmap == 2 and any(g == 1 and ga == 1 for *_, g, ga in want) and any(g == 0 and ga == 1 for g, ga in zip(K.rev_g[0], K.rev_ga[0]))
    assert any(m == 1 for _, _, dd, m, g, ga in want) and any(m == 0 for _, _, dd, m, g, ga in want)
    n = 1 << 16
    for split in ((2 * n,), (1, 60_001, 2 * n - 60_002)):
        with U.open_meth(fa, 0, 1) as h:
            at = 0
            for part in split:  # the two alignments alternate through the whole input
                h.add([pair[(at + i) & 1] for i in range(part)], 2)
                at += part
            got, got_nc, got_nd = rows(h, 1)
            assert h.valid_mappings() == 2 * n
        assert got == [(c, i, dd * n, m * n, g * n, ga * n) for c, i, dd, m, g, ga in want] and (got_nc, got_nd) == (nc, nd * n)
        assert max(g for *_, g, ga in got) == n > 65535 and max(ga for *_, ga in got) == n


# ---- 5. cycle trimming ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trim5,trim3", [(3, 0), (0, 4), (5, 5), (200, 0)])
def test_cycle_trimming(edges, trim5, trim3):
    K = edges.pile(2, True, trim5, trim3)
    with U.open_meth(edges.fa, 1, 1, trim=(trim5, trim3)) as h:
        h.add(edges.alns, 2)
        got = rows(h, 3)
        assert got == M.rows(K, 1, True, 1)
        assert h.valid_mappings() == K.nmap == edges.pile(2, True).nmap
        table = U.written_table(h, edges.dir / "trim.txt")
    if (trim5, trim3) == (200, 0):
        assert got == ([], 0, 0) and table == (M.HEADER12, 0, 0) and sum(map(sum, K.rev_ga)) == 0
    else:
        assert len(got[0]) > 100 and M.rows(K, 1, True, 1) != M.rows(edges.pile(2, True), 1, True, 1)


# ---- 6. context filter --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_context_filter(edges, mode):
    K = edges.pile(2, False)
    with U.open_meth(edges.fa, 0, mode) as h:
        h.add(edges.alns, 2)
        free = U.written_table(h, edges.dir / "free.txt")
        assert free == M.table(edges.names, K, 1, True, mode)
        lines = free[0].split("\n")[1:-1]
        cls = []   # the class of every unfiltered row
        for l in lines:
            f = l.split("\t")
            c, i = edges.names.index(f[0]), int(f[1]) - 1
            cls.append(M.context_class(edges.refs[c], i, f[2] == "+"))
        def model_rows(*a):  # with the mode off the library reports no opposite-strand counters
            rr, nc, nd = M.rows(K, *a)
            return (rr if mode else [r[:4] + (0, 0) for r in rr]), nc, nd
        for mask in range(0, 16):
            h.set_contexts(mask)
            assert rows(h, 3, snp=bool(mode)) == model_rows(1, True, mode, mask), mask
            got = U.written_table(h, edges.dir / "masked.txt")
            assert got == M.table(edges.names, K, 1, True, mode, mask), mask
            if mask in (0, 15):
                assert got == free
            else:  # exactly the unfiltered rows of the chosen classes, in their order
                assert got[0].split("\n")[1:-1] == [l for l, x in zip(lines, cls) if (mask >> x) & 1] and 0 < got[1] < free[1], mask
        h.set_contexts(3)
        assert rows(h, 3, 3, 0, snp=bool(mode)) == model_rows(3, False, mode, 3)


# ---- 7. state rules ---------------------------------------------------------------------------------------------------------------------------------
def test_state_rules(edges):
    g, ga = np.zeros(4096, np.uint32), np.zeros(4096, np.uint32)
    K = edges.pile(2, False)
    with U.open_meth(edges.fa) as h:
        L = h.L
        fetch = lambda: L.bsx_meth_fetch_rows_snp(h.h, g.ctypes.data, ga.ctypes.data)
        assert fetch() == BSX_ERR_STATE
        assert L.bsx_meth_set_ct_snp(h.h, 3) == BSX_ERR_ARG and L.bsx_meth_set_ct_snp(h.h, -1) == BSX_ERR_ARG
        assert L.bsx_meth_set_contexts(h.h, 16) == BSX_ERR_ARG and L.bsx_meth_set_contexts(h.h, 15) == 0 and L.bsx_meth_set_contexts(h.h, 0) == 0
        assert L.bsx_meth_set_ct_snp(h.h, 1) == 0 and fetch() == 0
        assert L.bsx_meth_set_ct_snp(h.h, 0) == 0 and fetch() == BSX_ERR_STATE     # 1 -> 0 before any add ...
        h.add(edges.alns, 2)
        assert L.bsx_meth_set_ct_snp(h.h, 1) == BSX_ERR_STATE and L.bsx_meth_set_ct_snp(h.h, 2) == BSX_ERR_STATE   # 0 -> 1 after an add
        assert L.bsx_meth_set_ct_snp(h.h, 0) == 0
        plain = U.written_table(h, edges.dir / "state.txt")                                  # ... then add: the plain table
        assert plain == M.table(edges.names, K, 1, True, 0) and plain[0].startswith(M.HEADER9)
    with U.open_meth(edges.fa, 0, 1) as h:
        h.add(edges.alns[:50], 2)
        assert h.L.bsx_meth_set_ct_snp(h.h, 0) == BSX_ERR_STATE                   # 1 -> 0 after an add
        assert h.L.bsx_meth_set_ct_snp(h.h, 2) == 0 and h.L.bsx_meth_set_ct_snp(h.h, 3) == BSX_ERR_ARG   # 1 -> 2 after an add
        assert rows(h, 3) == M.rows(M.pileup(edges.refs, edges.alns[:50], 2), 1, True, 2)


# ---- 8. command line -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["bsp", "sam"])
def test_command_line(fmt, edges, tmp_path, capsys):
    from bsmap_amd import methratio
    path = str(tmp_path / ("in." + fmt))
    with open(path, "w") as f:
        if fmt == "sam":
            f.write("".join("@SQ\tSN:%s\tLN:%d\n" % (n, len(r)) for n, r in zip(edges.names, edges.refs)))
        for k, (c, pos, st, insert, cut, s) in enumerate(edges.alns):
            if fmt == "sam":  # PNEXT = cut_at + 1; 0 (with a positive insert: "no cut" in the C ABI) where the set has none
                f.write("r%d\t0\t%s\t%d\t255\t%dM\t=\t%d\t%d\t%s\t%s\tNM:i:0\tZS:Z:%s\n" % (k, edges.names[c], pos + 1, len(s), cut + 1, insert, s, "I" * len(s), STRANDS[st]))
            else:
                f.write("r%d\t%s\t%s\tUM\t%s\t%d\t%s\t%d\n" % (k, s, "I" * len(s), edges.names[c], pos + 1, STRANDS[st], insert))
    out = str(tmp_path / "t.txt")
    methratio.main(["-q", "-z", "-r", "-i", "correct", "-x", "CG,CHG", "-o", out, "-d", edges.fa, path])
    stdout, table = capsys.readouterr().out, open(out).read()
    alns = edges.alns if fmt == "sam" else [(c, pos, st, insert, -1, s) for c, pos, st, insert, cut, s in edges.alns]  # a BSP line carries no mate position
    K = M.pileup(edges.refs, alns, 2, True)
    want, nc, nd = M.table(edges.names, K, 1, True, 1, 3)
    assert table == want and stdout == M.summary(K.nmap, nc, nd) and nc > 50
    methratio.main(["-q", "-z", "-r", "-o", out, "-d", edges.fa, path])
    plain = (capsys.readouterr().out, open(out, "rb").read())
    methratio.main(["-q", "-z", "-r", "-i", "no-action", "-o", out, "-d", edges.fa, path])
    assert (capsys.readouterr().out, open(out, "rb").read()) == plain and plain[1].startswith(M.HEADER9.encode())


# ---- 9. the tie to the pinned reference tables ----------------------------------------------------------------------------------------------------------------
GOLD = json.load(gzip.open(os.path.join(G.GOLDEN, "methratio.json.gz"), "rt"))
RUNS = [(c, i) for c in sorted(GOLD["cases"]) for i in range(len(GOLD["cases"][c]["runs"]))]


@pytest.fixture(scope="module")
def gold_files(tmp_path_factory):
    import base64
    d = tmp_path_factory.mktemp("ctsnp_gold")
    fa = str(d / "g.fa")
    open(fa, "w").write(GOLD["fasta"])
    paths = {}
    for c, case in GOLD["cases"].items():
        for fn, txt in case["files"].items():
            open(str(d / fn), "w").write(txt)
        for fn, b64 in case.get("files_b64", {}).items():
            open(str(d / fn), "wb").write(base64.b64decode(b64))
        paths[c] = [str(d / fn) for fn in case["infiles"]]
    return fa, paths, d


@pytest.mark.parametrize("case,i", RUNS, ids=[f"{c}-{'_'.join(GOLD['cases'][c]['runs'][i]['options']) or 'default'}" for c, i in RUNS])
def test_tie_to_the_pinned_tables(case, i, gold_files, capsys):
    """-i correct on real bsmap output: what it lists is a subsequence of the v2.6 table with the same counts, and where the other strand shows
    no converted letter the row's ratio and interval are the v2.6 row's"""
    from bsmap_amd import methratio
    fa, paths, d = gold_files
    run = GOLD["cases"][case]["runs"][i]
    opts = list(run["options"])
    if "same_as" in run:  # a BAM twin of that case's SAM file: same expected output
        run = [r for r in GOLD["cases"][run["same_as"]]["runs"] if r["options"] == run["options"]][0]
    out = str(d / f"{case}_{i}.txt")
    methratio.main(["-q", "-o", out, "-d", fa] + opts + ["-i", "correct"] + paths[case])
    capsys.readouterr()
    lines = open(out).read().split("\n")
    assert lines[0] + "\n" == M.HEADER12 and lines[-1] == ""
    got = [l.split("\t") for l in lines[1:-1]]
    pinned = [l.split("\t") for l in run["table"].split("\n")[1:-1]]
    at = missing = same = 0
    for f in got:
        key = f[:4] + [f[7], f[6]]                     # chr, pos, strand, context, CT_count, C_count
        while at < len(pinned) and pinned[at][:4] + pinned[at][5:7] != key:
            at += 1
            missing += 1
        assert at < len(pinned), f"row {f} is not in the pinned table (in this order)"
        if f[8] == f[9]:
            same += 1
            assert (f[4], f[10], f[11]) == (pinned[at][4], pinned[at][7], pinned[at][8]) and f[5] == "%.2f" % int(pinned[at][5]), (f, pinned[at])
        at += 1
    missing += len(pinned) - at
    assert missing + len(got) == len(pinned) and 2 * missing < max(len(pinned), 1), f"{missing} of {len(pinned)} pinned rows are not listed"
    assert same > 0 or not pinned
