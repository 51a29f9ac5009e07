"""bsmap_amd.methratio at the sizes where its untested branches live.  The golden fixtures stop at 8 738 table rows, depth 12 and
1.2 MB of input; here the inputs are generated (seeded numpy), the expected table AND summary line come from
oracle/methratio_oracle.py on the very same text (pinned to the reference script by tests/test_methratio_oracle.py, edge set
included), and both are compared as whole strings: every column is an integer or the same double arithmetic on the same integers.

Every fragment end (the slot of the duplicate filter) lies inside its chromosome, so that -r is defined by the reference."""
import os
import re

import numpy as np
import pytest

import meth_util as U
from oracle import methratio_oracle as MO

pytestmark = pytest.mark.gpu
STRANDS = ("++", "-+", "+-", "--")  # the library's strand codes 0..3


def _fasta(names, lens, genome):
    out, a = [], 0
    for n, l in zip(names, lens):
        s = genome[a:a + l].tobytes().decode()
        a += l
        out.append(">" + n + "\n" + "".join(s[i:i + 60] + "\n" for i in range(0, l, 60)))
    return "".join(out)


def _bisulfite(rng, genome, g0, L, st, sub=0.01, n_rate=0.003):
    """reads of lengths L at global offsets g0: C->T (reference strand '+', codes 0 and 2) or G->A on half of the sites"""
    so = np.concatenate([[0], np.cumsum(L)]).astype(np.int64)
    rid = np.repeat(np.arange(len(L)), L)
    g = np.minimum(g0[rid] + (np.arange(so[-1]) - so[rid]), len(genome) - 1)  # (a read that hangs over its chromosome's end: any letters)
    x = genome[g].copy()
    plus = (st[rid] & 1) == 0
    conv = rng.random(so[-1]) < 0.5
    x[plus & (x == ord("C")) & conv] = ord("T")
    x[~plus & (x == ord("G")) & conv] = ord("A")
    if sub:
        r = rng.random(so[-1])
        m = r < sub
        x[m] = rng.choice(np.frombuffer(b"ACGT", np.uint8), int(m.sum()))
        x[(r >= sub) & (r < sub + n_rate)] = ord("N")
    return x.tobytes(), so


def _lines(names, c, pos, st, ins, flag, seqs, so):
    """BSP lines (the eight columns the tool reads; NM lines have four, as bsmap writes them)"""
    c, pos, st, ins, so = c.tolist(), pos.tolist(), st.tolist(), ins.tolist(), so.tolist()
    qual = "I" * 200
    out = []
    for i in range(len(c)):
        s = seqs[so[i]:so[i + 1]].decode()
        if flag[i] == "NM":
            out.append("r%d\t%s\t%s\tNM\n" % (i, s, qual[:len(s)]))
        else:
            out.append("r%d\t%s\t%s\t%s\t%s\t%d\t%s\t%d\n" % (i, s, qual[:len(s)], flag[i], names[c[i]], pos[i] + 1, STRANDS[st[i]], ins[i]))
    return out


class Wide:
    """one chromosome of 400 000 letters among 300 contigs of 5-2 000, 200 000 alignments of 30-150 nt (a fifth of them placed on
    another alignment's fragment, 3 % hanging over the chromosome's end, 5 % NM lines)"""

    def __init__(self):
        rng = np.random.default_rng(7)
        n_ctg, n = 300, 200_000
        lens = rng.integers(5, 2001, n_ctg).tolist()
        self.i_long = 150  # the long chromosome in the middle of the offset table
        lens.insert(self.i_long, 400_000)
        self.names = ["ctg%03d" % i for i in range(n_ctg)]
        self.names.insert(self.i_long, "chrL")
        self.lens = np.array(lens, np.int64)
        self.off = np.concatenate([[0], np.cumsum(self.lens)])
        self.genome = rng.choice(np.frombuffer(b"ACGT", np.uint8), int(self.off[-1]))
        self.fasta = _fasta(self.names, lens, self.genome)
        c = np.where(rng.random(n) < 0.7, self.i_long, rng.integers(0, n_ctg + 1, n))
        L = np.minimum(rng.integers(30, 151, n), self.lens[c] - 1)
        st = rng.integers(0, 4, n)
        pos = np.floor(rng.random(n) * (self.lens[c] - L)).astype(np.int64)  # [0, clen-L-1]: the right end stays below clen-1
        over = ((st == 0) | (st == 3)) & (rng.random(n) < 0.03) & (L > 2)     # left-end fragments may hang over: skipped at methratio.py:102
        pos[over] = (self.lens[c] - 1 - np.floor(rng.random(n) * (L - 2)).astype(np.int64))[over]
        dup, src = rng.random(n) < 0.2, rng.integers(0, n, n)                 # same fragment, other letters: -r has to choose
        for a in (c, L, st, pos):
            a[dup] = a[src][dup]
        k = rng.integers(0, 7, n)
        ins = np.select([k == 0, k == 1, k == 2, k == 3, k == 4, k == 5], [0, L + 5, -(L + 5), 250, -250, L], L // 2)
        f = rng.random(n)
        self.flag = np.where(f < 0.85, "UM", np.where(f < 0.95, "MA", "NM")).tolist()
        seqs, so = _bisulfite(rng, self.genome, self.off[c] + pos, L, st)
        self.c, self.pos, self.st, self.ins, self.seqs, self.so = c, pos, st, ins.astype(np.int64), seqs, so
        self.lines = _lines(self.names, c, pos, st, self.ins, self.flag, seqs, so)
        self.text = "".join(self.lines)
        self._exp = {}

    def expected(self, opts, infiles=None):
        key = (tuple(opts), None if infiles is None else tuple(n for n, _ in infiles))
        if key not in self._exp:
            self._exp[key] = MO.run(self.fasta, infiles or [("wide.bsp", self.text)], MO.options_from_argv(list(opts)))
        return self._exp[key]


@pytest.fixture(scope="module")
def wide(tmp_path_factory):
    w = Wide()
    d = tmp_path_factory.mktemp("meth_wide")
    w.dir, w.fa, w.path = d, str(d / "wide.fa"), str(d / "wide.bsp")
    open(w.fa, "w").write(w.fasta)
    open(w.path, "w").write(w.text)
    return w


def _tool(fa, infiles, opts, out, capsys):
    from bsmap_amd import methratio
    capsys.readouterr()
    methratio.main(["-q", "-o", out, "-d", fa] + list(opts) + list(infiles))
    return open(out).read(), capsys.readouterr().out


def _rows(table, chrom=None):
    return [f for f in (l.split("\t") for l in table.split("\n")[1:] if l) if chrom is None or f[0] == chrom]


@pytest.mark.parametrize("opts", [("-z",), ("-z", "-r"), ("-g", "-z", "-m", "3")], ids=lambda o: "_".join(o))
def test_wide(opts, wide, capsys):
    """Reaches: k_meth_count / rocPRIM scan / k_meth_emit over 391 blocks of 1 024 positions (59 in the fixtures); more than one
    formatter thread in bsx_meth_write_table (one per 65 536 rows of a chromosome); one parser chunk per MB of input and the
    joining of their offset arrays in stream_text; the binary search of k_meth_cpg over 301 chromosomes; the `pos + len > clen`
    skip; k_meth_first over 190 000 alignments in one call."""
    table, summary = wide.expected(opts)
    assert len(_rows(table, "chrL")) > 65_536           # more than one formatter thread
    assert os.path.getsize(wide.path) > 16 << 20         # more than one parser chunk (one per MB, as many as CPUs)
    got, out = _tool(wide.fa, [wide.path], opts, str(wide.dir / "wide.txt"), capsys)
    assert got == table
    assert out == summary


def test_pieces(wide, capsys, tmp_path):
    """Reaches: the second 256 MB piece of the text path (bsx_meth_add_file -> stream_text), with first-wins order at stake: the
    wide file written seven times over.  Every alignment of copies 2-7 has its twin in copy 1, so with -r table and summary must be
    those of one copy."""
    table, summary = wide.expected(("-z", "-r"))
    big = str(tmp_path / "seven.bsp")
    try:
        data = wide.text.encode()
        with open(big, "wb") as f:
            for _ in range(7):
                f.write(data)
        assert os.path.getsize(big) > 256 << 20      # more than one piece
        got, out = _tool(wide.fa, [big], ("-z", "-r"), str(tmp_path / "seven.txt"), capsys)
    finally:
        if os.path.exists(big):
            os.remove(big)
    assert got == table
    assert out == summary


def test_three_files_in_an_order_that_matters(wide, capsys, tmp_path):
    """Reaches: the duplicate filter's index base across bsx_meth_add_file calls.  The lines dealt out over three files, read in an
    order that is not the one file's: other alignments come first, -r keeps other letters"""
    parts = [("b.bsp", "".join(wide.lines[2::3])), ("c.bsp", "".join(wide.lines[0::3])), ("a.bsp", "".join(wide.lines[1::3]))]
    table, summary = wide.expected(("-z", "-r"), parts)
    assert table != wide.expected(("-z", "-r"))[0]      # the order matters
    paths = []
    for n, t in parts:
        paths.append(str(tmp_path / n))
        open(paths[-1], "w").write(t)
    got, out = _tool(wide.fa, paths, ("-z", "-r"), str(tmp_path / "three.txt"), capsys)
    assert got == table
    assert out == summary


def test_calls(wide):
    """Reaches: first-wins across bsx_meth_add calls: the wide alignments as arrays in batches of 1, 53, 4 099 and the remaining
    ~186 000, duplicate removal on; rows and the count of valid mappings are the file path's (= the oracle's -z -r)"""
    from bsmap_amd.methratio import Meth
    table, summary = wide.expected(("-z", "-r"))
    with Meth.from_lengths(wide.lens, rm_dup=True) as m:
        for i in range(len(wide.names)):
            m.set_reference(i, wide.genome[wide.off[i]:wide.off[i + 1]])
        keep = np.array([f != "NM" for f in wide.flag])
        idx = np.nonzero(keep)[0]
        assert len(idx) > 180_000
        b0 = 0
        for size in (1, 53, 4099, len(idx)):
            part = idx[b0:b0 + size]
            b0 += len(part)
            seq = b"".join(wide.seqs[wide.so[i]:wide.so[i + 1]] for i in part.tolist()) + b"\0"
            off = np.concatenate([[0], np.cumsum(wide.so[part + 1] - wide.so[part])]).astype(np.uint64)
            m.add_arrays(len(part), wide.c[part].astype(np.uint32), wide.pos[part].astype(np.int64), wide.st[part].astype(np.uint8), wide.ins[part].astype(np.int32),
                         np.full(len(part), -1, np.int64), np.frombuffer(seq, np.uint8), off, 2)
        assert b0 == len(idx)
        got = [(wide.names[c], pos + 1, dep, met) for c, pos, dep, met in U.table_rows(m, len(wide.names))[0]]
        nmap = m.valid_mappings()
    exp = [(f[0], int(f[1]), int(f[5]), int(f[6])) for f in _rows(table)]
    assert sorted(got) == sorted(exp) and len(got) > 200_000
    assert nmap == int(re.match(r"total (\d+) valid mappings", summary).group(1))


class Deep:
    """70 000 alignments on one start position — all four strands, 68 000 of them on the '+' reference strand, every site
    methylated in about half of them — and 70 000 copies of one '++' fragment on another chromosome, shuffled into one file"""

    def __init__(self):
        rng = np.random.default_rng(11)
        self.names, lens = ["chrD", "chrE"], [3000, 2000]
        genome = rng.choice(np.frombuffer(b"ACGT", np.uint8), 5000)
        self.fasta = _fasta(self.names, lens, genome)
        n = 70_000
        st = np.concatenate([np.repeat([0, 2, 1, 3], [40_000, 28_000, 1_000, 1_000]), np.zeros(n, np.int64)])
        c = np.concatenate([np.zeros(n, np.int64), np.ones(n, np.int64)])
        pos = np.where(c == 0, 1000, 500)
        L = np.where(c == 0, 100, 80)
        order = rng.permutation(2 * n)
        c, st, pos, L = c[order], st[order], pos[order], L[order]
        seqs, so = _bisulfite(rng, genome, np.array([0, 3000])[c] + pos, L, st, sub=0)
        self.text = "".join(_lines(self.names, c, pos, st, np.zeros(2 * n, np.int64), ["UM"] * (2 * n), seqs, so))


@pytest.fixture(scope="module")
def deep(tmp_path_factory):
    dp = Deep()
    d = tmp_path_factory.mktemp("meth_deep")
    dp.dir, dp.fa, dp.path = d, str(d / "deep.fa"), str(d / "deep.bsp")
    open(dp.fa, "w").write(dp.fasta)
    open(dp.path, "w").write(dp.text)
    return dp


@pytest.mark.parametrize("opts", [("-z",), ("-g", "-z"), ("-z", "-r")], ids=lambda o: "_".join(o))
def test_deep(opts, deep, capsys):
    """Reaches: u32 counters above 65 535 — 68 000 waves' atomicAdd on the same depth / methylated words, k_meth_cpg's sums of two
    such counters, the %u columns and the confidence interval at that depth; with -r 70 000 atomicMin on one fragment-end slot per
    direction, of which the alignment that comes first in the file must win (the letters differ from copy to copy)."""
    table, summary = MO.run(deep.fasta, [("deep.bsp", deep.text)], MO.options_from_argv(list(opts)))
    depth = max(int(f[5]) for f in _rows(table))
    if "-r" in opts:
        assert depth <= 2       # one alignment per fragment end and direction survives
    else:
        assert depth > 65_535
    got, out = _tool(deep.fa, [deep.path], opts, str(deep.dir / "deep.txt"), capsys)
    assert got == table
    assert out == summary
