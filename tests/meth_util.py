"""What the GPU tests of bsmap_amd.methratio need on top of its Meth class: a handle with the settings of one test, and the reports of all sequences as the
lists of tuples the pure-Python models give."""
import numpy as np

import diff_model as D
from bsmap_amd.methratio import Meth


def open_meth(fa, rm_dup=False, snp=0, mbias=False, trim=None, nonconv=0, stats=False, min_cpg=0, epi=False):
    """Meth.from_fasta with the settings made in this order: C/T-SNP mode, M-bias, (trim5, trim3), non-conversion filter, histogram, PDR, epialleles"""
    m = Meth.from_fasta(fa, rm_dup=rm_dup)
    try:
        if snp:
            m.set_ct_snp(snp)
        if mbias:
            m.set_mbias()
        if trim:
            m.set_cycle_trim(*trim)
        if nonconv:
            m.set_nonconv(nonconv)
        if stats:
            m.set_read_stats()
        if min_cpg:
            m.set_pdr(min_cpg)
        if epi:
            m.set_epi()
    except BaseException:
        m.close()
        raise
    return m


def table_rows(m, n_chr, min_depth=1, meth0=1, snp=False, pad=False):
    """([(chr id, pos, depth, meth)], n_covered, sum_depth) over the sequences 0 .. n_chr - 1; with snp=True the rows end in rev_g, rev_ga, and with
    pad=True they do so with the mode off too, as 0, 0"""
    got, nc, nd = [], 0, 0
    for c in range(n_chr):
        *cols, cov, sd = m.report(c, min_depth, meth0, snp)
        cols = [x.tolist() for x in cols]
        if pad and not snp:
            cols += [[0] * len(cols[0])] * 2
        got += [(c,) + t for t in zip(*cols)]
        nc, nd = nc + cov, nd + sd
    return got, nc, nd


def rows_and_rev(m, n_chr, snp=0):
    """[(chr id, pos, depth, meth)] with min_depth 1 and meth0, and with the C/T-SNP mode on (snp) [(chr id, pos, rev_g, rev_ga)] of the same rows, else []"""
    got = table_rows(m, n_chr, snp=bool(snp))[0]
    return [r[:4] for r in got], [r[:2] + r[4:] for r in got] if snp else []


def read_hist(m):
    """(cg as nested lists, ch as a list, (reads, cg_over, ch_calls, ch_meth))"""
    cg, ch, tot = m.read_stats()
    return cg.tolist(), ch.tolist(), tot


def mbias_cells(m):
    """({(strand, context, cycle, methylated): count} of the non-zero M-bias cells, calls beyond the last cycle)"""
    cells, over = m.mbias()
    return {(int(s), int(x), int(cyc), int(k)): int(cells[s, x, cyc, k]) for s, x, cyc, k in zip(*np.nonzero(cells))}, over


def pdr_rows(m, n_chr, min_reads=1):
    """[(chr id, pos, reads, discordant)], the form of readlevel_model.pdr_rows"""
    return [(c,) + t for c in range(n_chr) for t in zip(*[x.tolist() for x in m.pdr_report(c, min_reads)])]


def epi_rows(m, n_chr, min_reads=1):
    """[(chr id, (four 0-based C positions), [16 counts])], the form of epi_model.epi_rows"""
    got = []
    for c in range(n_chr):
        pos, counts = m.epi_report(c, min_reads)
        got += [(c, tuple(p), n) for p, n in zip(pos.tolist(), counts.tolist())]
    return got


def joined(a, b, c, min_depth, permille=0):
    """the model of the two-sample rows of sequence c: [(pos0, mA, dA, mB, dB)] from the pinned single-sample reports of a and b"""
    pa, da, ma, _, _ = a.report(c, min_depth, True)
    pb, db, mb, _, _ = b.report(c, min_depth, True)
    sb = {int(p): (int(m), int(d)) for p, d, m in zip(pb, db, mb) if d > 0}
    rows = [(int(p), int(m), int(d)) + sb[int(p)] for p, d, m in zip(pa, da, ma) if d > 0 and int(p) in sb]
    return [r for r in rows if D.delta_keeps(*r[1:], permille)]


def interval_sums(rows_by_chr, lens, ivs):
    """[[N, MA, DA, MB, DB]] of the intervals [(chr id, start, end)] over the rows of joined(), the ends clipped to the sequences' lengths"""
    out = []
    for c, s, e in ivs:
        e = min(e, lens[c])
        inside = [r for r in rows_by_chr[c] if min(s, e) <= r[0] < e]
        out.append([len(inside)] + [sum(r[k] for r in inside) for k in (1, 2, 3, 4)])
    return out


def read_text(path):
    """a written file as str, line ends as they are"""
    return open(path, "rb").read().decode()


def written_table(m, path, min_depth=1, meth0=1):
    """(the table file's text, n_covered, sum_depth)"""
    nc, nd = m.write_table(path, min_depth, meth0)
    return read_text(path), nc, nd


def write_fasta(path, names, refs):
    with open(path, "w") as f:
        for n, s in zip(names, refs):
            f.write(">%s some text\n%s" % (n, "".join(s[i:i + 50] + "\n" for i in range(0, len(s), 50))))
    return str(path)
