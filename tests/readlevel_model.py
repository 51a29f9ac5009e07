"""Pure-Python model of the per-read calls of bsmap_amd.methratio (--nonconv-filter, --read-stats, --pdr): the yardstick of
test_methratio_readlevel_cpu.py and test_gpu_methratio_readlevel.py.  A plain helper module, no test and no conftest.

On the alignment tuples of ctsnp_model.py, (chr id, 0-based pos, strand code, insert, cut_at or -1, letters) in input order:
  window     the reference script's per-alignment code (duplicates by fragment end, fill-in trim, cut_at, bounds) on Python's own slices
  call       a letter of the window over the read strand's own cytosine (C under '+?', G under '-?') that shows the unconverted or the converted
             letter, at a cycle that trim5 / trim3 do not mask; its class is context_class (0 CG, 1 CHG, 2 CHH, 3 other)
  counts     per valid alignment n_cg, m_cg (class 0, methylated among them) and n_ch, m_ch (classes 1 and 2 together); class 3 enters nothing
  filter     N >= 1: a valid alignment with m_ch >= N is dropped: no call of any kind, not a valid mapping; the duplicate filter has run before, on all
  histogram  every valid alignment, dropped ones included: cg[n_cg][m_cg] for n_cg <= 31, cg_over beyond, ch[min(m_ch, 63)], reads, ch_calls, ch_meth
  PDR        K >= 1: a valid, not dropped alignment with n_cg >= K is eligible, discordant when 0 < m_cg < n_cg; each of its CG calls adds (1, discordant)
             at the call's position; the CpG fold moves the G's cell of every in-chromosome CG onto its C; a row is a position with reads >= min_reads
It never looks at the library's output."""
from ctsnp_model import STRANDS, context_class

CG_MAX, CH_MAX = 31, 63
PDR_HEADER = "chr\tpos\tstrand\treads\tdiscordant\tPDR\n"
STATS_HEADER = "kind\tcalls\tmeth\treads\n"


def windows(refs, alns, trim_fillin=2, rm_dup=False):
    """per alignment None (not a valid mapping) or (pos, [(index in the untrimmed read, letter)]) of what survives"""
    coverage = [[0] * len(r) for r in refs]
    out = []
    for c, pos, st, insert, cut_at, letters in alns:
        strand = STRANDS[st]
        seq = list(enumerate(letters))
        if rm_dup:
            if strand == "+-" or strand == "-+":
                frag_end, direction = pos + len(seq), 2
            else:
                frag_end, direction = pos, 1
            if 0 <= frag_end < len(refs[c]):
                if coverage[c][frag_end] & direction:
                    out.append(None)
                    continue
                coverage[c][frag_end] |= direction
        if trim_fillin > 0:
            if strand == "+-":
                seq = seq[:-trim_fillin]
            elif strand == "--":
                seq, pos = seq[trim_fillin:], pos + trim_fillin
            elif insert != 0 and len(seq) > abs(insert) - trim_fillin:
                trim_nt = len(seq) - (abs(insert) - trim_fillin)
                if strand == "++":
                    seq = seq[:-trim_nt]
                elif strand == "-+":
                    seq, pos = seq[trim_nt:], pos + trim_nt
        if cut_at >= 0:
            seq = seq[:cut_at - pos]
        if pos + len(seq) > len(refs[c]):
            out.append(None)
            continue
        assert pos >= 0
        out.append((pos, seq))
    return out


def letters_of(refs, aln, win, trim5=0, trim3=0):
    """the unmasked letters of a valid alignment as (position, cycle, reference letter, read letter)"""
    c, _, st, _, _, letters = aln
    pos, seq = win
    n0 = len(letters)
    for k, (j, ch) in enumerate(seq):
        cycle = j if STRANDS[st] in ("++", "--") else n0 - 1 - j
        if cycle < trim5 or cycle >= n0 - trim3:
            continue
        yield pos + k, cycle, refs[c][pos + k], ch


def calls_of(refs, aln, win, trim5=0, trim3=0):
    """the calls of a valid alignment as (position, cycle, class, methylated)"""
    c, st = aln[0], aln[2]
    plus = STRANDS[st][0] == "+"
    match, convert = ("C", "T") if plus else ("G", "A")
    for g, cycle, r, ch in letters_of(refs, aln, win, trim5, trim3):
        if r == match and ch in (match, convert):
            yield g, cycle, context_class(refs[c], g, plus), ch == match


def counts_of(calls):
    n_cg = sum(1 for _, _, x, _ in calls if x == 0)
    m_cg = sum(1 for _, _, x, m in calls if x == 0 and m)
    n_ch = sum(1 for _, _, x, _ in calls if x in (1, 2))
    m_ch = sum(1 for _, _, x, m in calls if x in (1, 2) and m)
    return n_cg, m_cg, n_ch, m_ch


class Result:
    """counts: per alignment None or (n_cg, m_cg, n_ch, m_ch); verdict: per alignment 'invalid', 'dropped', 'discordant', 'concordant' or 'plain' (valid,
    kept, not eligible); kept: the indices of the valid, not dropped alignments; dropped, nmap; cg[32][32], cg_over, ch[64], reads, ch_calls, ch_meth;
    pdr: per chromosome lists of [reads, discordant]; depth, meth, rev_g, rev_ga: per chromosome lists; mbias: {(strand code, class, cycle, methylated): n}"""


def analyse(refs, alns, trim_fillin=2, rm_dup=False, trim5=0, trim3=0, nonconv=0, min_cpg=4):
    R = Result()
    R.refs = refs
    R.counts, R.verdict, R.kept = [], [], []
    R.dropped = R.nmap = R.cg_over = R.reads = R.ch_calls = R.ch_meth = 0
    R.cg = [[0] * (CG_MAX + 1) for _ in range(CG_MAX + 1)]
    R.ch = [0] * (CH_MAX + 1)
    R.pdr = [[[0, 0] for _ in r] for r in refs]
    R.depth, R.meth, R.rev_g, R.rev_ga = ([[0] * len(r) for r in refs] for _ in range(4))
    R.mbias = {}
    for i, (aln, win) in enumerate(zip(alns, windows(refs, alns, trim_fillin, rm_dup))):
        if win is None:
            R.counts.append(None)
            R.verdict.append("invalid")
            continue
        c, st = aln[0], aln[2]
        calls = list(calls_of(refs, aln, win, trim5, trim3))
        n_cg, m_cg, n_ch, m_ch = cnt = counts_of(calls)
        R.counts.append(cnt)
        R.reads += 1
        R.ch_calls += n_ch
        R.ch_meth += m_ch
        if n_cg <= CG_MAX:
            R.cg[n_cg][m_cg] += 1
        else:
            R.cg_over += 1
        R.ch[min(m_ch, CH_MAX)] += 1
        if nonconv and m_ch >= nonconv:
            R.dropped += 1
            R.verdict.append("dropped")
            continue
        R.nmap += 1
        R.kept.append(i)
        for g, cycle, x, m in calls:
            R.depth[c][g] += 1
            R.meth[c][g] += int(m)
            key = (st, x, cycle, int(m))
            R.mbias[key] = R.mbias.get(key, 0) + 1
        rc_match, rc_convert = ("G", "A") if STRANDS[st][0] == "+" else ("C", "T")
        for g, cycle, r, ch in letters_of(refs, aln, win, trim5, trim3):  # the reverse calls of the C/T-SNP mode
            if r == rc_match and ch in (rc_match, rc_convert):
                R.rev_ga[c][g] += 1
                R.rev_g[c][g] += int(ch == rc_match)
        if min_cpg and n_cg >= min_cpg:
            disc = 0 < m_cg < n_cg
            R.verdict.append("discordant" if disc else "concordant")
            for g, _, x, _ in calls:
                if x == 0:
                    R.pdr[c][g][0] += 1
                    R.pdr[c][g][1] += int(disc)
        else:
            R.verdict.append("plain")
    return R


def fold(refs, per_chr):
    """a folded copy of per-chromosome cells (numbers, or lists of numbers): every CG inside a chromosome gives its G's cell to its C"""
    out = []
    for ref, cells in zip(refs, per_chr):
        cells = [list(x) if isinstance(x, list) else x for x in cells]
        at = ref.find("CG")
        while at >= 0:
            if isinstance(cells[at], list):
                cells[at] = [a + b for a, b in zip(cells[at], cells[at + 1])]
                cells[at + 1] = [0] * len(cells[at])
            else:
                cells[at] += cells[at + 1]
                cells[at + 1] = 0
            at = ref.find("CG", at + 1)
        out.append(cells)
    return out


def pdr_rows(pdr, min_reads=1):
    """[(chr id, pos, reads, discordant)] in id and position order"""
    return [(c, i, r, d) for c, cells in enumerate(pdr) for i, (r, d) in enumerate(cells) if r >= min_reads]


def pdr_text(names, refs, pdr, min_reads=1):
    rows = pdr_rows(pdr, min_reads)
    out = [PDR_HEADER]
    for name, c in sorted((n, c) for c, n in enumerate(names)):
        for cc, i, r, d in rows:
            if cc == c:
                out.append("%s\t%d\t%s\t%d\t%d\t%.3f\n" % (name, i + 1, "+" if refs[c][i] == "C" else "-", r, d, float(d) / r))
    return "".join(out)


def read_stats_text(R):
    out = [STATS_HEADER]
    for n in range(CG_MAX + 1):
        for m in range(n + 1):
            if R.cg[n][m]:
                out.append("CG\t%d\t%d\t%d\n" % (n, m, R.cg[n][m]))
    out.append("CG\t>%d\t.\t%d\n" % (CG_MAX, R.cg_over))
    for k in range(CH_MAX):
        out.append("CH\t.\t%d\t%d\n" % (k, R.ch[k]))
    out.append("CH\t.\t%d+\t%d\n" % (CH_MAX, R.ch[CH_MAX]))
    out.append("# reads\t%d\n# CH calls\t%d\n# CH methylated\t%d\n" % (R.reads, R.ch_calls, R.ch_meth))
    out.append("# CH ratio\t%s\n" % ("%.5f" % (float(R.ch_meth) / R.ch_calls) if R.ch_calls else "NA"))
    return "".join(out)


def table_rows(R, depth=None, meth=None):
    """[(chr id, pos, depth, meth)] of the positions with depth > 0: the rows of bsx_meth_report_chr with min_depth 1 and meth0"""
    depth, meth = depth or R.depth, meth or R.meth
    return [(c, i, d, meth[c][i]) for c, dd in enumerate(depth) for i, d in enumerate(dd) if d > 0]
