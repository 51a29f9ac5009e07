"""Pure-Python model of the C/T-SNP correction (-i) and the context filter (-x) of bsmap_amd.methratio: the yardstick of
test_methratio_ctsnp_cpu.py and test_gpu_methratio_ctsnp.py.  A plain helper module, no test and no conftest.

It restates the reference script's per-alignment code (its methratio.py:31-65 and :100-113) on parsed tuples with Python's own slices, as model() of
test_gpu_methratio_mbias.py does, and adds the rules of this feature:
  reverse calls  a '+' read over a reference G that shows G counts in rev_G and rev_GA, one that shows A in rev_GA; a '-' read over a reference C
                 likewise with C and T.  Same window (duplicates, fill-in trim, cut_at, bounds) and same cycle mask as the forward calls.
  CpG fold       the G of every in-chromosome CG gives all four counters to its C
  row rule       depth >= min_depth; context class in the mask; mode 2: rev_G == rev_GA, mode 1: not (rev_G == 0 < rev_GA), both: depth > 0;
                 then the position is covered (n_covered += 1, sum_depth += the raw depth); listed if methylated > 0 or meth0
  table          eff = depth * rev_G / rev_GA if rev_G != rev_GA else depth; ratio = min(methylated, eff) / eff; Wilson interval over eff
It never looks at the library's output."""

STRANDS = ("++", "-+", "+-", "--")  # the library's strand codes 0..3
MODES = ("no-action", "correct", "skip")
HEADER9 = "chr\tpos\tstrand\tcontext\tratio\ttotal_C\tmethy_C\tCI_lower\tCI_upper\n"
HEADER12 = "chr\tpos\tstrand\tcontext\tratio\teff_CT_count\tC_count\tCT_count\trev_G_count\trev_GA_count\tCI_lower\tCI_upper\n"


def context_class(refseq, g, plus):
    """0 CG, 1 CHG, 2 CHH, 3 other, of the cytosine at refseq[g] ('C' looks at the next two letters, 'G' at the previous two)"""
    if plus:
        n1 = refseq[g + 1] if g + 1 < len(refseq) else ""
        n2 = refseq[g + 2] if g + 2 < len(refseq) else ""
        gl, h = "G", "ACT"
    else:
        n1 = refseq[g - 1] if g - 1 >= 0 else ""
        n2 = refseq[g - 2] if g - 2 >= 0 else ""
        gl, h = "C", "AGT"
    if n1 == gl:
        return 0
    if n1 and n1 in h:
        if n2 == gl:
            return 1
        if n2 and n2 in h:
            return 2
    return 3


class Counters:
    """depth, meth, rev_g, rev_ga: per chromosome lists; nmap: valid mappings"""
    def __init__(self, refs):
        self.refs = refs
        self.depth, self.meth, self.rev_g, self.rev_ga = ([[0] * len(r) for r in refs] for _ in range(4))
        self.nmap = 0

    def copy(self):
        o = Counters(self.refs)
        for f in ("depth", "meth", "rev_g", "rev_ga"):
            setattr(o, f, [list(x) for x in getattr(self, f)])
        o.nmap = self.nmap
        return o


def pileup(refs, alns, trim_fillin=2, rm_dup=False, trim5=0, trim3=0):
    """refs: upper-case chromosome strings in id order; alns: (chr id, 0-based pos, strand code, insert, cut_at or -1, letters) in input order"""
    K = Counters(refs)
    coverage = [[0] * len(r) for r in refs]
    for c, pos, st, insert, cut_at, letters in alns:
        strand, n0 = STRANDS[st], len(letters)
        seq = list(enumerate(letters))  # (index in the untrimmed read, letter): sliced like the script slices its string
        if rm_dup:
            if strand == "+-" or strand == "-+":
                frag_end, direction = pos + len(seq), 2
            else:
                frag_end, direction = pos, 1
            if 0 <= frag_end < len(refs[c]):
                if coverage[c][frag_end] & direction:
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
            continue
        K.nmap += 1
        assert pos >= 0
        if strand[0] == "+":
            match, convert, rc_match, rc_convert = "C", "T", "G", "A"
        else:
            match, convert, rc_match, rc_convert = "G", "A", "C", "T"
        for k, (j, ch) in enumerate(seq):
            g = pos + k
            cycle = j if strand in ("++", "--") else n0 - 1 - j
            if cycle < trim5 or cycle >= n0 - trim3:
                continue  # a masked cycle makes no call of any kind
            r = refs[c][g]
            if r == match:
                if ch == match:
                    K.depth[c][g] += 1
                    K.meth[c][g] += 1
                elif ch == convert:
                    K.depth[c][g] += 1
            elif r == rc_match:
                if ch == rc_match:
                    K.rev_g[c][g] += 1
                    K.rev_ga[c][g] += 1
                elif ch == rc_convert:
                    K.rev_ga[c][g] += 1
    return K


def combine_cpg(K):
    """a folded copy: every CG inside a chromosome (occurrences cannot overlap), all four counters"""
    K = K.copy()
    for c, ref in enumerate(K.refs):
        pos = ref.find("CG")
        while pos >= 0:
            for a in (K.depth[c], K.meth[c], K.rev_g[c], K.rev_ga[c]):
                a[pos] += a[pos + 1]
                a[pos + 1] = 0
            pos = ref.find("CG", pos + 1)
    return K


def covered(ref, i, dd, g, ga, min_depth, mode, mask):
    if dd < min_depth:
        return False
    if mask not in (0, 0xF):
        if ref[i] not in "CG" or not (mask >> context_class(ref, i, ref[i] == "C")) & 1:
            return False
    if mode == 2 and g != ga:
        return False
    if mode == 1 and g == 0 and ga > 0:
        return False
    if mode in (1, 2) and dd == 0:
        return False
    return True


def rows(K, min_depth=1, meth0=True, mode=0, mask=0):
    """[(chr id, pos, dd, m, g, ga)] in id and position order, n_covered, sum_depth"""
    out, nc, nd = [], 0, 0
    for c, ref in enumerate(K.refs):
        for i in range(len(ref)):
            dd, m, g, ga = K.depth[c][i], K.meth[c][i], K.rev_g[c][i], K.rev_ga[c][i]
            if not covered(ref, i, dd, g, ga, min_depth, mode, mask):
                continue
            nc += 1
            nd += dd
            if m == 0 and not meth0:
                continue
            out.append((c, i, dd, m, g, ga))
    return out, nc, nd


def effective(dd, m, g, ga):
    """eff and ratio of a listed row, in the table's operation order"""
    eff = (float(dd) * g) / ga if g != ga else float(dd)
    return eff, (float(m) if float(m) < eff else eff) / eff


def row_fields(dd, m, g, ga, mode):
    """the columns from `ratio` on"""
    z95, z95sq = 1.96, 1.96 * 1.96
    if mode:
        d, ratio = effective(dd, m, g, ga)
    else:
        d = float(dd)
        ratio = float(m) / d
    pmid = ratio + z95sq / (2 * d)
    sd = z95 * ((ratio * (1 - ratio) / d + z95sq / (4 * d * d)) ** 0.5)
    norminator = 1 + z95sq / d
    lo, hi = (pmid - sd) / norminator, (pmid + sd) / norminator
    if mode:
        return "%.3f\t%.2f\t%d\t%d\t%d\t%d\t%.3f\t%.3f" % (ratio, d, m, dd, g, ga, lo, hi)
    return "%.3f\t%d\t%d\t%.3f\t%.3f" % (ratio, dd, m, lo, hi)


def table(names, K, min_depth=1, meth0=True, mode=0, mask=0):
    """the table text (chromosomes in sorted name order), n_covered, sum_depth"""
    listed, nc, nd = rows(K, min_depth, meth0, mode, mask)
    by_chr = {}
    for r in listed:
        by_chr.setdefault(r[0], []).append(r)
    out = [HEADER12 if mode else HEADER9]
    for name, c in sorted((n, c) for c, n in enumerate(names)):
        ref = K.refs[c]
        for _, i, dd, m, g, ga in by_chr.get(c, []):
            out.append("%s\t%d\t%s\t%s\t%s\n" % (name, i + 1, "+" if ref[i] == "C" else "-", ref[i - 2:i + 3], row_fields(dd, m, g, ga, mode)))
    return "".join(out), nc, nd


def summary(nmap, nc, nd):
    if nc == 0:
        return "total %d valid mappings, 0 covered cytosines.\n" % nmap
    return "total %d valid mappings, %d covered cytosines, average coverage: %.2f fold.\n" % (nmap, nc, float(nd) / nc)
