"""Pure-Python model of the epiallele table of bsmap_amd.methratio (--epi): the yardstick of test_methratio_epi_cpu.py and
test_gpu_methratio_epi.py.  A plain helper module, no test and no conftest.  Windows, calls, classes and the non-conversion filter are those of
readlevel_model.py (windows / calls_of / analyse).

  reference CpG   a position p with ref[p] == 'C' and ref[p + 1] == 'G', both inside the chromosome; its ordinal is its index among them in position order
  CpGs of a read  for a valid, not dropped alignment with window [pos, pos + len): the reference CpGs whose call position (p under '+?', p + 1 under '-?')
                  lies in the window; they have consecutive ordinals
  state           M: a class-0 call there with the unconverted letter, U: with the converted letter, X: anything else (another letter, N, a masked cycle)
  window o        the CpGs o .. o+3 of one chromosome; a read adds 1 to cell[o][pattern] when all four are CpGs of the read and none is X; bit j of the
                  pattern (j = 0: the leftmost) is set when CpG o+j is M
  row             a window whose cells sum to at least min_reads, in chromosome order, then in ordinal order
It never looks at the library's output."""
import math

import readlevel_model as RL

PATTERNS = ["".join("M" if (k >> j) & 1 else "U" for j in range(4)) for k in range(16)]
EPI_HEADER = "chr\tpos1\tpos2\tpos3\tpos4\treads\tmeth\tmean\tepipoly\tentropy\t" + "\t".join(PATTERNS) + "\n"


def cpgs(refs):
    """per chromosome the positions of the C of every reference CpG, ascending"""
    return [[p for p in range(len(r) - 1) if r[p] == "C" and r[p + 1] == "G"] for r in refs]


def states_of(refs, alns, trim_fillin=2, rm_dup=False, trim5=0, trim3=0, nonconv=0):
    """per alignment None (not valid, or dropped) or [(ordinal, 'M' | 'U' | 'X')] of the CpGs of the read"""
    sites = cpgs(refs)
    R = RL.analyse(refs, alns, trim_fillin, rm_dup, trim5, trim3, nonconv, 0)
    kept = set(R.kept)
    out = []
    for i, (aln, win) in enumerate(zip(alns, RL.windows(refs, alns, trim_fillin, rm_dup))):
        if win is None or i not in kept:
            out.append(None)
            continue
        c, plus = aln[0], RL.STRANDS[aln[2]][0] == "+"
        pos, seq = win
        calls = {g: m for g, _, x, m in RL.calls_of(refs, aln, win, trim5, trim3) if x == 0}
        st = []
        for o, p in enumerate(sites[c]):
            at = p if plus else p + 1
            if pos <= at < pos + len(seq):
                st.append((o, "X" if at not in calls else "M" if calls[at] else "U"))
        assert [o for o, _ in st] == list(range(st[0][0], st[0][0] + len(st))) if st else True
        out.append(st)
    return out


def epi_cells(refs, alns, trim_fillin=2, rm_dup=False, trim5=0, trim3=0, nonconv=0):
    """per chromosome {ordinal of the window's first CpG: [16 counts]}"""
    cells = [{} for _ in refs]
    for aln, st in zip(alns, states_of(refs, alns, trim_fillin, rm_dup, trim5, trim3, nonconv)):
        if st is None:
            continue
        for a in range(len(st) - 3):
            four = st[a:a + 4]
            if any(s == "X" for _, s in four):
                continue
            pattern = sum(1 << j for j, (_, s) in enumerate(four) if s == "M")
            cells[aln[0]].setdefault(four[0][0], [0] * 16)[pattern] += 1
    return cells


def epi_rows(cells, refs, min_reads=1):
    """[(chr id, (four 0-based C positions), [16 counts])] in chromosome and ordinal order"""
    sites = cpgs(refs)
    return [(c, tuple(sites[c][o:o + 4]), list(cells[c][o])) for c in range(len(refs)) for o in sorted(cells[c]) if sum(cells[c][o]) >= min_reads]


def scores(counts):
    """(reads, methylated calls, mean, epipolymorphism, entropy) of sixteen counts with a sum above 0"""
    reads = sum(counts)
    meth = sum(bin(k).count("1") * n for k, n in enumerate(counts))
    p = [n / reads for n in counts if n]
    return reads, meth, meth / (4.0 * reads), 1.0 - sum(x * x for x in p), 0.25 * sum(-x * math.log2(x) for x in p) + 0.0


def row_text(name, pos, counts):
    """the file's line for one window: pos the four 0-based positions"""
    reads, meth, mean, epipoly, entropy = scores(counts)
    return "%s\t%s\t%d\t%d\t%.3f\t%.4f\t%.4f\t%s\n" % (name, "\t".join(str(p + 1) for p in pos), reads, meth, mean, epipoly, entropy, "\t".join(map(str, counts)))


def epi_text(names, refs, cells, min_reads=1):
    rows = epi_rows(cells, refs, min_reads)
    out = [EPI_HEADER]
    for name, c in sorted((n, c) for c, n in enumerate(names)):
        out += [row_text(name, pos, counts) for cc, pos, counts in rows if cc == c]
    return "".join(out)


DERIVED = {7: 1e-3, 8: 1e-4, 9: 1e-4}   # the columns mean, epipolymorphism, entropy and one unit of their last printed place


def same_text(got, want):
    """the comparison rule of the epiallele file: the header and the integer columns byte for byte, the three derived columns within one unit of their last
    printed place (each side rounds by at most half a unit: nothing tighter holds across two libm / printf paths)"""
    g, w = got.split("\n"), want.split("\n")
    if len(g) != len(w) or g[0] != w[0] or g[-1] != "" or w[-1] != "":
        return False
    for a, b in zip(g[1:-1], w[1:-1]):
        a, b = a.split("\t"), b.split("\t")
        if len(a) != 26 or len(b) != 26:
            return False
        for k, (x, y) in enumerate(zip(a, b)):
            if k in DERIVED:
                # (in whole units of the last place, so that the binary form of the printed numbers plays no part)
                if len(x.split(".")[-1]) != len(y.split(".")[-1]) or abs(round(float(x) / DERIVED[k]) - round(float(y) / DERIVED[k])) > 1:
                    return False
            elif x != y:
                return False
    return True
