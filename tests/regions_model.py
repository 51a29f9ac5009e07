"""Pure-Python model of the pooled methylation per interval and per bin of bsmap_amd.methratio (--regions / --region-out, -w / -b;
bsx_meth_regions, bsx_meth_bins, bsx_meth_write_regions, bsx_meth_write_wig): the yardstick of test_methratio_regions_cpu.py,
test_regions_parse_cpu.py and test_gpu_methratio_regions.py.  A plain helper module, no test and no conftest.

The pile-up, the CpG fold, the row rule and the table's effective depth are those of ctsnp_model.py; this module adds
  site       a position the row rule covers (covered(): min_depth, context mask, SNP mode) whose raw depth is above 0; -z plays no part
  per site   e = d << 16, or with a mode on and g != ga round-to-even of effective()'s depth times 65536; mc = min(m << 16, e)
  sums       N (sites), M, D, E, MC over the sites of an interval, plain loops over its positions
  bins       per chromosome, bin j = [j B, min((j + 1) B, len)), len // B + 1 of them
  ratio      float(MC) / float(E); the effective depth E / 65536.0; the Wilson interval of the table over those two
  files      the wiggle text, the region text and the BED parse as the library's header defines them
It never looks at the library's output."""
import re

import ctsnp_model as M

REGION_HEADER = "chr\tstart\tend\tname\tn_C\tmethy_C\ttotal_C\teff_CT\tratio\tCI_lower\tCI_upper\n"


def site(K, c, i, min_depth, mode, mask):
    """None, or (1, m, d, e, mc) of position i of chromosome c"""
    dd, m, g, ga = K.depth[c][i], K.meth[c][i], K.rev_g[c][i], K.rev_ga[c][i]
    if dd <= 0 or not M.covered(K.refs[c], i, dd, g, ga, min_depth, mode, mask):
        return None
    e = dd << 16
    if mode and g != ga:
        e = int(round(M.effective(dd, m, g, ga)[0] * 65536.0))  # round(): to nearest, ties to even
    return (1, m, dd, e, min(m << 16, e))


def site_table(K, min_depth=1, mode=0, mask=0):
    """per chromosome, per position: None or the site's (1, m, d, e, mc).  What the functions below sum over"""
    return [[site(K, c, i, min_depth, mode, mask) for i in range(len(ref))] for c, ref in enumerate(K.refs)]


def interval_sums(S, c, start, end):
    """[N, M, D, E, MC] of [start, end) of chromosome c; end beyond the chromosome is clipped, then start to end"""
    end = min(end, len(S[c]))
    start = min(start, end)
    s = [0] * 5
    for i in range(start, end):
        if S[c][i]:
            s = [a + b for a, b in zip(s, S[c][i])]
    return s


def bin_sums(S, c, B):
    """the len // B + 1 bins of chromosome c, each [N, M, D, E, MC]"""
    out = [[0] * 5 for _ in range(len(S[c]) // B + 1)]
    for i, v in enumerate(S[c]):
        if v:
            out[i // B] = [a + b for a, b in zip(out[i // B], v)]
    return out


def ratio(s):
    return float(s[4]) / float(s[3])


def wig_text(names, S, B):
    out = ["track type=wiggle_0\n"]
    for name, c in sorted((n, c) for c, n in enumerate(names)):
        out.append("variableStep chrom=%s span=%d\n" % (name, B))
        for j, s in enumerate(bin_sums(S, c, B)):
            if s[0] > 0 and s[3] > 0:
                out.append("%d\t%.3f\n" % (j * B + 1, ratio(s)))
    return "".join(out)


def region_fields(s):
    """the columns from n_C on"""
    d = float(s[3]) / 65536.0
    if s[0] == 0 or s[3] == 0:
        return "%d\t%d\t%d\t%.2f\tNA\tNA\tNA" % (s[0], s[1], s[2], d)
    z95, z95sq = 1.96, 1.96 * 1.96
    r = ratio(s)
    pmid = r + z95sq / (2 * d)
    sd = z95 * ((r * (1 - r) / d + z95sq / (4 * d * d)) ** 0.5)
    norminator = 1 + z95sq / d
    return "%d\t%d\t%d\t%.2f\t%.3f\t%.3f\t%.3f" % (s[0], s[1], s[2], d, r, (pmid - sd) / norminator, (pmid + sd) / norminator)


def parse_bed(text, names, lens):
    """-> ([(chr id, start, end, label)] in the file's order, number of dropped records), or the 1-based number of the first bad line.
    text: the file's bytes as a latin-1 string"""
    recs, dropped = [], 0
    lines = text.split("\n")
    if lines and lines[-1] == "":
        lines.pop()  # the text behind the last newline is a line only if there is any
    for no, line in enumerate(lines, 1):
        if line.endswith("\r"):
            line = line[:-1]
        if line == "" or line[0] == "#" or line.startswith("track") or line.startswith("browser"):
            continue
        col = [x for x in re.split("[ \t]+", line) if x != ""]
        if not col:
            continue
        if len(col) < 3 or not all(re.fullmatch("[0-9]{1,18}", x) for x in col[1:3]) or int(col[1]) > int(col[2]):
            return no
        if col[0] not in names:
            dropped += 1
            continue
        c = names.index(col[0])
        end = min(int(col[2]), lens[c])
        recs.append((c, min(int(col[1]), end), end, col[3] if len(col) > 3 else "."))
    return recs, dropped


def region_text(names, S, recs):
    out = [REGION_HEADER]
    for c, start, end, label in recs:
        out.append("%s\t%d\t%d\t%s\t%s\n" % (names[c], start, end, label, region_fields(interval_sums(S, c, start, end))))
    return "".join(out)
