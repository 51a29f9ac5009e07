// bsx_meth_text.h — the rows of the methratio text files as plain C++, no device code: tests/harness/meth_text_check.cpp compiles them on their own under
// the host sanitizers.  The table (bsx_meth_write_table, 9 columns, or 12 with the C/T-SNP mode on), the region file and the wiggle track
// (bsx_meth_write_regions, bsx_meth_write_wig; §3.9) and the PDR file (bsx_meth_write_pdr; §3.10).  The epiallele rows are in bsx_meth_epi.h.
// Every function appends one line to `o`; the sequence name goes in as it is, whatever its length, and only the numbers pass through a fixed buffer.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>

namespace bsx_meth_text {

// The Wilson score interval of methratio.py:141-145 for a ratio over the depth d, with the reference's expressions in the reference's order (its `** 0.5`
// is pow(x, 0.5) here): the table's rows and the region file share it, so their last printed digits agree.
struct Interval { double lo, hi; };
static inline Interval wilson(double ratio, double d)
{
    const double z95 = 1.96, z95sq = 1.96 * 1.96;
    const double pmid = ratio + z95sq / (2 * d);
    const double sd = z95 * pow(ratio * (1 - ratio) / d + z95sq / (4 * d * d), 0.5);
    const double norminator = 1 + z95sq / d;
    return Interval{(pmid - sd) / norminator, (pmid + sd) / norminator};
}

// A table row: pos0 the 0-based position, ctx the packed context of k_meth_emit (bytes 0..4 the letters of refcr[i-2:i+3], zero-ended; byte 7 the letter at
// i).  With snp the 12-column row of later BSMAP releases: d is the effective depth, the share of the raw depth that the opposite strand shows to be a real C
// (rev_g of rev_ga calls), and the methylated count is clipped to it.
static inline void append_table_row(std::string &o, const char *name, uint32_t pos0, uint32_t depth, uint32_t meth, uint64_t ctx, bool snp, uint32_t rev_g, uint32_t rev_ga)
{
    const double d = (snp && rev_g != rev_ga) ? ((double)depth * rev_g) / rev_ga : (double)depth, mm = meth;
    const double ratio = snp ? (mm < d ? mm : d) / d : mm / d;
    const Interval ci = wilson(ratio, d);
    char cx[8];
    int nb = 0;
    for (; nb < 5; nb++) { const char ch = (char)((ctx >> (8 * nb)) & 0xff); if (!ch) break; cx[nb] = ch; }
    cx[nb] = 0;
    const char strand = (char)(ctx >> 56) == 'C' ? '+' : '-';
    char num[192];
    o += name;
    if (snp) o.append(num, (size_t)snprintf(num, sizeof(num), "\t%u\t%c\t%s\t%.3f\t%.2f\t%u\t%u\t%u\t%u\t%.3f\t%.3f\n", pos0 + 1, strand, cx, ratio, d, meth, depth, rev_g, rev_ga, ci.lo, ci.hi));
    else o.append(num, (size_t)snprintf(num, sizeof(num), "\t%u\t%c\t%s\t%.3f\t%u\t%u\t%.3f\t%.3f\n", pos0 + 1, strand, cx, ratio, depth, meth, ci.lo, ci.hi));
}

// A row of the region file over the interval's sums s = [N, M, D, E, MC] (E and MC in units of 1/65536): the table's interval over the pooled effective depth;
// NA where there is no ratio (no site, or E == 0 with a site: d * g / ga below 2^-17, no real pile-up)
static inline void append_region_row(std::string &o, const char *name, uint32_t start, uint32_t end, const std::string &label, const uint64_t *s)
{
    char num[256];
    o += name;
    o.append(num, (size_t)snprintf(num, sizeof(num), "\t%u\t%u\t", start, end));
    o += label;
    const unsigned long long n = s[0], m = s[1], dd = s[2];
    const double d = (double)s[3] / 65536.0;
    if (!s[0] || !s[3]) { o.append(num, (size_t)snprintf(num, sizeof(num), "\t%llu\t%llu\t%llu\t%.2f\tNA\tNA\tNA\n", n, m, dd, d)); return; }
    const double ratio = (double)s[4] / (double)s[3];
    const Interval ci = wilson(ratio, d);
    o.append(num, (size_t)snprintf(num, sizeof(num), "\t%llu\t%llu\t%llu\t%.2f\t%.3f\t%.3f\t%.3f\n", n, m, dd, d, ratio, ci.lo, ci.hi));
}

// The wiggle line of bin j of width `bin` over the bin's sums; a bin without a ratio (as above) has no line
static inline void append_wig_line(std::string &o, uint64_t j, uint32_t bin, const uint64_t *s)
{
    if (!s[0] || !s[3]) return;
    char num[64];
    o.append(num, (size_t)snprintf(num, sizeof(num), "%llu\t%.3f\n", (unsigned long long)j * bin + 1, (double)s[4] / (double)s[3]));
}

// A PDR row: letter the reference letter at the position (C: '+'), reads >= 1
static inline void append_pdr_row(std::string &o, const char *name, uint32_t pos0, uint8_t letter, uint32_t reads, uint32_t discordant)
{
    char num[96];
    o += name;
    o.append(num, (size_t)snprintf(num, sizeof(num), "\t%u\t%c\t%u\t%u\t%.3f\n", pos0 + 1, letter == 'C' ? '+' : '-', reads, discordant, (double)discordant / (double)reads));
}

}  // namespace bsx_meth_text
