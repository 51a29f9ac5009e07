// bsx_meth_diff.h — two-sample differential methylation: the two-sided Fisher exact test of one row, and the text of the three files
// (bsx_meth_write_diff, bsx_meth_write_diff_regions, bsx_meth_write_diff_bins).  Plain C++: fisher_p compiles for the host and, under hipcc, for the
// device (k_meth_fisher of bsx_meth.hip runs this same text); tests/harness/diff_check.cpp compiles the header on its own under the host sanitizers.
// Also here: the delta rule and the direction of a row for the device rules and the host writers alike, the host's filter of the DMR runs, and
// the text of the q-value and DMR files (bsx_meth_write_diff_fdr, _write_diff_regions_fdr, _write_dmrs); tests/harness/fdr_check.cpp compiles those.
//
// The test: the table [[mA, dA - mA], [mB, dB - mB]] with its margins fixed.  x, the methylated count of A, runs over the support
// [max(0, c - dB), min(dA, c)] with c = mA + mB, and w(x) = C(dA, x) C(dB, c - x).  p = sum{w(x) : w(x) <= w(mA) (1 + 1e-7)} / sum w(x): R's fisher.test,
// its rule for ties included.  No lgamma: weights relative to the one at x* = floor((dA + 1)(c + 1) / (dA + dB + 2)) (the mode, clamped to the support)
// by the ratio w(x + 1) / w(x) = (dA - x)(c - x) / ((x + 1)(dB - c + x + 1)).  Relative weights never exceed 1 by more than rounding, so nothing
// overflows; far tails run into the denormals and then to 0, which is what they are worth beside 1.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>

#if defined(__HIPCC__)
#define BSX_DIFF_HD __host__ __device__
#else
#define BSX_DIFF_HD
#endif

namespace bsx_meth_diff {

// Counts as doubles (a row's are 32-bit and exact; an interval's sums are exact below 2^53), 0 <= mA <= dA, 0 <= mB <= dB.  Two walks over the support:
// the first from x* to mA for the threshold, the second over all of it for both sums.  The second passes mA by the same operations as the first, so the
// observed table always selects itself; both sums take their terms in the same order, so a row whose every table is selected is exactly 1.0.
BSX_DIFF_HD inline double fisher_p(double mA, double dA, double mB, double dB)
{
    const double c = mA + mB;
    const double lo = c > dB ? c - dB : 0.0, hi = dA < c ? dA : c;
    if (!(lo < hi)) return 1.0;  // one table
    double xs = floor(((dA + 1.0) * (c + 1.0)) / (dA + dB + 2.0));
    xs = xs < lo ? lo : (xs > hi ? hi : xs);
    double w = 1.0;
    if (mA > xs) for (double x = xs; x < mA; x += 1.0) w = w * (((dA - x) * (c - x)) / ((x + 1.0) * (dB - c + x + 1.0)));
    else for (double x = xs; x > mA; x -= 1.0) w = w * ((x * (dB - c + x)) / ((dA - x + 1.0) * (c - x + 1.0)));
    const double limit = w * (1.0 + 1e-7);
    double all = 1.0, sel = 1.0 <= limit ? 1.0 : 0.0;
    w = 1.0;
    for (double x = xs; x < hi; x += 1.0) {
        w = w * (((dA - x) * (c - x)) / ((x + 1.0) * (dB - c + x + 1.0)));
        all += w;
        if (w <= limit) sel += w;
    }
    w = 1.0;
    for (double x = xs; x > lo; x -= 1.0) {
        w = w * ((x * (dB - c + x)) / ((dA - x + 1.0) * (c - x + 1.0)));
        all += w;
        if (w <= limit) sel += w;
    }
    return sel / all;
}

// The delta rule of a row: |mA dB - mB dA| 1000 >= permille dA dB, both sides as 128-bit integers (a product of two 32-bit counts fits 64 bits).  The one
// place that says it: DiffRule and CandRule of bsx_meth.hip ask here on the device, the writers of the q-value files on the host.
BSX_DIFF_HD inline bool delta_keeps(uint32_t mA, uint32_t dA, uint32_t mB, uint32_t dB, uint32_t permille)
{
    const unsigned long long x = (unsigned long long)mA * dB, y = (unsigned long long)mB * dA, diff = x > y ? x - y : y - x, dd = (unsigned long long)dA * dB;
#if defined(__HIP_DEVICE_COMPILE__)
    const unsigned long long lhi = __umul64hi(diff, 1000ull), llo = diff * 1000ull, rhi = __umul64hi(dd, (unsigned long long)permille), rlo = dd * (unsigned long long)permille;
    return lhi > rhi || (lhi == rhi && llo >= rlo);
#else
    return (unsigned __int128)diff * 1000u >= (unsigned __int128)dd * permille;
#endif
}

// The direction of a row, sign(mB dA - mA dB): +1 where B's ratio is the higher one, -1 where A's is, 0 where they are equal (64-bit integers)
BSX_DIFF_HD inline int delta_sign(uint32_t mA, uint32_t dA, uint32_t mB, uint32_t dB)
{
    const unsigned long long x = (unsigned long long)mA * dB, y = (unsigned long long)mB * dA;
    return y > x ? 1 : (y < x ? -1 : 0);
}

// The runs of k_dmr_runs as (chr, start, end, n_sig) quadruples: those with n_sig >= min_sites move to the front in their order; returns how many stay
static inline size_t keep_runs(uint32_t *runs4, size_t n, uint32_t min_sites)
{
    size_t kept = 0;
    for (size_t i = 0; i < n; i++) {
        if (runs4[i * 4 + 3] < min_sites) continue;
        if (kept != i) for (int q = 0; q < 4; q++) runs4[kept * 4 + q] = runs4[i * 4 + q];
        kept++;
    }
    return kept;
}

// ---- the files ----
static const char *const POS_HEADER = "chr\tpos\tstrand\tcontext\tC_a\tCT_a\tratio_a\tC_b\tCT_b\tratio_b\tdelta\tp\n";
static const char *const REGION_HEADER = "chr\tstart\tend\tname\tn_C\tC_a\tCT_a\tratio_a\tC_b\tCT_b\tratio_b\tdelta\tp\n";
static const char *const BIN_HEADER = "chr\tstart\tend\tn_C\tC_a\tCT_a\tratio_a\tC_b\tCT_b\tratio_b\tdelta\tp\n";
// with Benjamini-Hochberg q-values: the same columns and q behind them; the DMR file
static const char *const POS_FDR_HEADER = "chr\tpos\tstrand\tcontext\tC_a\tCT_a\tratio_a\tC_b\tCT_b\tratio_b\tdelta\tp\tq\n";
static const char *const REGION_FDR_HEADER = "chr\tstart\tend\tname\tn_C\tC_a\tCT_a\tratio_a\tC_b\tCT_b\tratio_b\tdelta\tp\tq\n";
static const char *const DMR_HEADER = "chr\tstart\tend\tn_sig\tn_C\tC_a\tCT_a\tratio_a\tC_b\tCT_b\tratio_b\tdelta\tp\n";

// the two ratios, delta = ratio_b - ratio_a and p, as every file prints them; counts above 0 in both depths
static inline void append_numbers(std::string &o, unsigned long long mA, unsigned long long dA, unsigned long long mB, unsigned long long dB, double p)
{
    const double ra = (double)mA / (double)dA, rb = (double)mB / (double)dB;
    char num[192];
    o.append(num, (size_t)snprintf(num, sizeof(num), "\t%llu\t%llu\t%.3f\t%llu\t%llu\t%.3f\t%+.3f\t%.4e\n", mA, dA, ra, mB, dB, rb, rb - ra, p));
}

// A position row: pos0 the 0-based position; cls the byte k_diff_emit stores: bits 0-1 the context class (CG, CHG, CHH, CN), bit 2 set over a G ('-');
// counts: mA, dA, mB, dB
static inline void append_pos_row(std::string &o, const char *name, uint32_t pos0, uint8_t cls, const uint32_t *counts, double p)
{
    static const char *const contexts[4] = {"CG", "CHG", "CHH", "CN"};
    char num[64];
    o += name;
    o.append(num, (size_t)snprintf(num, sizeof(num), "\t%u\t%c\t%s", pos0 + 1, (cls & 4) ? '-' : '+', contexts[cls & 3]));
    append_numbers(o, counts[0], counts[1], counts[2], counts[3], p);
}

// A row of the region file (label != nullptr) or the bin file (label == nullptr) over the interval's sums s = [N, MA, DA, MB, DB]; without a common site
// there is no ratio, no delta and no p
static inline void append_interval_row(std::string &o, const char *name, uint32_t start, uint32_t end, const std::string *label, const uint64_t *s, double p)
{
    char num[96];
    o += name;
    o.append(num, (size_t)snprintf(num, sizeof(num), "\t%u\t%u", start, end));
    if (label) { o += '\t'; o += *label; }
    if (!s[0]) { o += "\t0\t0\t0\tNA\t0\t0\tNA\tNA\tNA\n"; return; }
    o.append(num, (size_t)snprintf(num, sizeof(num), "\t%llu", (unsigned long long)s[0]));
    append_numbers(o, s[1], s[2], s[3], s[4], p);
}

// q behind a row that one of the functions above has just appended: the row's line end becomes a tab, then q as "%.4e", NA for a NaN (a row outside the
// family), and the line end
static inline void append_q(std::string &o, double q)
{
    char num[48];
    o.back() = '\t';
    if (q != q) o += "NA\n";
    else o.append(num, (size_t)snprintf(num, sizeof(num), "%.4e\n", q));
}

// A row of the DMR file: the span [start, end) of a run of n_sig candidates and the interval's sums s = [N, MA, DA, MB, DB] (N >= n_sig >= 1) with their p
static inline void append_dmr_row(std::string &o, const char *name, uint32_t start, uint32_t end, uint32_t n_sig, const uint64_t *s, double p)
{
    char num[96];
    o += name;
    o.append(num, (size_t)snprintf(num, sizeof(num), "\t%u\t%u\t%u\t%llu", start, end, n_sig, (unsigned long long)s[0]));
    append_numbers(o, s[1], s[2], s[3], s[4], p);
}

}  // namespace bsx_meth_diff
