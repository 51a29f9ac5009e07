// bsx_meth_epi.h — the text of the epiallele file (bsx_meth_write_epi, --epi).  Plain C++, no device code: tests/harness/epi_check.cpp
// compiles it on its own under the host sanitizers.
//
// One row per window of four neighbouring reference CpGs: the sequence name, the four 1-based positions of the Cs, `reads` (the sum of the sixteen
// counts), `meth` (methylated calls: sum of popcount(k) * n_k), mean = meth / (4 * reads) as %.3f, the epipolymorphism 1 - sum p_k^2 as %.4f (Landan et al.
// 2012), the methylation entropy -1/4 sum p_k log2 p_k as %.4f (Xie et al. 2011), and the sixteen counts n_0 .. n_15.  p_k = n_k / reads in double
// precision.  Bit j of the pattern index k is the state of the window's CpG j, leftmost first, 1 = methylated; the count columns are headed by the pattern
// as four letters in CpG order: UUUU, MUUU, UMUU, MMUU, .. MMMM.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>

namespace bsx_meth_epi {

inline std::string header()
{
    std::string o = "chr\tpos1\tpos2\tpos3\tpos4\treads\tmeth\tmean\tepipoly\tentropy";
    for (int k = 0; k < 16; k++) {
        o += '\t';
        for (int j = 0; j < 4; j++) o += ((k >> j) & 1) ? 'M' : 'U';
    }
    o += '\n';
    return o;
}

// appends the row of one window; pos0: the four 0-based positions, counts: n_0 .. n_15 with a sum of at least 1 (a window without a read is no row)
inline void append_row(std::string &o, const char *name, const uint32_t *pos0, const uint32_t *counts)
{
    unsigned long long reads = 0, meth = 0;
    for (int k = 0; k < 16; k++) { reads += counts[k]; meth += (unsigned long long)__builtin_popcount((unsigned)k) * counts[k]; }
    double sq = 0.0, ent = 0.0;
    for (int k = 0; k < 16; k++) {
        if (!counts[k]) continue;
        const double p = (double)counts[k] / (double)reads;
        sq += p * p;
        ent -= p * std::log2(p);
    }
    char num[160];
    o += name;
    o.append(num, (size_t)snprintf(num, sizeof(num), "\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%.3f\t%.4f\t%.4f", (unsigned long long)pos0[0] + 1, (unsigned long long)pos0[1] + 1,
                                   (unsigned long long)pos0[2] + 1, (unsigned long long)pos0[3] + 1, reads, meth, reads ? (double)meth / (4.0 * (double)reads) : 0.0,
                                   reads ? 1.0 - sq : 0.0, 0.25 * ent));
    for (int k = 0; k < 16; k++) o.append(num, (size_t)snprintf(num, sizeof(num), "\t%u", counts[k]));
    o += '\n';
}

}  // namespace bsx_meth_epi
