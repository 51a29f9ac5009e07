// bsx_meth.hip — methylation-ratio pile-up on the GPU (reference: methratio.py of the BSMAP tree).
//
// The reference walks the alignments one by one in Python: duplicate removal by fragment end (methratio.py:50-54),
// fill-in trimming (:55-63), then for every reference C (G on the minus strand) under the read one or two counter
// increments (:104-114), optionally folding CpG pairs (:118-128), and a table of the covered cytosines (:135-151).
// Here the per-alignment part runs as one wave per alignment with atomic counters in HBM:
//   k_meth_first   input-order duplicate removal: atomicMin of the alignment's global index on its fragment-end slot
//   k_meth_pile    trim, bounds test, compare read and reference letters, atomicAdd on depth / methylated counters
//   k_meth_pile_mbias   the same pile-up in a persistent grid that also tallies every call by strand, context and read cycle (M-bias, --mbias) in LDS
//   k_meth_cpg     fold the G of every CG into its C
//   k_meth_reads   per-read call counts ahead of the pile-up: non-conversion filter, read histogram, PDR cells; off by default
//   k_meth_epi     per read, the methylation pattern of every four neighbouring CpGs it covers, tallied per window (epialleles); off by default;
//                  k_cpg_count / k_cpg_emit build the CpG index it needs
// With the C/T-SNP mode on (bsx_meth_set_ct_snp, an extension: -i of later BSMAP releases) the same pile-up pass also counts, per reference position, what the reads
// of the OTHER reference strand show there (G over an intact C, A over a C->T SNP), and the row selection and the table use those two counters.
//   k_meth_bins / k_meth_regions   pooled sums per fixed bin (wiggle track, -w / -b) and per interval (BED, --regions) under the table's row rule
// The reports that list rows in order share one ordered compaction, compact_count / compact_emit, over a rule struct (what a row is, what it stores):
//   k_meth_count / k_meth_emit (TableRule: the positions the table lists), k_pdr_count / k_pdr_emit (PdrRule), k_epi_count / k_epi_emit (EpiRule)
// and one host path, meth_compact (count, scan, size, emit).  A new per-position or per-window report is a rule struct and two wrappers.
// Two handles at once (differential methylation): k_diff_count / k_diff_emit (DiffRule: the common sites of two samples whose ratios differ),
//   k_meth_fisher (the two-sided Fisher exact test of every row, bsx_meth_diff.h) and k_meth_diff_regions (the joint form of k_meth_regions; bins are intervals)
// Over the rows of all sequences at once (the store of bsx_meth_diff_report_all): k_bh_keys / k_bh_ratio / k_bh_scatter around a radix sort and a
//   running minimum (Benjamini-Hochberg q-values), k_cand_count / k_cand_emit (CandRule) and k_head_count / k_head_emit (HeadRule) on the same compaction with store
//   rows and candidates as items, and k_dmr_runs (a thread per run: de novo DMRs)
// One place per idea elsewhere too: meth_forward_call (what a forward call is), meth_chr_of / meth_is_cpg (which chromosome, which CpG), meth_covered (the row
// rule), meth_site (a site's five values); on the host DevBuf (device memory that owns itself), OutFile, guarded (no exception across the C ABI), format_rows,
// sorted_chromosomes, and the row formatters of bsx_meth_text.h and bsx_meth_epi.h.
// The host side (bsmap_amd/methratio.py) parses the option surface; the library reads the FASTA and the BSP / SAM / BAM files (bsx_meth_parse.h) and prints the
// table with the reference's arithmetic.  All counters are integers: results are exact.
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <stdexcept>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "bsx_cpus.h"
#include "bsx_internal.h"
#include "bsx_meth_diff.h"
#include "bsx_meth_epi.h"
#include "bsx_meth_parse.h"
#include "bsx_meth_text.h"
#include "bsx_devbuf.h"
#include "bsx_meth_tiles.h"

namespace {

typedef unsigned long long u64;

struct MethDev {
    const uint8_t *ref;      // all chromosomes, upper-case letters, concatenated
    const u64 *chr_off;      // [n_chr+1] offsets into ref / depth / meth
    uint32_t *depth, *meth;  // per reference position
    uint32_t *first;         // [2][total] fragment-end slots of the duplicate filter (direction 1, 2), or null
    u64 total;
    uint32_t n_chr;
};

struct AlnBatch {
    const uint32_t *chr;
    const int64_t *pos;        // 0-based leftmost reference position of the (untrimmed) read
    const uint8_t *strand;     // 0 '++', 1 '-+', 2 '+-', 3 '--'   (first char: reference strand, second: read orientation)
    const int32_t *insert;     // BSP column 8 / SAM TLEN
    const int64_t *cut_at;     // SAM with insert > 0: PNEXT-1 (the read is cut where its mate starts); -1 otherwise
    const uint8_t *seq;
    const u64 *seq_off;
    uint32_t n, index_base, trim_fillin;
    uint32_t trim5, trim3;     // calls of the first trim5 / last trim3 sequencing cycles of every read are ignored
    const uint8_t *drop;       // [n] non-zero: dropped by the non-conversion filter (written by k_meth_reads), or null when the filter is off
};

// C/T-SNP mode: the kernels take `rev`, one cell per reference position: low word rev_GA (opposite-strand calls that show the unconverted or the converted
// letter), high word rev_G (those that show the unconverted letter); null when the mode is off.  (A kernel argument of its own, not a field of MethDev: the
// kernels' other arguments stay where they were.)

// M-bias tally: cells[strand code 0..3][context 0..3][cycle 0..BSX_MBIAS_CYCLES-1][methylated ? 1 : 0], then one counter of the calls at later cycles
struct MbiasDev {
    u64 *cells, *overflow;
};
constexpr int MB_LDS_CYCLES = 256;                    // cycles a block tallies in LDS: 16 groups x 2 x 256 x 4 B = 32 KiB; later cycles go to HBM directly
constexpr int MB_LDS_CELLS = 16 * 2 * MB_LDS_CYCLES;
constexpr int MB_BLOCK = 1024, MB_BLOCKS_PER_CU = 2;  // 32 waves per CU, 64 KiB of its LDS
constexpr size_t MB_CELLS = (size_t)16 * BSX_MBIAS_CYCLES * 2;

// Python's s[a:b] on a string of length n (a, b may be negative or past the ends) as [lo, hi)
__device__ __forceinline__ void py_slice(int64_t n, bool has_a, int64_t a, bool has_b, int64_t b, int64_t &lo, int64_t &hi)
{
    lo = 0; hi = n;
    if (has_a) { if (a < 0) a += n; lo = a < 0 ? 0 : (a > n ? n : a); }
    if (has_b) { if (b < 0) b += n; hi = b < 0 ? 0 : (b > n ? n : b); }
    if (hi < lo) hi = lo;
}

__device__ __forceinline__ bool dup_slot(const MethDev &M, const AlnBatch &B, uint32_t i, u64 &slot)
{
    const uint32_t c = B.chr[i];
    const int64_t len = (int64_t)(B.seq_off[i + 1] - B.seq_off[i]), clen = (int64_t)(M.chr_off[c + 1] - M.chr_off[c]);
    const uint32_t st = B.strand[i];
    const bool end_side = st == 2 || st == 1;  // '+-' or '-+': the fragment end is the read's right end (methratio.py:51)
    const int64_t fe = end_side ? B.pos[i] + len : B.pos[i];
    if (fe < 0 || fe >= clen) return false;    // (the reference would index outside its coverage array here)
    slot = (end_side ? M.total : 0) + M.chr_off[c] + (u64)fe;
    return true;
}

__global__ void k_meth_first(MethDev M, AlnBatch B)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B.n) return;
    u64 slot;
    if (dup_slot(M, B, i, slot)) atomicMin(&M.first[slot], B.index_base + i);
}

// What survives of alignment i: the read letters seq[lo:hi) of its n0, aligned at pos of chromosome c.  False for an alignment that is not a valid
// mapping: a duplicate (methratio.py:52-56) or one that fails a bounds test (:102).  Depends on i alone, so it is uniform over the wave.
struct MethWindow {
    int64_t n0, lo, hi, pos;
    uint32_t c, st;
};

__device__ __forceinline__ bool meth_window(const MethDev &M, const AlnBatch &B, uint32_t i, MethWindow &W)
{
    if (B.drop && B.drop[i]) return false;  // the non-conversion filter took it: not a valid mapping, no call of any kind
    if (M.first) {
        u64 slot;
        if (dup_slot(M, B, i, slot) && M.first[slot] != B.index_base + i) return false;  // an earlier alignment owns this fragment end
    }
    const uint32_t c = B.chr[i], st = B.strand[i];
    const int64_t n0 = (int64_t)(B.seq_off[i + 1] - B.seq_off[i]), clen = (int64_t)(M.chr_off[c + 1] - M.chr_off[c]);
    int64_t pos = B.pos[i], lo = 0, hi = n0;  // the read letters that survive are seq[lo:hi), aligned at pos
    if (pos > clen) return false;  // skipped by methratio.py:100 whatever is trimmed (no trim moves a read left); also keeps the sums below from overflowing on a hostile position
    const int64_t t = (int64_t)B.trim_fillin, ins = B.insert[i];
    if (t > 0) {  // methratio.py:55-63
        if (st == 2) py_slice(n0, false, 0, true, -t, lo, hi);                         // '+-': seq[:-t]
        else if (st == 3) { py_slice(n0, true, t, false, 0, lo, hi); pos += t; }       // '--': seq[t:], pos + t
        else if (ins != 0 && n0 > (ins < 0 ? -ins : ins) - t) {
            const int64_t trim_nt = n0 - ((ins < 0 ? -ins : ins) - t);
            if (st == 0) py_slice(n0, false, 0, true, -trim_nt, lo, hi);               // '++': seq[:-trim_nt]
            else if (st == 1) { py_slice(n0, true, trim_nt, false, 0, lo, hi); pos += trim_nt; }  // '-+': seq[trim_nt:]
        }
    }
    if (B.cut_at[i] >= 0) {  // SAM, insert > 0: seq[:PNEXT-1-pos]  (methratio.py:64)
        int64_t l2, h2;
        py_slice(hi - lo, false, 0, true, B.cut_at[i] - pos, l2, h2);
        hi = lo + h2;
    }
    if (pos + (hi - lo) > clen) return false;  // methratio.py:100
    W.n0 = n0; W.lo = lo; W.hi = hi; W.pos = pos; W.c = c; W.st = st;
    return true;
}

// Context class of the cytosine at global letter g of the chromosome [c0, c1): 0 CG, 1 CHG, 2 CHH, 3 "CN".  '+' strands look at the next two letters; '-'
// strands (the call is a G) at the previous two, with C in the role of G.  A neighbour outside the chromosome counts as no letter: the concatenated text
// goes on with the next chromosome there (the trap of meth_is_cpg), so both indices are tested against [c0, c1) before they are read.
__device__ __forceinline__ uint32_t meth_context(const uint8_t *ref, u64 g, u64 c0, u64 c1, bool plus)
{
    uint8_t n1 = 0, n2 = 0;
    if (plus) { if (g + 1 < c1) n1 = ref[g + 1]; if (g + 2 < c1) n2 = ref[g + 2]; }
    else { if (g >= c0 + 1) n1 = ref[g - 1]; if (g >= c0 + 2) n2 = ref[g - 2]; }
    const uint8_t gl = plus ? 'G' : 'C', other = plus ? 'C' : 'G';  // H = A, T and `other`
    if (n1 == gl) return 0;
    if (n1 != 'A' && n1 != 'T' && n1 != other) return 3;
    if (n2 == gl) return 1;
    return (n2 == 'A' || n2 == 'T' || n2 == other) ? 2 : 3;
}

// Whether letter k of the window, over the reference letter rl, is a forward call: the one place that holds its three tests, in this order: own cytosine
// (C under a '+' read, G under a '-' read), one of the two letters, cycle mask.  Returns the call's cycle and in `m` whether it shows the unconverted
// letter, or -1 where there is no forward call.
__device__ __forceinline__ int64_t meth_forward_call(const AlnBatch &B, const MethWindow &W, const uint8_t *s, uint8_t rl, int64_t k, bool &m)
{
    const bool plus = !(W.st & 1), backward = W.st == 1 || W.st == 2;
    const uint8_t match = plus ? 'C' : 'G', convert = plus ? 'T' : 'A';  // strand[0]: '+' -> C/T, '-' -> G/A
    if (rl != match) return -1;
    const uint8_t ch = s[k];
    if (ch != convert && ch != match) return -1;
    const int64_t j = W.lo + k, cyc = backward ? W.n0 - 1 - j : j;  // 0 <= cyc < n0
    if (cyc < (int64_t)B.trim5 || cyc >= W.n0 - (int64_t)B.trim3) return -1;
    m = ch == match;
    return cyc;
}

// The calls of one valid alignment, a lane per letter: depth / methylated counters, and with MBIAS the tally cell of every call.
// Cycle of letter j of the untrimmed read = its 0-based index in sequencing direction: j for '++' and '--', n0-1-j for '-+' and '+-'.  (methratio.py:52-63:
// the fragment end of '+-' / '-+' is the displayed right end, '+-' loses its fill-in at the displayed right = its first cycles, '--' at the displayed left.)
// A call at cycle c is dropped when c < trim5 or c >= n0 - trim3; the window, and with it pos, the bounds tests and the duplicate filter, does not move.
// With SNP a letter over the OTHER strand's cytosine (reference G under a '+' read, C under a '-' read) makes a reverse call: one 64-bit add on the position's
// packed cell, rev_G and rev_GA for the unconverted letter, rev_GA alone for the converted one.  A reference letter is C or G or neither, so a lane makes at most
// one call per letter; the cycle mask drops a reverse call like a forward one, and a reverse call enters nothing else.
template <bool MBIAS, bool SNP>
__device__ __forceinline__ void meth_calls(const MethDev &M, const AlnBatch &B, uint32_t i, const MethWindow &W, int lane, uint32_t *s_tally, const MbiasDev &D, u64 &over, u64 *rev)
{
    if (W.pos < 0) return;         // (a negative position would make the reference slice from the chromosome's end: never produced by bsmap)
    const uint32_t st = W.st;
    const bool plus = !(st & 1), backward = st == 1 || st == 2;
    const uint8_t *s = B.seq + B.seq_off[i] + W.lo;
    const u64 c0 = M.chr_off[W.c], c1 = M.chr_off[W.c + 1], g0 = c0 + (u64)W.pos;
    const int64_t len = W.hi - W.lo, cyc_lo = (int64_t)B.trim5, cyc_hi = W.n0 - (int64_t)B.trim3;
    for (int64_t k = lane; k < len; k += 64) {
        const uint8_t rl = M.ref[g0 + k];
        bool mb = false;
        const int64_t cyc = meth_forward_call(B, W, s, rl, k, mb);
        if (cyc < 0) {
            if (SNP) {  // (the other strand's letter is not the read strand's own: a letter that failed a later forward test ends at the first test here)
                const uint8_t rc_match = plus ? 'G' : 'C', rc_convert = plus ? 'A' : 'T';
                if (rl != rc_match) continue;
                const uint8_t rch = s[k];
                if (rch != rc_convert && rch != rc_match) continue;
                const int64_t rj = W.lo + k, rcyc = backward ? W.n0 - 1 - rj : rj;
                if (rcyc < cyc_lo || rcyc >= cyc_hi) continue;
                atomicAdd(&rev[g0 + k], rch == rc_match ? ((1ull << 32) | 1ull) : 1ull);  // < 2^32 alignments per handle: the low word cannot carry
            }
            continue;
        }
        const uint32_t m = mb;
        if (m) atomicAdd(&M.meth[g0 + k], 1u);
        atomicAdd(&M.depth[g0 + k], 1u);
        if (MBIAS) {
            if (cyc >= BSX_MBIAS_CYCLES) { over++; continue; }
            const uint32_t grp = st * 4 + meth_context(M.ref, g0 + k, c0, c1, plus);
            // LDS cells are [group][methylated][cycle]: the lanes of a wave hold consecutive cycles, so consecutive words (no bank is hit twice)
            if (cyc < MB_LDS_CYCLES) atomicAdd(&s_tally[(grp * 2 + m) * MB_LDS_CYCLES + (uint32_t)cyc], 1u);
            else atomicAdd(&D.cells[((u64)grp * BSX_MBIAS_CYCLES + (u64)cyc) * 2 + m], 1ull);
        }
    }
}

// one wave per alignment
template <bool SNP>
__global__ __launch_bounds__(256) void k_meth_pile(MethDev M, AlnBatch B, u64 *n_valid, u64 *rev)
{
    const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= B.n) return;
    MethWindow W;
    if (!meth_window(M, B, i, W)) return;
    if (lane == 0) atomicAdd(n_valid, 1ull);
    u64 over = 0;
    meth_calls<false, SNP>(M, B, i, W, lane, nullptr, MbiasDev{nullptr, nullptr}, over, rev);
}

// The twin of k_meth_pile with the M-bias tally: a grid sized by the CU count, every wave walks the alignments with the grid's stride.  The cells of the
// first MB_LDS_CYCLES cycles are private to the block in LDS (a wave's 64 lanes are 64 cycles of one read: distinct cells) and reach HBM once, when the
// block is done, as one 64-bit atomicAdd per non-zero cell; the count of valid mappings and the overflow count take the same way.  An LDS cell gets at
// most one call per alignment and a batch has fewer than 2^32 alignments, so 32 bits hold it.
template <bool SNP>
__global__ __launch_bounds__(MB_BLOCK) void k_meth_pile_mbias(MethDev M, AlnBatch B, u64 *n_valid, MbiasDev D, u64 *rev)
{
    __shared__ uint32_t s_tally[MB_LDS_CELLS];
    __shared__ u64 s_over;
    __shared__ uint32_t s_valid;
    for (uint32_t t = threadIdx.x; t < (uint32_t)MB_LDS_CELLS; t += blockDim.x) s_tally[t] = 0;
    if (threadIdx.x == 0) { s_over = 0; s_valid = 0; }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const uint32_t waves = blockDim.x >> 6;
    uint32_t valid = 0;
    u64 over = 0;
    for (u64 i = (u64)blockIdx.x * waves + (threadIdx.x >> 6); i < B.n; i += (u64)gridDim.x * waves) {
        MethWindow W;
        if (!meth_window(M, B, (uint32_t)i, W)) continue;
        valid++;
        meth_calls<true, SNP>(M, B, (uint32_t)i, W, lane, s_tally, D, over, rev);
    }
    if (lane == 0 && valid) atomicAdd(&s_valid, valid);
    if (over) atomicAdd(&s_over, over);
    __syncthreads();
    for (uint32_t t = threadIdx.x; t < (uint32_t)MB_LDS_CELLS; t += blockDim.x) {
        const uint32_t v = s_tally[t];
        if (!v) continue;
        const uint32_t gm = t / MB_LDS_CYCLES, cyc = t % MB_LDS_CYCLES;  // gm = group * 2 + methylated
        atomicAdd(&D.cells[((u64)(gm >> 1) * BSX_MBIAS_CYCLES + cyc) * 2 + (gm & 1)], (u64)v);
    }
    if (threadIdx.x == 0) {
        if (s_valid) atomicAdd(n_valid, (u64)s_valid);
        if (s_over) atomicAdd(D.overflow, s_over);
    }
}

// ---- per-read calls: non-conversion filter, read histogram, PDR ----
// What k_meth_reads gets beside the batch.  hist: cg[32][32], ch[64], then the four totals (reads, cg_over, ch_calls, ch_meth), or null; pdr: one cell per
// reference position, low word reads, high word discordant, or null; drop: the batch's flags to write, or null when the filter is off.
struct ReadsDev {
    u64 *hist, *pdr, *dropped;
    uint8_t *drop;
    uint32_t nonconv, min_cpg;
};
constexpr int RS_CG = BSX_RS_CG_MAX + 1, RS_CH = BSX_RS_CH_MAX + 1;
constexpr int RS_LDS_CELLS = RS_CG * RS_CG + RS_CH;  // the cells a block tallies in LDS: 1 088 x 4 B
constexpr size_t RS_CELLS = (size_t)RS_LDS_CELLS + 4;
constexpr int RS_BLOCK = 512, RS_BLOCKS_PER_CU = 3;  // 78 VGPRs: 6 waves per SIMD, 24 per CU

// Letter k of the window as a call: its context class 0..3 and in `m` whether it shows the unconverted letter; -1 where meth_calls makes no forward call
__device__ __forceinline__ int meth_call_class(const MethDev &M, const AlnBatch &B, const MethWindow &W, const uint8_t *s, u64 c0, u64 c1, u64 g0, int64_t k, bool &m)
{
    if (meth_forward_call(B, W, s, M.ref[g0 + k], k, m) < 0) return -1;
    return (int)meth_context(M.ref, g0 + k, c0, c1, !(W.st & 1));
}

// One wave per alignment in a persistent grid (the shape of k_meth_pile_mbias), ahead of the pile-up.  The wave walks the window 64 letters at a time; a lane
// classifies its letter, four ballots and popcounts give the wave n_cg, m_cg, n_ch, m_ch of the step as uniform values, summed over the steps of a read
// longer than 64.  Then, uniform over the wave: lane 0 tallies the read in the block's LDS histogram (cg[0..1][..] and ch[0] receive nearly every read: one
// atomic per read on them in HBM would serialise; the block flushes its non-zero cells once, as 64-bit atomic adds), lane 0 writes the drop flag the
// pile-up kernels read through AlnBatch::drop, and for an eligible read a second walk adds one packed 64-bit value per CG call to the PDR cells.
// The totals are uniform too and stay in registers until the block is done.  B.drop is null here: the window is the unfiltered one.
__global__ __launch_bounds__(RS_BLOCK) void k_meth_reads(MethDev M, AlnBatch B, ReadsDev R)
{
    __shared__ uint32_t s_hist[RS_LDS_CELLS];
    __shared__ u64 s_tot[5];  // reads, cg_over, ch_calls, ch_meth, dropped
    for (uint32_t t = threadIdx.x; t < (uint32_t)RS_LDS_CELLS; t += blockDim.x) s_hist[t] = 0;
    if (threadIdx.x < 5) s_tot[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const uint32_t waves = blockDim.x >> 6;
    u64 tot[5] = {0, 0, 0, 0, 0};
    for (u64 i = (u64)blockIdx.x * waves + (threadIdx.x >> 6); i < B.n; i += (u64)gridDim.x * waves) {
        MethWindow W;
        bool drop = false;
        if (meth_window(M, B, (uint32_t)i, W)) {
            uint32_t n_cg = 0, m_cg = 0, n_ch = 0, m_ch = 0;
            const uint8_t *s = B.seq + B.seq_off[i] + W.lo;
            const u64 c0 = M.chr_off[W.c], c1 = M.chr_off[W.c + 1], g0 = c0 + (u64)W.pos;
            const int64_t len = W.pos < 0 ? 0 : W.hi - W.lo;  // (a negative position makes no call: meth_calls)
            for (int64_t k0 = 0; k0 < len; k0 += 64) {  // uniform bounds: every lane takes part in the ballots
                bool m = false;
                const int cls = k0 + lane < len ? meth_call_class(M, B, W, s, c0, c1, g0, k0 + lane, m) : -1;
                const bool cg = cls == 0, chx = cls == 1 || cls == 2;
                n_cg += (uint32_t)__builtin_popcountll(__ballot(cg)); m_cg += (uint32_t)__builtin_popcountll(__ballot(cg && m));
                n_ch += (uint32_t)__builtin_popcountll(__ballot(chx)); m_ch += (uint32_t)__builtin_popcountll(__ballot(chx && m));
            }
            if (R.hist) {
                if (lane == 0) {
                    if (n_cg <= BSX_RS_CG_MAX) atomicAdd(&s_hist[n_cg * RS_CG + m_cg], 1u);
                    atomicAdd(&s_hist[RS_CG * RS_CG + (m_ch < BSX_RS_CH_MAX ? m_ch : BSX_RS_CH_MAX)], 1u);
                }
                tot[0]++; tot[1] += n_cg > BSX_RS_CG_MAX; tot[2] += n_ch; tot[3] += m_ch;
            }
            drop = R.nonconv && m_ch >= R.nonconv;
            tot[4] += drop;
            if (R.pdr && !drop && n_cg >= R.min_cpg) {  // eligible (min_cpg >= 1: n_cg > 0, so the position is not negative)
                const u64 add = (m_cg != 0 && m_cg != n_cg) ? ((1ull << 32) | 1ull) : 1ull;  // < 2^32 alignments per handle: the low word cannot carry
                for (int64_t k = lane; k < len; k += 64) {
                    bool m = false;
                    if (meth_call_class(M, B, W, s, c0, c1, g0, k, m) == 0) atomicAdd(&R.pdr[g0 + k], add);
                }
            }
        }
        if (R.drop && lane == 0) R.drop[i] = drop;
    }
    if (lane == 0) for (int q = 0; q < 5; q++) if (tot[q]) atomicAdd(&s_tot[q], tot[q]);
    __syncthreads();
    if (R.hist) {
        for (uint32_t t = threadIdx.x; t < (uint32_t)RS_LDS_CELLS; t += blockDim.x) { const uint32_t v = s_hist[t]; if (v) atomicAdd(&R.hist[t], (u64)v); }
        if (threadIdx.x < 4 && s_tot[threadIdx.x]) atomicAdd(&R.hist[RS_LDS_CELLS + threadIdx.x], s_tot[threadIdx.x]);
    }
    if (threadIdx.x == 0 && s_tot[4]) atomicAdd(R.dropped, s_tot[4]);
}

// ---- epiallele patterns per window of four CpGs ----
// The CpG index of the handle (meth_epi_index): the chromosome-relative positions of the C of every reference CpG, all chromosomes in order (a CpG's index in
// that list is its GLOBAL ordinal; the host keeps the ordinal of every chromosome's first CpG), and the rank directory `dir`: the number of CpGs ahead of
// every 64-letter block of the concatenated text, blocks counted from letter 0 of the text (not of a chromosome).  cells: 16 counters per CpG, those of the
// window that STARTS at this CpG; n_cpg: the number of CpGs, the bound of every index into cells.
struct EpiDev {
    const uint32_t *dir;
    uint32_t *cells;
    u64 n_cpg;
};

// the chromosome that holds letter x < M.total of the concatenated text
__device__ __forceinline__ uint32_t meth_chr_of(const MethDev &M, u64 x)
{
    uint32_t lo = 0, hi = M.n_chr;
    while (hi - lo > 1) { const uint32_t mid = (lo + hi) / 2; if (M.chr_off[mid] <= x) lo = mid; else hi = mid; }
    return lo;
}

// Whether letter x of the concatenated text is the C of a reference CpG.  The G must lie in x's own chromosome: a C at the end of one sequence and a G at
// the start of the next are no CpG (the search runs only behind a "CG").  The text is zero-padded behind M.total.  The one place that knows this trap: the
// CpG index and the fold of k_meth_cpg both ask here.
__device__ __forceinline__ bool meth_is_cpg(const MethDev &M, u64 x)
{
    if (x + 1 >= M.total || M.ref[x] != 'C' || M.ref[x + 1] != 'G') return false;
    return x + 1 < M.chr_off[meth_chr_of(M, x) + 1];
}

// The number of reference CpGs whose C lies ahead of letter g (g <= M.total): the directory's count for g's block, and for the rest of the way one 64-letter
// load, a ballot and a masked popcount.  Every lane of the wave calls it with the same g.  (A CpG whose C is letter 63 of a block has its G in the next one:
// meth_is_cpg reads it from there.)
__device__ __forceinline__ uint32_t meth_cpg_rank(const MethDev &M, const uint32_t *dir, u64 g, int lane)
{
    const u64 bal = __ballot(meth_is_cpg(M, (g & ~63ull) + (u64)lane));
    return dir[g >> 6] + (uint32_t)__builtin_popcountll(bal & ((1ull << (g & 63)) - 1));
}

// one wave per 64-letter block: its number of CpGs (cnt[block]; the directory is the exclusive scan of these) ...
__global__ __launch_bounds__(256) void k_cpg_count(MethDev M, u64 n_blocks, uint32_t *cnt)
{
    const u64 b = (u64)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= n_blocks) return;
    const u64 bal = __ballot(meth_is_cpg(M, b * 64 + (threadIdx.x & 63)));
    if ((threadIdx.x & 63) == 0) cnt[b] = (uint32_t)__builtin_popcountll(bal);
}

// ... and their positions, each CpG at its ordinal
__global__ __launch_bounds__(256) void k_cpg_emit(MethDev M, u64 n_blocks, const uint32_t *dir, uint32_t *pos)
{
    const u64 b = (u64)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= n_blocks) return;
    const int lane = threadIdx.x & 63;
    const u64 x = b * 64 + lane;
    const bool cpg = meth_is_cpg(M, x);
    const u64 bal = __ballot(cpg);
    if (!cpg) return;
    pos[dir[b] + (uint32_t)__builtin_popcountll(bal & ((1ull << lane) - 1))] = (uint32_t)(x - M.chr_off[meth_chr_of(M, x)]);
}

// one wave per chromosome border: the global ordinal of the first CpG at or behind it
__global__ __launch_bounds__(64) void k_cpg_chr_first(MethDev M, const uint32_t *dir, uint32_t *chr_first)
{
    const uint32_t r = meth_cpg_rank(M, dir, M.chr_off[blockIdx.x], (int)threadIdx.x);
    if (threadIdx.x == 0) chr_first[blockIdx.x] = r;
}

// The tally: one wave per alignment, behind k_meth_reads (B.drop holds this add's verdicts, so meth_window admits the valid, not dropped alignments) and ahead
// of the pile-up.  The CpGs of the read are the lanes at a reference CpG's call position (the C under a '+?' read, the G under a '-?' read); they have
// consecutive ordinals from ord0, the rank of the first letter that can be the C of one of them.  Per 64-letter step three ballots: those lanes (cmask),
// the lanes that make a class-0 call (vmask: state M or U; a CpG lane outside it is X) and the methylated ones among them (mmask).  A CpG lane forms the
// window that ENDS at its CpG: it finds the three set bits of cmask below its own, reads their states from vmask / mmask, and where cmask has fewer it takes
// them from the carry, the states of the last three CpGs of the steps before (bit 0 the latest).  So a window that straddles a step border is counted like
// any other, and a read may have any number of CpGs.  One 32-bit atomic add per window without an X.
__global__ __launch_bounds__(256) void k_meth_epi(MethDev M, AlnBatch B, EpiDev E)
{
    const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= B.n) return;
    MethWindow W;
    if (!meth_window(M, B, i, W) || W.pos < 0) return;  // (a negative position makes no call: meth_calls)
    const int64_t len = W.hi - W.lo;
    if (len < 7) return;                                // four CpGs have call positions at least 6 letters apart
    const bool plus = !(W.st & 1);
    const uint8_t *s = B.seq + B.seq_off[i] + W.lo;
    const u64 c0 = M.chr_off[W.c], c1 = M.chr_off[W.c + 1], g0 = c0 + (u64)W.pos;
    const uint32_t ord0 = meth_cpg_rank(M, E.dir, plus || g0 == c0 ? g0 : g0 - 1, lane);
    uint32_t seen = 0, carry_n = 0;    // CpGs of the steps before, and how many of them the carry holds (at most 3)
    uint32_t carry_v = 0, carry_m = 0;
    for (int64_t k0 = 0; k0 < len; k0 += 64) {  // uniform bounds: every lane takes part in the ballots
        const int64_t k = k0 + lane;
        bool m = false, cpg = false;
        int cls = -1;
        if (k < len) {
            const u64 g = g0 + (u64)k;
            cpg = plus ? (M.ref[g] == 'C' && g + 1 < c1 && M.ref[g + 1] == 'G') : (M.ref[g] == 'G' && g >= c0 + 1 && M.ref[g - 1] == 'C');
            if (cpg) cls = meth_call_class(M, B, W, s, c0, c1, g0, k, m);  // 0 or -1 here: the position's class is CG
        }
        const u64 cmask = __ballot(cpg);
        if (!cmask) continue;
        const u64 vmask = __ballot(cls == 0), mmask = __ballot(cls == 0 && m);
        if (cpg) {
            u64 below = cmask & ((1ull << lane) - 1);
            const uint32_t r = (uint32_t)__builtin_popcountll(below);
            bool ok = cls == 0 && seen + r >= 3;
            uint32_t pattern = m ? 8u : 0u, q = 0;
            for (int t = 2; t >= 0; t--) {  // the CpG 3 - t places to the left gives bit t
                if (below) {
                    const int p = 63 - __builtin_clzll(below);
                    below &= ~(1ull << p);
                    ok = ok && ((vmask >> p) & 1);
                    pattern |= (uint32_t)((mmask >> p) & 1) << t;
                } else {
                    ok = ok && q < carry_n && ((carry_v >> q) & 1);
                    pattern |= ((carry_m >> q) & 1) << t;
                    q++;
                }
            }
            const u64 w = (u64)ord0 + seen + r - 3;  // the window's first CpG
            if (ok && w + 3 < E.n_cpg) atomicAdd(&E.cells[w * 16 + pattern], 1u);  // (the bound holds by construction: the lanes' CpG test is meth_is_cpg's)
        }
        // the carry for the next step: this step's last CpGs, then what the old carry still has to give (all uniform over the wave)
        uint32_t nv = 0, nm = 0, cnt = 0;
        for (u64 rem = cmask; rem && cnt < 3; cnt++) {
            const int p = 63 - __builtin_clzll(rem);
            rem &= ~(1ull << p);
            nv |= (uint32_t)((vmask >> p) & 1) << cnt; nm |= (uint32_t)((mmask >> p) & 1) << cnt;
        }
        for (uint32_t q = 0; q < carry_n && cnt < 3; q++, cnt++) { nv |= ((carry_v >> q) & 1) << cnt; nm |= ((carry_m >> q) & 1) << cnt; }
        carry_v = nv; carry_m = nm; carry_n = cnt;
        seen += (uint32_t)__builtin_popcountll(cmask);
    }
}

__global__ void k_meth_cpg(MethDev M, u64 *rev, u64 *pdr)
{
    // every "CG" of every chromosome (occurrences cannot overlap): the G's counters move onto the C  (methratio.py:118-128)
    for (u64 g = (u64)blockIdx.x * blockDim.x + threadIdx.x; g + 1 < M.total; g += (u64)gridDim.x * blockDim.x) {
        if (!meth_is_cpg(M, g)) continue;  // (a C that is the last letter of a chromosome does not pair with the first letter of the next one)
        M.depth[g] += M.depth[g + 1]; M.meth[g] += M.meth[g + 1];
        M.depth[g + 1] = 0; M.meth[g + 1] = 0;
        if (rev) { rev[g] += rev[g + 1]; rev[g + 1] = 0; }  // both halves at once: each sum stays below 2^32
        if (pdr) { pdr[g] += pdr[g + 1]; pdr[g + 1] = 0; }  // likewise
    }
}

// What the table lists (bsx_meth_report_chr): the lowest depth, -z, the C/T-SNP mode (0 off, 1 correct, 2 skip) and the context mask (bit 0 CG, 1 CHG, 2 CHH,
// 3 other; 0 and 0xF: no filter)
struct RowRule {
    uint32_t min_depth, ctx_mask;
    int meth0, snp;
};

// Whether position k of the chromosome [g0, g0 + n) is covered, with its counters.  Integer tests only, in this order: depth, context class of the position's own
// letter (C: '+' strand, G: '-' strand; another letter is in no class), then the SNP tests: mode 2 drops a position with any converted opposite-strand call, mode 1
// one whose opposite-strand calls are all converted (its effective depth is 0), and both drop depth 0.
__device__ __forceinline__ bool meth_covered(const MethDev &M, const u64 *rev, u64 g0, u64 n, u64 k, const RowRule &R, uint32_t &d, uint32_t &m, uint32_t &g, uint32_t &ga)
{
    d = M.depth[g0 + k]; m = M.meth[g0 + k]; g = ga = 0;
    // (one flag, no early return: with a return per test the compiler's unrolled k_meth_count lost the depth of its first position in the SNP path)
    bool ok = d >= R.min_depth;
    if (ok && R.ctx_mask != 0 && R.ctx_mask != 0xF) {
        const uint8_t l = M.ref[g0 + k];
        ok = (l == 'C' || l == 'G') && ((R.ctx_mask >> meth_context(M.ref, g0 + k, g0, g0 + n, l == 'C')) & 1);
    }
    if (ok && R.snp) {
        const u64 cell = rev[g0 + k];
        ga = (uint32_t)cell; g = (uint32_t)(cell >> 32);
        ok = d != 0 && (R.snp == 2 ? g == ga : (g != 0 || ga == 0));
    }
    return ok;
}

// ---- ordered compaction: the rows of a report in ascending item order ----
// Every per-position or per-window report is the same two passes over the items [0, n) of one chromosome, in blocks of 1 024 items taken in 4 rounds of
// 256 (item = block * 1024 + round * 256 + thread: ascending with (round, thread)): compact_count leaves the number of rows of every block, the host scans
// them (meth_compact), and compact_emit gives every row its place: the block's start, the rows of the rounds and waves before (one ballot per wave, a
// prefix over s_wave[4]), the rows of the lower lanes.  What a row is and what it stores comes from a rule struct:
//   Row                          the payload row() reads and store() writes
//   bool row(k, Row &)           whether item k < n is a row; the same answer in both passes
//   void store(o, k, const Row &)   row number o of the chromosome (64 bits: a rule may scale it) is item k
// A new report is a rule struct and two one-line kernels.
template <class Rule>
__device__ __forceinline__ void compact_count(Rule &rule, u64 n, uint32_t *blk_rows)
{
    __shared__ uint32_t s_rows;
    if (threadIdx.x == 0) s_rows = 0;
    __syncthreads();
    uint32_t rows = 0;
    for (int r = 0; r < 4; r++) {
        const u64 k = (u64)blockIdx.x * 1024 + (u64)r * 256 + threadIdx.x;
        typename Rule::Row w;
        if (k < n) rows += rule.row(k, w);
    }
    if (rows) atomicAdd(&s_rows, rows);
    __syncthreads();
    if (threadIdx.x == 0) blk_rows[blockIdx.x] = s_rows;
}

template <class Rule>
__device__ __forceinline__ void compact_emit(Rule &rule, u64 n, const uint32_t *blk_start)
{
    __shared__ uint32_t s_wave[4];
    uint32_t base = blk_start[blockIdx.x];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int r = 0; r < 4; r++) {
        const u64 k = (u64)blockIdx.x * 1024 + (u64)r * 256 + threadIdx.x;
        typename Rule::Row w{};
        bool row = false;
        if (k < n) row = rule.row(k, w);
        const u64 bal = __ballot(row);
        if (lane == 0) s_wave[wv] = (uint32_t)__builtin_popcountll(bal);
        __syncthreads();
        uint32_t off = base;
        for (int q = 0; q < wv; q++) off += s_wave[q];
        if (row) rule.store((u64)(off + (uint32_t)__builtin_popcountll(bal & ((1ull << lane) - 1))), k, w);
        base += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
        __syncthreads();
    }
}

// The table (bsx_meth_report_chr): the covered positions of the chromosome [g0, g0 + n) that are methylated or listed under -z.  nc, nd: the covered
// positions this thread has seen and their raw depth (in every mode), kept with SUMS for k_meth_count to flush (without it they stay 0: k_meth_emit has no
// use for them and is a tenth slower when it keeps them)
template <bool SUMS>
struct TableRule {
    struct Row { uint32_t d, m, g, ga; };
    MethDev M;
    u64 g0, n;
    RowRule R;
    const u64 *rev;
    uint32_t *out_pos, *out_depth, *out_meth;
    u64 *out_ctx;
    uint32_t *out_rev_g, *out_rev_ga;
    u64 nc, nd;
    __device__ __forceinline__ bool row(u64 k, Row &w)
    {
        const bool ok = meth_covered(M, rev, g0, n, k, R, w.d, w.m, w.g, w.ga);
        if (SUMS) { nc += ok; nd += ok ? w.d : 0u; }
        return ok && (w.m != 0 || R.meth0);
    }
    __device__ __forceinline__ void store(u64 o, u64 k, const Row &w) const
    {
        out_pos[o] = (uint32_t)k; out_depth[o] = w.d; out_meth[o] = w.m;
        if (R.snp) { out_rev_g[o] = w.g; out_rev_ga[o] = w.ga; }
        if (out_ctx) {  // refcr[i-2:i+3] with Python's slice rules, byte 7 = the letter at i.  For i < 2 the start i-2 is negative and counts from the
                        // chromosome's end: empty on a chromosome of at least five letters, but not below that ("CCGG": position 1 -> "G", "C": -> "C")
            u64 ctx = 0;
            int nb = 0;
            int64_t lo, hi;
            py_slice((int64_t)n, true, (int64_t)k - 2, true, (int64_t)k + 3, lo, hi);
            for (int64_t q = lo; q < hi; q++) ctx |= (u64)M.ref[g0 + (u64)q] << (8 * nb++);
            out_ctx[o] = ctx | ((u64)M.ref[g0 + k] << 56);
        }
    }
};

__global__ __launch_bounds__(256) void k_meth_count(MethDev M, u64 g0, u64 n, RowRule R, uint32_t *blk_rows, u64 *nc_nd, const u64 *rev)
{
    __shared__ u64 s_nc, s_nd;
    if (threadIdx.x == 0) { s_nc = 0; s_nd = 0; }  // (compact_count's first barrier stands between this and the adds)
    TableRule<true> rule{M, g0, n, R, rev, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0};
    compact_count(rule, n, blk_rows);
    atomicAdd(&s_nc, rule.nc); atomicAdd(&s_nd, rule.nd);
    __syncthreads();
    if (threadIdx.x == 0 && s_nc) { atomicAdd(&nc_nd[0], s_nc); atomicAdd(&nc_nd[1], s_nd); }
}

__global__ __launch_bounds__(256) void k_meth_emit(MethDev M, u64 g0, u64 n, RowRule R, const uint32_t *blk_start, uint32_t *out_pos, uint32_t *out_depth,
                                                   uint32_t *out_meth, u64 *out_ctx, uint32_t *out_rev_g, uint32_t *out_rev_ga, const u64 *rev)
{
    TableRule<false> rule{M, g0, n, R, rev, out_pos, out_depth, out_meth, out_ctx, out_rev_g, out_rev_ga, 0, 0};
    compact_emit(rule, n, blk_start);
}

// PDR (bsx_meth_pdr_report_chr): the positions of the chromosome at g0 with reads >= min_reads (min_reads >= 1) on the cell's low word
struct PdrRule {
    struct Row { u64 cell; };
    const uint8_t *ref;
    const u64 *pdr;
    u64 g0;
    uint32_t min_reads;
    uint32_t *out_pos, *out_reads, *out_disc;
    uint8_t *out_letter;
    __device__ __forceinline__ bool row(u64 k, Row &w) const { w.cell = pdr[g0 + k]; return (uint32_t)w.cell >= min_reads; }
    __device__ __forceinline__ void store(u64 o, u64 k, const Row &w) const
    {
        out_pos[o] = (uint32_t)k; out_reads[o] = (uint32_t)w.cell; out_disc[o] = (uint32_t)(w.cell >> 32); out_letter[o] = ref[g0 + k];
    }
};

__global__ __launch_bounds__(256) void k_pdr_count(const u64 *pdr, u64 g0, u64 n, uint32_t min_reads, uint32_t *blk_rows)
{
    PdrRule rule{nullptr, pdr, g0, min_reads, nullptr, nullptr, nullptr, nullptr};
    compact_count(rule, n, blk_rows);
}

__global__ __launch_bounds__(256) void k_pdr_emit(const uint8_t *ref, const u64 *pdr, u64 g0, u64 n, uint32_t min_reads, const uint32_t *blk_start, uint32_t *out_pos,
                                                  uint32_t *out_reads, uint32_t *out_disc, uint8_t *out_letter)
{
    PdrRule rule{ref, pdr, g0, min_reads, out_pos, out_reads, out_disc, out_letter};
    compact_emit(rule, n, blk_start);
}

// Epialleles (bsx_meth_epi_report_chr): the chromosome's n windows in ordinal order, the first of them at the global ordinal o0, with reads >= min_reads
// (min_reads >= 1) on the sum of a window's sixteen cells.  A row is four positions and sixteen counts: the row number times 4 and times 16, in 64 bits
struct EpiRule {
    struct Row { uint4 v[4]; };
    const uint32_t *cells, *cpg_pos;
    u64 o0;
    uint32_t min_reads;
    uint32_t *out_pos, *out_counts;
    __device__ __forceinline__ bool row(u64 k, Row &w) const
    {
        const uint4 *c = (const uint4 *)(cells + (o0 + k) * 16);
        uint32_t sum = 0;
        for (int q = 0; q < 4; q++) { w.v[q] = c[q]; sum += w.v[q].x + w.v[q].y + w.v[q].z + w.v[q].w; }  // (< 2^32 alignments per handle: no carry)
        return sum >= min_reads;
    }
    __device__ __forceinline__ void store(u64 o, u64 k, const Row &w) const
    {
        for (int j = 0; j < 4; j++) out_pos[o * 4 + j] = cpg_pos[o0 + k + j];  // a window has its four CpGs in one chromosome
        uint4 *oc = (uint4 *)(out_counts + o * 16);
        for (int q = 0; q < 4; q++) oc[q] = w.v[q];
    }
};

__global__ __launch_bounds__(256) void k_epi_count(const uint32_t *cells, u64 o0, u64 n, uint32_t min_reads, uint32_t *blk_rows)
{
    EpiRule rule{cells, nullptr, o0, min_reads, nullptr, nullptr};
    compact_count(rule, n, blk_rows);
}

__global__ __launch_bounds__(256) void k_epi_emit(const uint32_t *cells, const uint32_t *cpg_pos, u64 o0, u64 n, uint32_t min_reads, const uint32_t *blk_start,
                                                  uint32_t *out_pos, uint32_t *out_counts)
{
    EpiRule rule{cells, cpg_pos, o0, min_reads, out_pos, out_counts};
    compact_emit(rule, n, blk_start);
}

// ---- pooled methylation per bin and per interval (bsx_meth_bins, bsx_meth_regions) ----
// A position is a site when meth_covered says so and its raw depth is above 0 (-z plays no part).  A site gives five values: 1, m, d, the effective depth
// e in units of 1/65536 (d << 16, or with the SNP mode on and g != ga the table's own double expression d * g / ga, scaled and rounded to nearest-even) and
// mc = min(m << 16, e), the table's min(mm, d) clip in those units.  All integers: sums of them are the same bits in any order.
// The one place that forms them; both kernels below call it, and it calls meth_covered for the row rule.  SNP = false: R.snp is 0, rev is not read, and the
// double division is not in the code.
template <bool SNP>
__device__ __forceinline__ bool meth_site(const MethDev &M, const u64 *rev, u64 g0, u64 n, u64 k, const RowRule &R, uint32_t &d, uint32_t &m, u64 &e, u64 &mc)
{
    uint32_t g, ga;
    const bool ok = meth_covered(M, rev, g0, n, k, R, d, m, g, ga) && d != 0;
    e = (u64)d << 16;
    if (SNP && ok && g != ga) e = (u64)rint((((double)d * g) / ga) * 65536.0);
    const u64 m16 = (u64)m << 16;
    mc = m16 < e ? m16 : e;
    return ok;
}

// Position-major: a block takes rounds * 256 consecutive positions of the chromosome [g0, g0 + n), a wave 64 consecutive ones per round.  The five values
// are reduced by bin inside the wave (a segmented reduction: the lanes' bins ascend, a lane adds its neighbour at distance 1, 2, .. 32 while that one is
// in the same bin, and the first lane of every bin ends with the bin's sum; with B >= 64 that is one or two segments, with B = 1 sixty-four), then
// across the waves in an LDS table of the bins the block touches, and reach HBM once per block and bin: plain stores for a bin that lies inside the
// block's positions (no other block touches it), 64-bit atomic adds for the one or two it shares with its neighbours.  A wave step without a site
// (the common case on sparse data) skips all of it.  LDS: ((P - 1) / B + 2) x 5 x 8 bytes, at most 40 KiB (B = 1, P = 1 024), given at the launch.
template <bool SNP>
__global__ __launch_bounds__(256) void k_meth_bins(MethDev M, u64 g0, u64 n, RowRule R, const u64 *rev, uint32_t B, uint32_t rounds, u64 *bins)
{
    extern __shared__ u64 s_bins[];  // [bins of the block][N, M, D, E, MC]
    const u64 P = (u64)rounds * 256, k0 = (u64)blockIdx.x * P, k1 = k0 + P < n ? k0 + P : n;  // k0 < n: the grid is ceil(n / P)
    const u64 bin_lo = k0 / B, rem0 = k0 % B;
    const uint32_t nb = (uint32_t)((k1 - 1) / B - bin_lo) + 1;
    for (uint32_t t = threadIdx.x; t < nb * 5; t += 256) s_bins[t] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    for (uint32_t r0 = 0; r0 < rounds; r0 += 4) {  // (rounds is a multiple of 4)
        // the raw depths of four rounds first, so that a wave has four loads in flight, not one; a wave step whose depths are all zero holds no site (the
        // site's own definition) and ends here, the others go through meth_site, which finds the depth in the cache
        uint32_t ahead[4];
        for (int q = 0; q < 4; q++) { const u64 ka = k0 + (u64)(r0 + q) * 256 + threadIdx.x; ahead[q] = ka < k1 ? M.depth[g0 + ka] : 0u; }
        for (int q = 0; q < 4; q++) {
            if (!__ballot(ahead[q] != 0)) continue;  // (uniform over the wave)
            const uint32_t o = (r0 + q) * 256 + threadIdx.x;
            const u64 k = k0 + o;
            uint32_t d = 0, m = 0;
            u64 e = 0, mc = 0;
            bool ok = false;
            if (k < k1) ok = meth_site<SNP>(M, rev, g0, n, k, R, d, m, e, mc);
            if (!__ballot(ok)) continue;
            // the lane's bin, counted from the block's first: (rem0 + o) / B without a 64-bit division (the sum is below 2 B whenever it is above 2^32)
            const u64 t = rem0 + (k < k1 ? o : (uint32_t)(k1 - 1 - k0));  // lanes behind the end hold zeroes in the last position's bin
            const uint32_t key = t <= 0xffffffffull ? (uint32_t)t / B : 1u;
            uint32_t vn = ok;
            u64 vm = ok ? m : 0u, vd = ok ? d : 0u, ve = ok ? e : 0ull, vmc = ok ? mc : 0ull;
            for (int off = 1; off < 64; off <<= 1) {
                const uint32_t ko = __shfl_down(key, off);
                const uint32_t an = __shfl_down(vn, off);
                const u64 am = __shfl_down(vm, off), ad = __shfl_down(vd, off), amc = __shfl_down(vmc, off);
                u64 ae = 0;
                if (SNP) ae = __shfl_down(ve, off);
                if (lane + off < 64 && ko == key) { vn += an; vm += am; vd += ad; vmc += amc; ve += ae; }
            }
            const uint32_t kp = __shfl_up(key, 1);
            if ((lane == 0 || kp != key) && vn) {
                if (!SNP) ve = vd << 16;  // the sum of d << 16
                u64 *c = &s_bins[key * 5];
                atomicAdd(&c[0], (u64)vn); atomicAdd(&c[1], vm); atomicAdd(&c[2], vd); atomicAdd(&c[3], ve); atomicAdd(&c[4], vmc);
            }
        }
    }
    __syncthreads();
    for (uint32_t t = threadIdx.x; t < nb; t += 256) {
        const u64 *c = &s_bins[t * 5];
        if (!c[0]) continue;  // no site: the cells in HBM stay zero
        const u64 b = bin_lo + t, lo = b * B, hi = lo + B < n ? lo + B : n;
        u64 *out = bins + b * 5;
        if (lo >= k0 && hi <= k1) { for (int q = 0; q < 5; q++) out[q] = c[q]; }
        else { for (int q = 0; q < 5; q++) atomicAdd(&out[q], c[q]); }
    }
}

// Interval-major: one wave per tile of at most bsx_meth_tiles::TILE positions (the host cuts the intervals: bsx_meth_tiles.h), the lanes stride the
// tile, so a wave's loads are 64 consecutive cells.  The context class near a tile's or an interval's border is the chromosome's: meth_context gets the
// chromosome's bounds through meth_site.  Lane 0 of the wave holds the tile's sums: where the tile is the interval's only one it writes them with plain
// stores.  The tiles of a longer interval follow each other in the tile list, so the block's REGION_WAVES waves mostly hold tiles of one interval: their
// sums meet in LDS, and the first wave of each run of equal intervals adds the run's total with five 64-bit atomic adds into the interval's zeroed
// cells (one set per block and interval, not one per tile: the five cells of an interval share a cache line, and a 2^27-nt interval has 65 536 tiles).
// Blocks of 4 waves where the launch is mostly short intervals (every wave of a block waits for its slowest at the barrier), of 16 where it is mostly
// long ones (a quarter of the adds): the host chooses per launch.
template <bool SNP, int REGION_WAVES>
__global__ __launch_bounds__(REGION_WAVES * 64) void k_meth_regions(MethDev M, RowRule R, const u64 *rev, const bsx_meth_tiles::Tile *tiles, uint32_t n_tiles,
                                                                   const uint32_t *iv_chr, const uint32_t *iv_start, u64 *sums)
{
    __shared__ u64 s_part[REGION_WAVES][5];
    __shared__ uint32_t s_iv[REGION_WAVES];  // the interval of the wave's tile where it has to be added, ~0 otherwise
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t t = blockIdx.x * REGION_WAVES + wv;
    uint32_t shared_iv = ~0u;
    if (t < n_tiles) {  // (uniform over the wave)
        const bsx_meth_tiles::Tile T = tiles[t];
        const uint32_t len = T.len & ~bsx_meth_tiles::SINGLE, c = iv_chr[T.iv];
        const u64 g0 = M.chr_off[c], n = M.chr_off[c + 1] - g0, k0 = (u64)iv_start[T.iv] + T.off;  // the host has clipped the interval: k0 + len <= n
        uint32_t vn = 0;
        u64 vm = 0, vd = 0, ve = 0, vmc = 0;
        for (uint32_t j0 = lane; j0 < len; j0 += 256) {  // four strides at a time: their raw depths first (four loads in flight); no site without depth
            uint32_t ahead[4];
            for (int q = 0; q < 4; q++) ahead[q] = j0 + 64 * q < len ? M.depth[g0 + k0 + j0 + 64 * q] : 0u;
            for (int q = 0; q < 4; q++) {
                if (!ahead[q]) continue;
                uint32_t d, m;
                u64 e, mc;
                if (!meth_site<SNP>(M, rev, g0, n, k0 + j0 + 64 * q, R, d, m, e, mc)) continue;
                vn++; vm += m; vd += d; vmc += mc;
                if (SNP) ve += e;
            }
        }
        for (int off = 32; off; off >>= 1) {
            vn += __shfl_down(vn, off); vm += __shfl_down(vm, off); vd += __shfl_down(vd, off); vmc += __shfl_down(vmc, off);
            if (SNP) ve += __shfl_down(ve, off);
        }
        if (!SNP) ve = vd << 16;
        if (lane == 0) {
            if (T.len & bsx_meth_tiles::SINGLE) { u64 *out = sums + (u64)T.iv * 5; out[0] = vn; out[1] = vm; out[2] = vd; out[3] = ve; out[4] = vmc; }
            else { shared_iv = T.iv; s_part[wv][0] = vn; s_part[wv][1] = vm; s_part[wv][2] = vd; s_part[wv][3] = ve; s_part[wv][4] = vmc; }
        }
    }
    if (lane == 0) s_iv[wv] = shared_iv;
    __syncthreads();
    if (lane != 0 || shared_iv == ~0u || (wv > 0 && s_iv[wv - 1] == shared_iv)) return;  // the first wave of a run of tiles of one interval goes on
    u64 tot[5] = {0, 0, 0, 0, 0};
    for (int w = wv; w < REGION_WAVES && s_iv[w] == shared_iv; w++) for (int q = 0; q < 5; q++) tot[q] += s_part[w][q];
    if (!tot[0]) return;
    u64 *out = sums + (u64)shared_iv * 5;
    for (int q = 0; q < 5; q++) atomicAdd(&out[q], tot[q]);
}

// ---- two samples: differential methylation (bsx_meth_diff_report_chr, bsx_meth_diff_regions) ----
// Position k is a COMMON SITE of the samples A and B when meth_covered holds for it in both (R.snp is 0: no rev cells) and both raw depths are above 0.
// B is B's counters under A's letters and offsets (the host builds it so).  The one place that says it: the rows and the interval sums both ask here.
__device__ __forceinline__ bool diff_site(const MethDev &A, const MethDev &B, u64 g0, u64 n, u64 k, const RowRule &R, uint32_t &dA, uint32_t &mA, uint32_t &dB, uint32_t &mB)
{
    uint32_t g, ga;
    dB = mB = 0;
    if (!meth_covered(A, nullptr, g0, n, k, R, dA, mA, g, ga) || dA == 0) return false;
    return meth_covered(B, nullptr, g0, n, k, R, dB, mB, g, ga) && dB != 0;
}

// The rows (bsx_meth_diff_report_chr): the common sites whose ratios differ by at least permille / 1000: |mA dB - mB dA| 1000 >= permille dA dB, both
// sides as 128-bit integers (a product of two 32-bit counts fits 64 bits).  cls: bits 0-1 the context class, bit 2 set over a G
struct DiffRule {
    struct Row { uint32_t mA, dA, mB, dB; };
    MethDev A, B;
    u64 g0, n;
    RowRule R;
    uint32_t permille;
    uint32_t *out_pos;
    uint4 *out_counts;
    uint8_t *out_cls;
    __device__ __forceinline__ bool row(u64 k, Row &w) const
    {
        if (!diff_site(A, B, g0, n, k, R, w.dA, w.mA, w.dB, w.mB)) return false;
        return bsx_meth_diff::delta_keeps(w.mA, w.dA, w.mB, w.dB, permille);
    }
    __device__ __forceinline__ void store(u64 o, u64 k, const Row &w) const
    {
        const bool plus = A.ref[g0 + k] == 'C';
        out_pos[o] = (uint32_t)k; out_counts[o] = make_uint4(w.mA, w.dA, w.mB, w.dB);
        out_cls[o] = (uint8_t)(meth_context(A.ref, g0 + k, g0, g0 + n, plus) | (plus ? 0u : 4u));
    }
};

__global__ __launch_bounds__(256) void k_diff_count(MethDev A, MethDev B, u64 g0, u64 n, RowRule R, uint32_t permille, uint32_t *blk_rows)
{
    DiffRule rule{A, B, g0, n, R, permille, nullptr, nullptr, nullptr};
    compact_count(rule, n, blk_rows);
}

__global__ __launch_bounds__(256) void k_diff_emit(MethDev A, MethDev B, u64 g0, u64 n, RowRule R, uint32_t permille, const uint32_t *blk_start, uint32_t *out_pos,
                                                   uint4 *out_counts, uint8_t *out_cls)
{
    DiffRule rule{A, B, g0, n, R, permille, out_pos, out_counts, out_cls};
    compact_emit(rule, n, blk_start);
}

// p of every row, a thread per row: over the compacted rows of k_diff_emit (rows4: mA, dA, mB, dB) or over interval sums (sums5: N, MA, DA, MB, DB; NaN
// where N == 0), whichever pointer is not null.  Every lane has a row; the lanes of a wave differ in the length of their walks (the row's support).
__global__ __launch_bounds__(256) void k_meth_fisher(const uint4 *rows4, const u64 *sums5, u64 n, double *p)
{
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (rows4) {
        const uint4 c = rows4[i];
        p[i] = bsx_meth_diff::fisher_p((double)c.x, (double)c.y, (double)c.z, (double)c.w);
    } else {
        const u64 *s = sums5 + i * 5;
        p[i] = s[0] ? bsx_meth_diff::fisher_p((double)s[1], (double)s[2], (double)s[3], (double)s[4]) : __longlong_as_double(0x7ff8000000000000ll);
    }
}

// The joint form of k_meth_regions<false, REGION_WAVES>: the same tiles, one wave per tile, the same meeting of a block's waves in LDS; the five sums of an
// interval are N, MA, DA, MB, DB over its common sites.  No common site without a depth in A: the look-ahead loads are A's.
template <int REGION_WAVES>
__global__ __launch_bounds__(REGION_WAVES * 64) void k_meth_diff_regions(MethDev A, MethDev B, RowRule R, const bsx_meth_tiles::Tile *tiles, uint32_t n_tiles,
                                                                        const uint32_t *iv_chr, const uint32_t *iv_start, u64 *sums)
{
    __shared__ u64 s_part[REGION_WAVES][5];
    __shared__ uint32_t s_iv[REGION_WAVES];  // the interval of the wave's tile where it has to be added, ~0 otherwise
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t t = blockIdx.x * REGION_WAVES + wv;
    uint32_t shared_iv = ~0u;
    if (t < n_tiles) {  // (uniform over the wave)
        const bsx_meth_tiles::Tile T = tiles[t];
        const uint32_t len = T.len & ~bsx_meth_tiles::SINGLE, c = iv_chr[T.iv];
        const u64 g0 = A.chr_off[c], n = A.chr_off[c + 1] - g0, k0 = (u64)iv_start[T.iv] + T.off;  // the host has clipped the interval: k0 + len <= n
        u64 v[5] = {0, 0, 0, 0, 0};
        for (uint32_t j0 = lane; j0 < len; j0 += 256) {
            uint32_t ahead[4];
            for (int q = 0; q < 4; q++) ahead[q] = j0 + 64 * q < len ? A.depth[g0 + k0 + j0 + 64 * q] : 0u;
            for (int q = 0; q < 4; q++) {
                if (!ahead[q]) continue;
                uint32_t dA, mA, dB, mB;
                if (!diff_site(A, B, g0, n, k0 + j0 + 64 * q, R, dA, mA, dB, mB)) continue;
                v[0]++; v[1] += mA; v[2] += dA; v[3] += mB; v[4] += dB;
            }
        }
        for (int off = 32; off; off >>= 1) for (int q = 0; q < 5; q++) v[q] += __shfl_down(v[q], off);
        if (lane == 0) {
            if (T.len & bsx_meth_tiles::SINGLE) { u64 *out = sums + (u64)T.iv * 5; for (int q = 0; q < 5; q++) out[q] = v[q]; }
            else { shared_iv = T.iv; for (int q = 0; q < 5; q++) s_part[wv][q] = v[q]; }
        }
    }
    if (lane == 0) s_iv[wv] = shared_iv;
    __syncthreads();
    if (lane != 0 || shared_iv == ~0u || (wv > 0 && s_iv[wv - 1] == shared_iv)) return;  // the first wave of a run of tiles of one interval goes on
    u64 tot[5] = {0, 0, 0, 0, 0};
    for (int w = wv; w < REGION_WAVES && s_iv[w] == shared_iv; w++) for (int q = 0; q < 5; q++) tot[q] += s_part[w][q];
    if (!tot[0]) return;
    u64 *out = sums + (u64)shared_iv * 5;
    for (int q = 0; q < 5; q++) atomicAdd(&out[q], tot[q]);
}

// ---- Benjamini-Hochberg q-values (bsx_meth_bh and the store of bsx_meth_diff_report_all) ----
// The key of a p-value is its bit pattern (p >= 0: the order of the bits is the order of the values; -0.0 counts as 0.0); a NaN is outside the family and
// gets the largest key, so that the sort leaves the family in front.  nan_count: one integer add per block that holds a NaN.
constexpr u64 BH_NAN_KEY = ~0ull;

__global__ __launch_bounds__(256) void k_bh_keys(const double *p, u64 n, u64 *keys, uint32_t *idx, u64 *nan_count)
{
    __shared__ uint32_t s_nan;
    if (threadIdx.x == 0) s_nan = 0;
    __syncthreads();
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    bool nan = false;
    if (i < n) {
        const double x = p[i];
        nan = x != x;
        keys[i] = nan ? BH_NAN_KEY : (x == 0.0 ? 0ull : (u64)__double_as_longlong(x));
        idx[i] = (uint32_t)i;
    }
    const u64 bal = __ballot(nan);
    if ((threadIdx.x & 63) == 0 && bal) atomicAdd(&s_nan, (uint32_t)__builtin_popcountll(bal));
    __syncthreads();
    if (threadIdx.x == 0 && s_nan) atomicAdd(nan_count, (u64)s_nan);
}

// r_k = (p_(k) n_fam) / k for the k-th smallest p of a family of n_fam = n - *nan_count, k from 1: two roundings, the product first (no contraction is
// possible between a product and a quotient; the intrinsics say so).  Written back to front, r[n - 1 - j] for the sorted place j = k - 1, so that the
// suffix minimum of the definition is a forward inclusive scan; the places of the NaN keys, which are in front then, hold +inf.
__global__ __launch_bounds__(256) void k_bh_ratio(const u64 *sorted_keys, u64 n, const u64 *nan_count, double *r_rev)
{
    const u64 j = (u64)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const u64 n_fam = n - *nan_count;
    r_rev[n - 1 - j] = j < n_fam ? __ddiv_rn(__dmul_rn(__longlong_as_double((long long)sorted_keys[j]), (double)n_fam), (double)(j + 1))
                                 : __longlong_as_double(0x7ff0000000000000ll);
}

// q of the row at sorted place j: min(1, the suffix minimum at j), NaN outside the family.  Every row is written once: plain stores.
__global__ __launch_bounds__(256) void k_bh_scatter(const double *min_rev, const uint32_t *sorted_idx, u64 n, const u64 *nan_count, double *q)
{
    const u64 j = (u64)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const double v = min_rev[n - 1 - j];
    q[sorted_idx[j]] = j < n - *nan_count ? (v < 1.0 ? v : 1.0) : __longlong_as_double(0x7ff8000000000000ll);
}

struct MinDouble {
    __host__ __device__ double operator()(double a, double b) const { return b < a ? b : a; }
};

// ---- de novo DMRs over the store (bsx_meth_diff_dmrs) ----
// The store of bsx_meth_diff_report_all as the kernels see it: row_start[n_seq + 1] in the writer's sequence order, per row pos, counts and q
struct StoreDev {
    const uint32_t *row_start, *pos;
    const uint4 *counts;
    const double *q;
    uint32_t n_seq;
};

// A CANDIDATE is a row of the store with q <= max_q that passes the delta rule and whose ratios differ (sign != 0).  Items are store rows.  Payload: the
// row's position and key = (rank of its sequence in the writer's order) * 2 + (1 where B's ratio is the higher one): two candidates may share a
// run only under one key.
struct CandRule {
    struct Row { uint32_t key; };
    StoreDev S;
    double max_q;
    uint32_t permille;
    uint32_t *out_key, *out_pos;
    __device__ __forceinline__ bool row(u64 i, Row &w) const
    {
        const uint4 c = S.counts[i];
        const int s = bsx_meth_diff::delta_sign(c.x, c.y, c.z, c.w);
        w.key = s > 0 ? 1u : 0u;
        return s != 0 && S.q[i] <= max_q && bsx_meth_diff::delta_keeps(c.x, c.y, c.z, c.w, permille);
    }
    __device__ __forceinline__ void store(u64 o, u64 i, const Row &w) const
    {
        uint32_t lo = 0, hi = S.n_seq;  // the sequence with row_start[lo] <= i < row_start[lo + 1]: the last lo with row_start[lo] <= i
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (S.row_start[mid] <= (uint32_t)i) lo = mid; else hi = mid;
        }
        out_key[o] = lo * 2 + w.key; out_pos[o] = S.pos[i];
    }
};

__global__ __launch_bounds__(256) void k_cand_count(StoreDev S, u64 n, double max_q, uint32_t permille, uint32_t *blk_rows)
{
    CandRule rule{S, max_q, permille, nullptr, nullptr};
    compact_count(rule, n, blk_rows);
}

__global__ __launch_bounds__(256) void k_cand_emit(StoreDev S, u64 n, double max_q, uint32_t permille, const uint32_t *blk_start, uint32_t *out_key, uint32_t *out_pos)
{
    CandRule rule{S, max_q, permille, out_key, out_pos};
    compact_emit(rule, n, blk_start);
}

// Candidate j is the HEAD of a run when it is the first one, or its key differs from its predecessor's (another sequence or another direction), or it lies
// more than max_gap nt behind it (positions ascend within a key).  Items are candidates; payload: the candidate's index.
struct HeadRule {
    struct Row {};
    const uint32_t *key, *pos;
    uint32_t max_gap;
    uint32_t *out_head;
    __device__ __forceinline__ bool row(u64 j, Row &) const { return j == 0 || key[j] != key[j - 1] || pos[j] - pos[j - 1] > max_gap; }
    __device__ __forceinline__ void store(u64 o, u64 j, const Row &) const { out_head[o] = (uint32_t)j; }
};

__global__ __launch_bounds__(256) void k_head_count(const uint32_t *key, const uint32_t *pos, u64 n, uint32_t max_gap, uint32_t *blk_rows)
{
    HeadRule rule{key, pos, max_gap, nullptr};
    compact_count(rule, n, blk_rows);
}

__global__ __launch_bounds__(256) void k_head_emit(const uint32_t *key, const uint32_t *pos, u64 n, uint32_t max_gap, const uint32_t *blk_start, uint32_t *out_head)
{
    HeadRule rule{key, pos, max_gap, out_head};
    compact_emit(rule, n, blk_start);
}

// A thread per run: the candidates [head[o], head[o + 1]) (the last run ends with the last candidate) as (sequence id, start, end, n_sig), the span
// [pos_first, pos_last + 1).  order[rank]: the sequence id at a rank of the writer's order.
__global__ __launch_bounds__(256) void k_dmr_runs(const uint32_t *head, uint32_t n_runs, uint32_t n_cand, const uint32_t *key, const uint32_t *pos, const uint32_t *order,
                                                  uint4 *runs)
{
    const uint32_t o = blockIdx.x * 256 + threadIdx.x;
    if (o >= n_runs) return;
    const uint32_t first = head[o], last = (o + 1 < n_runs ? head[o + 1] : n_cand) - 1;
    runs[o] = make_uint4(order[key[first] >> 1], pos[first], pos[last] + 1, last - first + 1);
}

}  // namespace

enum Count { CNT_VALID, CNT_NC, CNT_ND, CNT_DROPPED, CNT_CELLS = 8 };  // d_counts: valid alignments, the nc and nd of the last table report, alignments the non-conversion filter dropped

// a value no earlier call has returned (from 1): the identity of a handle's state, for the store of bsx_meth_diff_report_all
static u64 meth_next_stamp()
{
    static std::atomic<u64> stamp{0};
    return ++stamp;
}

struct bsx_meth {
    int device = 0;
    uint32_t n_chr = 0;
    std::vector<u64> chr_off;
    DevBuf<uint8_t> d_ref;
    DevBuf<u64> d_chr_off, d_counts;
    DevBuf<uint32_t> d_depth, d_meth, d_first;  // d_first: empty without the duplicate filter
    uint32_t index_base = 0;
    uint32_t trim5 = 0, trim3 = 0;  // bsx_meth_set_cycle_trim
    int snp = 0;                    // bsx_meth_set_ct_snp: 0 off, 1 correct, 2 skip
    uint32_t ctx_mask = 0;          // bsx_meth_set_contexts
    DevBuf<u64> d_rev;              // the packed opposite-strand counters, (total + 16) cells, or empty when snp == 0
    DevBuf<u64> d_mbias;            // bsx_meth_set_mbias: MB_CELLS cells and the overflow counter, or empty
    uint32_t nonconv = 0, min_cpg = 0;  // bsx_meth_set_nonconv, bsx_meth_set_pdr
    DevBuf<u64> d_hist;             // bsx_meth_set_read_stats: RS_CELLS cells, or empty
    DevBuf<u64> d_pdr;              // the packed PDR cells, (total + 16) of them, or empty when min_cpg == 0
    int epi = 0;                    // bsx_meth_set_epi
    bool cpg_built = false;         // the CpG index and the cells below exist (meth_epi_index builds them at the first add or report that needs them)
    DevBuf<uint32_t> d_cpg_dir, d_cpg_pos, d_epi;  // rank directory, positions by ordinal, 16 cells per CpG (EpiDev)
    std::vector<uint32_t> cpg_first;  // [n_chr + 1] the global ordinal of every chromosome's first CpG, then the number of CpGs
    int n_cu = 0;
    hipStream_t stream = nullptr;
    // what the reports share (meth_compact): per-block row counts, their scan, the scan's scratch
    DevBuf<uint32_t> d_blk, d_blk_start;
    DevBuf<char> d_temp;
    // the rows of the last bsx_meth_report_chr: pos, depth, meth, packed context, and with snp != 0 rev_G / rev_GA
    DevBuf<uint32_t> d_out[3], d_out_rev[2];
    DevBuf<u64> d_ctx;
    uint32_t last_rows = 0;
    // of the last bsx_meth_pdr_report_chr: pos, reads, discordant, reference letter
    DevBuf<uint32_t> d_pdr_out[3];
    DevBuf<uint8_t> d_pdr_letter;
    uint32_t pdr_last_rows = 0;
    // of the last bsx_meth_epi_report_chr: pos[rows][4], counts[rows][16]
    DevBuf<uint32_t> d_epi_out[2];
    uint32_t epi_last_rows = 0;
    // of the last bsx_meth_diff_report_chr with this handle as sample A: pos, counts[rows][4] (mA, dA, mB, dB), context class and strand, p
    DevBuf<uint32_t> d_diff_pos;
    DevBuf<uint4> d_diff_counts;
    DevBuf<uint8_t> d_diff_cls;
    DevBuf<double> d_diff_p;
    uint32_t diff_last_rows = 0;
    // The genome-wide store of the last bsx_meth_diff_report_all with this handle as sample A: every common site of every sequence in the
    // writer's sequence order (store_order[rank] = sequence id), row_start[n_chr + 1] by rank, and per row pos, counts, class byte, p and q: 37 bytes a row.
    // It stands for (sample B, store_min_depth) while neither handle's counters, letters or context mask have changed since: `changes` is a stamp from one
    // process-wide counter, new at create and at every such change, so no two handles and no two states of one handle ever share a value (a handle made
    // at the address of a destroyed one is another sample B).
    DevBuf<uint32_t> d_store_row_start, d_store_order, d_store_pos;
    DevBuf<uint4> d_store_counts;
    DevBuf<uint8_t> d_store_cls;
    DevBuf<double> d_store_p, d_store_q;
    std::vector<uint32_t> store_row_start, store_order;
    bool store_valid = false;
    uint32_t store_min_depth = 0;
    u64 store_changes_a = 0, store_changes_b = 0;
    u64 changes = meth_next_stamp();  // renewed by the calls that change what a diff call reads: add, combine_cpg, set_reference, set_contexts
    // of the last bsx_meth_diff_dmrs: (sequence id, start, end, n_sig) per DMR, its five sums and p
    std::vector<uint32_t> dmr_runs;
    std::vector<uint64_t> dmr_sums;
    std::vector<double> dmr_p;
    std::vector<std::string> names;  // filled by bsx_meth_create_from_fasta
    MethDev dev() const { MethDev M; M.ref = d_ref.p; M.chr_off = d_chr_off.p; M.depth = d_depth.p; M.meth = d_meth.p; M.first = d_first.p; M.total = chr_off.back(); M.n_chr = n_chr; return M; }
};

// out[k] = in[0] + .. + in[k - 1] for k < n, on the handle's stream and with its scratch buffer
static int meth_scan_u32(bsx_meth *m, uint32_t *in, uint32_t *out, size_t n)
{
    size_t need = 0;
    HIP_TRY(rocprim::exclusive_scan(nullptr, need, in, out, 0u, n, rocprim::plus<uint32_t>(), m->stream));
    HIP_TRY(m->d_temp.reserve(need));
    HIP_TRY(rocprim::exclusive_scan(m->d_temp.p, need, in, out, 0u, n, rocprim::plus<uint32_t>(), m->stream));
    return BSX_OK;
}

// ---- the CpG index of the epiallele tally ----
static void meth_epi_drop_index(bsx_meth *m)
{
    m->d_cpg_dir.reset(); m->d_cpg_pos.reset(); m->d_epi.reset();
    m->cpg_first.clear();
    m->cpg_built = false; m->epi_last_rows = 0;
}

// Builds what is missing of EpiDev: per-block counts, their scan (the directory), the ordinal of every chromosome's first CpG, the positions, zeroed cells.
// Ordinals are 32 bits wide: a text of 2^33 letters or more could hold more CpGs than that and is refused.
static int meth_epi_index(bsx_meth *m)
{
    if (m->cpg_built) return BSX_OK;
    const u64 total = m->chr_off.back(), n_blocks = (total + 63) / 64;
    if (total >= (1ull << 33)) { g_bsx_err = "the epiallele tally takes a reference of fewer than 2^33 letters"; return BSX_ERR_LIMIT; }
    DevBuf<uint32_t> d_cnt, d_first;
    const MethDev M = m->dev();
    const size_t n_first = (size_t)m->n_chr + 1;
    auto build = [&]() -> int {
        HIP_TRY(d_cnt.reserve((n_blocks + 1) * 4)); HIP_TRY(m->d_cpg_dir.reserve((n_blocks + 1) * 4)); HIP_TRY(d_first.reserve(n_first * 4));
        HIP_TRY(hipMemsetAsync(d_cnt.p + n_blocks, 0, 4, m->stream));
        if (n_blocks) { hipLaunchKernelGGL(k_cpg_count, dim3((unsigned)((n_blocks + 3) / 4)), dim3(256), 0, m->stream, M, n_blocks, d_cnt.p); HIP_TRY(hipGetLastError()); }
        const int rc = meth_scan_u32(m, d_cnt.p, m->d_cpg_dir.p, (size_t)n_blocks + 1);
        if (rc) return rc;
        hipLaunchKernelGGL(k_cpg_chr_first, dim3(m->n_chr + 1), dim3(64), 0, m->stream, M, (const uint32_t *)m->d_cpg_dir.p, d_first.p);
        HIP_TRY(hipGetLastError());
        m->cpg_first.assign(n_first, 0);
        HIP_TRY(hipMemcpyAsync(m->cpg_first.data(), d_first.p, n_first * 4, hipMemcpyDeviceToHost, m->stream));
        HIP_TRY(hipStreamSynchronize(m->stream));
        const size_t n_cpg = m->cpg_first.back();
        HIP_TRY(m->d_cpg_pos.reserve((n_cpg + 4) * 4));
        HIP_TRY(m->d_epi.zeroed((n_cpg + 1) * 64, m->stream));
        if (n_blocks) {
            hipLaunchKernelGGL(k_cpg_emit, dim3((unsigned)((n_blocks + 3) / 4)), dim3(256), 0, m->stream, M, n_blocks, (const uint32_t *)m->d_cpg_dir.p, m->d_cpg_pos.p);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipStreamSynchronize(m->stream));
        }
        return BSX_OK;
    };
    const int rc = build();
    if (rc != BSX_OK) { meth_epi_drop_index(m); return rc; }
    m->cpg_built = true;
    return BSX_OK;
}

extern "C" void bsx_meth_destroy(bsx_meth *m)
{
    if (!m) return;
    (void)hipSetDevice(m->device);  // ahead of the buffers' release
    if (m->stream) (void)hipStreamDestroy(m->stream);
    delete m;
}

extern "C" int bsx_meth_create(uint32_t n_chr, const uint64_t *chr_len, int rm_dup, int device, bsx_meth **out)
{
    if (!n_chr || !chr_len || !out) return BSX_ERR_ARG;
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || nd <= 0) { g_bsx_err = "no HIP device visible; libbsx has no CPU fallback"; return BSX_ERR_NODEVICE; }
    if (device < 0 || device >= nd) return BSX_ERR_NODEVICE;
    HIP_TRY(hipSetDevice(device));
    bsx_meth *m = new bsx_meth();
    m->device = device; m->n_chr = n_chr;
    if (hipDeviceGetAttribute(&m->n_cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || m->n_cu <= 0) { delete m; return BSX_ERR_DEVICE; }
    m->chr_off.assign(1, 0);
    for (uint32_t c = 0; c < n_chr; c++) m->chr_off.push_back(m->chr_off.back() + chr_len[c]);
    const u64 total = m->chr_off.back();
    auto fail = [&](int rc) { bsx_meth_destroy(m); return rc; };
    if (hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking) != hipSuccess) return fail(BSX_ERR_DEVICE);
    if (m->d_ref.reserve(total + 16) != hipSuccess || m->d_depth.reserve((total + 16) * 4) != hipSuccess || m->d_meth.reserve((total + 16) * 4) != hipSuccess ||
        m->d_chr_off.reserve((n_chr + 1) * 8) != hipSuccess || m->d_counts.reserve(CNT_CELLS * 8) != hipSuccess)
        return fail(BSX_ERR_NOMEM);
    if (rm_dup && m->d_first.reserve(2 * (total + 16) * 4) != hipSuccess) return fail(BSX_ERR_NOMEM);
    if (hipMemsetAsync(m->d_ref.p, 0, total + 16, m->stream) != hipSuccess || hipMemsetAsync(m->d_depth.p, 0, (total + 16) * 4, m->stream) != hipSuccess ||
        hipMemsetAsync(m->d_meth.p, 0, (total + 16) * 4, m->stream) != hipSuccess || hipMemsetAsync(m->d_counts.p, 0, CNT_CELLS * 8, m->stream) != hipSuccess)
        return fail(BSX_ERR_DEVICE);
    if (rm_dup && hipMemsetAsync(m->d_first.p, 0xff, 2 * (total + 16) * 4, m->stream) != hipSuccess) return fail(BSX_ERR_DEVICE);
    if (hipMemcpyAsync(m->d_chr_off.p, m->chr_off.data(), (n_chr + 1) * 8, hipMemcpyHostToDevice, m->stream) != hipSuccess) return fail(BSX_ERR_DEVICE);
    if (hipStreamSynchronize(m->stream) != hipSuccess) return fail(BSX_ERR_DEVICE);
    *out = m;
    return BSX_OK;
}

extern "C" int bsx_meth_set_reference(bsx_meth *m, uint32_t chr, const char *upper_seq)
{
    if (!m || chr >= m->n_chr || !upper_seq) return BSX_ERR_ARG;
    HIP_TRY(hipSetDevice(m->device));
    if (m->cpg_built) meth_epi_drop_index(m);  // other letters, other CpGs: the index and the cells are built again when they are next needed
    m->changes = meth_next_stamp();
    HIP_TRY(hipMemcpy(m->d_ref.p + m->chr_off[chr], upper_seq, m->chr_off[chr + 1] - m->chr_off[chr], hipMemcpyHostToDevice));
    return BSX_OK;
}

extern "C" int bsx_meth_add(bsx_meth *m, uint32_t n, const uint32_t *chr, const int64_t *pos, const uint8_t *strand, const int32_t *insert, const int64_t *cut_at,
                            const char *seqs, const uint64_t *seq_off, uint32_t trim_fillin)
{
    if (!m || (n && (!chr || !pos || !strand || !insert || !cut_at || !seqs || !seq_off))) return BSX_ERR_ARG;
    if (!n) return BSX_OK;
    if ((u64)m->index_base + n >= 0xFFFFFFFFull) return BSX_ERR_LIMIT;
    for (uint32_t i = 0; i < n; i++) if (chr[i] >= m->n_chr || strand[i] > 3) return BSX_ERR_ARG;
    HIP_TRY(hipSetDevice(m->device));
    m->changes = meth_next_stamp();
    if (m->epi) { const int erc = meth_epi_index(m); if (erc) return erc; }
    const u64 nbytes = seq_off[n];
    uint32_t *d_chr = nullptr; int64_t *d_pos = nullptr, *d_cut = nullptr; uint8_t *d_strand = nullptr, *d_seq = nullptr, *d_drop = nullptr; int32_t *d_ins = nullptr; u64 *d_off = nullptr;
    int rc = BSX_OK;
    auto chk = [&](hipError_t e) { if (e != hipSuccess && rc == BSX_OK) rc = bsx_hip_fail(e, "bsx_meth_add", __FILE__, __LINE__); };
    chk(hipMalloc((void **)&d_chr, (size_t)n * 4)); chk(hipMalloc((void **)&d_pos, (size_t)n * 8)); chk(hipMalloc((void **)&d_cut, (size_t)n * 8));
    chk(hipMalloc((void **)&d_strand, n)); chk(hipMalloc((void **)&d_ins, (size_t)n * 4)); chk(hipMalloc((void **)&d_seq, nbytes + 16)); chk(hipMalloc((void **)&d_off, ((size_t)n + 1) * 8));
    if (m->nonconv) chk(hipMalloc((void **)&d_drop, n));
    if (rc == BSX_OK) {
        chk(hipMemcpyAsync(d_chr, chr, (size_t)n * 4, hipMemcpyHostToDevice, m->stream)); chk(hipMemcpyAsync(d_pos, pos, (size_t)n * 8, hipMemcpyHostToDevice, m->stream));
        chk(hipMemcpyAsync(d_cut, cut_at, (size_t)n * 8, hipMemcpyHostToDevice, m->stream)); chk(hipMemcpyAsync(d_strand, strand, n, hipMemcpyHostToDevice, m->stream));
        chk(hipMemcpyAsync(d_ins, insert, (size_t)n * 4, hipMemcpyHostToDevice, m->stream)); chk(hipMemcpyAsync(d_seq, seqs, nbytes, hipMemcpyHostToDevice, m->stream));
        chk(hipMemcpyAsync(d_off, seq_off, ((size_t)n + 1) * 8, hipMemcpyHostToDevice, m->stream));
    }
    if (rc == BSX_OK) {
        AlnBatch B; B.chr = d_chr; B.pos = d_pos; B.strand = d_strand; B.insert = d_ins; B.cut_at = d_cut; B.seq = d_seq; B.seq_off = d_off;
        B.n = n; B.index_base = m->index_base; B.trim_fillin = trim_fillin; B.trim5 = m->trim5; B.trim3 = m->trim3; B.drop = nullptr;
        const MethDev M = m->dev();
        u64 *const n_valid = m->d_counts.p + CNT_VALID, *const rev = m->d_rev.p;
        if (M.first) hipLaunchKernelGGL(k_meth_first, dim3((n + 255) / 256), dim3(256), 0, m->stream, M, B);
        if (m->nonconv || m->d_hist.p || m->d_pdr.p) {  // the per-read pass: it sees the unfiltered window (B.drop is still null) and writes every flag of d_drop
            const unsigned waves = RS_BLOCK / 64, grid = (unsigned)std::min<u64>((u64)m->n_cu * RS_BLOCKS_PER_CU, ((u64)n + waves - 1) / waves);
            const ReadsDev R{m->d_hist.p, m->d_pdr.p, m->d_counts.p + CNT_DROPPED, d_drop, m->nonconv, m->min_cpg};
            hipLaunchKernelGGL(k_meth_reads, dim3(grid), dim3(RS_BLOCK), 0, m->stream, M, B, R);
            B.drop = d_drop;
        }
        if (m->epi)  // behind the verdicts of the non-conversion filter, ahead of the pile-up
            hipLaunchKernelGGL(k_meth_epi, dim3((n + 3) / 4), dim3(256), 0, m->stream, M, B, EpiDev{m->d_cpg_dir.p, m->d_epi.p, (u64)m->cpg_first.back()});
        if (m->d_mbias.p) {  // the grid comes from the CU count; a batch too small to give every wave an alignment gets fewer blocks (fewer flushes)
            const unsigned waves = MB_BLOCK / 64, grid = (unsigned)std::min<u64>((u64)m->n_cu * MB_BLOCKS_PER_CU, ((u64)n + waves - 1) / waves);
            const MbiasDev D{m->d_mbias.p, m->d_mbias.p + MB_CELLS};
            if (rev) hipLaunchKernelGGL(k_meth_pile_mbias<true>, dim3(grid), dim3(MB_BLOCK), 0, m->stream, M, B, n_valid, D, rev);
            else hipLaunchKernelGGL(k_meth_pile_mbias<false>, dim3(grid), dim3(MB_BLOCK), 0, m->stream, M, B, n_valid, D, rev);
        } else if (rev)
            hipLaunchKernelGGL(k_meth_pile<true>, dim3((n + 3) / 4), dim3(256), 0, m->stream, M, B, n_valid, rev);
        else
            hipLaunchKernelGGL(k_meth_pile<false>, dim3((n + 3) / 4), dim3(256), 0, m->stream, M, B, n_valid, rev);
        chk(hipGetLastError());
        chk(hipStreamSynchronize(m->stream));
        m->index_base += n;
    }
    for (void *q : {(void *)d_chr, (void *)d_pos, (void *)d_cut, (void *)d_strand, (void *)d_ins, (void *)d_seq, (void *)d_off, (void *)d_drop}) if (q) (void)hipFree(q);
    return rc;
}

extern "C" int bsx_meth_set_cycle_trim(bsx_meth *m, uint32_t trim5, uint32_t trim3)
{
    if (!m) return BSX_ERR_ARG;
    m->trim5 = trim5; m->trim3 = trim3;
    return BSX_OK;
}

extern "C" int bsx_meth_set_mbias(bsx_meth *m, int on)
{
    if (!m) return BSX_ERR_ARG;
    if (m->index_base) { g_bsx_err = "bsx_meth_set_mbias after alignments have been added"; return BSX_ERR_STATE; }
    HIP_TRY(hipSetDevice(m->device));
    if (!on) m->d_mbias.reset();
    else if (!m->d_mbias.p) HIP_TRY(m->d_mbias.zeroed((MB_CELLS + 1) * 8, m->stream));
    return BSX_OK;
}

extern "C" int bsx_meth_set_ct_snp(bsx_meth *m, int mode)
{
    if (!m || mode < 0 || mode > 2) return BSX_ERR_ARG;
    if ((mode != 0) == (m->snp != 0)) { m->snp = mode; return BSX_OK; }  // 1 <-> 2 at any time: the counters are the same
    if (m->index_base) { g_bsx_err = "bsx_meth_set_ct_snp on or off after alignments have been added"; return BSX_ERR_STATE; }
    HIP_TRY(hipSetDevice(m->device));
    if (!mode) m->d_rev.reset();
    else HIP_TRY(m->d_rev.zeroed((size_t)(m->chr_off.back() + 16) * 8, m->stream));
    m->snp = mode;
    return BSX_OK;
}

extern "C" int bsx_meth_set_contexts(bsx_meth *m, uint32_t mask)
{
    if (!m || mask > 0xF) return BSX_ERR_ARG;
    m->ctx_mask = mask;
    m->changes = meth_next_stamp();
    return BSX_OK;
}

extern "C" int bsx_meth_mbias_fetch(bsx_meth *m, uint64_t *cells, uint64_t *overflow_calls)
{
    if (!m || !cells) return BSX_ERR_ARG;
    if (!m->d_mbias.p) { g_bsx_err = "the M-bias tally is off (bsx_meth_set_mbias)"; return BSX_ERR_STATE; }
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipMemcpy(cells, m->d_mbias.p, MB_CELLS * 8, hipMemcpyDeviceToHost));
    if (overflow_calls) HIP_TRY(hipMemcpy(overflow_calls, m->d_mbias.p + MB_CELLS, 8, hipMemcpyDeviceToHost));
    return BSX_OK;
}

// ---- what the file writers and readers share ----
namespace {

// no C++ exception may cross the C ABI: fn() with a failed host allocation as BSX_ERR_NOMEM and any other exception as BSX_ERR_IO; `doing`: "writing" or "reading"
template <class Fn>
int guarded(const char *path, const char *doing, Fn fn)
{
    try {
        return fn();
    } catch (const std::bad_alloc &) {
        g_bsx_err = std::string("out of host memory while ") + doing + " " + path; return BSX_ERR_NOMEM;
    } catch (const std::exception &x) {
        g_bsx_err = std::string(doing) + " " + path + ": " + x.what(); return BSX_ERR_IO;
    }
}

struct OutFile {  // an output file that is closed on every way out; finish() closes it and says whether all of it was written
    FILE *f;
    const char *path;
    explicit OutFile(const char *p) : f(fopen(p, "w")), path(p) {}
    OutFile(const OutFile &) = delete;
    OutFile &operator=(const OutFile &) = delete;
    ~OutFile() { if (f) fclose(f); }
    int cannot_write() const { g_bsx_err = std::string("cannot write ") + path; return BSX_ERR_IO; }  // (also the answer to f == nullptr)
    int finish(bool bad = false)
    {
        FILE *const g = f;
        f = nullptr;
        return ((fclose(g) != 0) | bad) ? cannot_write() : BSX_OK;
    }
};

// the whole text to `path`; BSX_ERR_IO when it cannot be written
int meth_write_text(const char *path, const std::string &o)
{
    OutFile out(path);
    if (!out.f) return out.cannot_write();
    return out.finish(fwrite(o.data(), 1, o.size(), out.f) != o.size());
}

struct Mapping {  // a read-only memory map of a whole file, unmapped on every way out
    const char *base = nullptr; size_t len = 0;
    ~Mapping() { if (base) munmap((void *)base, len); }
    int open(const char *path)  // BSX_OK (len == 0 for an empty file) or BSX_ERR_IO
    {
        const int fd = ::open(path, O_RDONLY);
        if (fd < 0) { g_bsx_err = std::string("cannot open ") + path; return BSX_ERR_IO; }
        struct stat st;
        if (fstat(fd, &st) != 0) { ::close(fd); g_bsx_err = std::string("cannot stat ") + path; return BSX_ERR_IO; }
        len = (size_t)st.st_size;
        if (!len) { ::close(fd); return BSX_OK; }
        void *q = mmap(nullptr, len, PROT_READ, MAP_PRIVATE, fd, 0);
        ::close(fd);
        if (q == MAP_FAILED) { len = 0; g_bsx_err = std::string("cannot map ") + path; return BSX_ERR_IO; }
        base = (const char *)q;
        return BSX_OK;
    }
};

// the chromosomes in sorted name order, the order the reference's table has; chr_names: the caller's names in place of the handle's own
std::vector<uint32_t> sorted_chromosomes(const bsx_meth *m, const char *const *chr_names = nullptr)
{
    std::vector<std::string> names;
    for (uint32_t c = 0; c < m->n_chr; c++) names.push_back(chr_names ? std::string(chr_names[c]) : m->names[c]);
    std::vector<uint32_t> o;
    for (uint32_t c = 0; c < m->n_chr; c++) o.push_back(c);
    std::sort(o.begin(), o.end(), [&](uint32_t a, uint32_t b) { return names[a] < names[b]; });
    return o;
}

// `rows` lines formatted by a pool of host threads, each a contiguous range, appended to `f` in order
template <class Fmt>
void format_rows(FILE *f, size_t rows, size_t reserve_per_row, Fmt fmt_row)
{
    const unsigned nt = (unsigned)std::max<size_t>(1, std::min<size_t>(std::min(32u, std::max(1u, bsx_usable_cpus())), rows / 65536 + 1));
    std::vector<std::string> parts(nt);
    auto fmt = [&](unsigned t) {
        std::string &o = parts[t];
        const size_t lo = rows * t / nt, hi = rows * (t + 1) / nt;
        o.reserve((hi - lo) * reserve_per_row);
        for (size_t i = lo; i < hi; i++) fmt_row(i, o);
    };
    std::vector<std::thread> th;
    for (unsigned t = 1; t < nt; t++) th.emplace_back(fmt, t);
    fmt(0);
    for (std::thread &x : th) x.join();
    for (const std::string &o : parts) fwrite(o.data(), 1, o.size(), f);
}

}  // namespace

extern "C" int bsx_meth_write_mbias(bsx_meth *m, const char *path)
{
    if (!m || !path) return BSX_ERR_ARG;
    return guarded(path, "writing", [&]() -> int {
        std::vector<uint64_t> cells(MB_CELLS);
        uint64_t over = 0;
        const int rc = bsx_meth_mbias_fetch(m, cells.data(), &over);
        if (rc) return rc;
        auto cell = [&](int grp, int cyc, int me) { return cells[((size_t)grp * BSX_MBIAS_CYCLES + (size_t)cyc) * 2 + (size_t)me]; };
        int lmax = 0;  // cycles to print: up to the last one with a call in any group
        for (int grp = 0; grp < 16; grp++)
            for (int cyc = lmax; cyc < BSX_MBIAS_CYCLES; cyc++) if (cell(grp, cyc, 0) | cell(grp, cyc, 1)) lmax = cyc + 1;
        static const char *const strands[4] = {"++", "-+", "+-", "--"}, *const contexts[4] = {"CG", "CHG", "CHH", "CN"};
        std::string o = "strand\tcontext\tcycle\tmeth\tdepth\tratio\n";
        char line[160];
        auto ratio = [](uint64_t me, uint64_t d, char *buf, size_t cap) { if (d) snprintf(buf, cap, "%.3f", (double)me / (double)d); else snprintf(buf, cap, "NA"); };
        uint64_t tot[4][2] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}};
        for (int grp = 0; grp < 16; grp++)
            for (int cyc = 0; cyc < BSX_MBIAS_CYCLES; cyc++) {
                const uint64_t me = cell(grp, cyc, 1), d = cell(grp, cyc, 0) + me;
                tot[grp & 3][0] += me; tot[grp & 3][1] += d;
                if (cyc >= lmax) continue;
                char r[32];
                ratio(me, d, r, sizeof(r));
                o.append(line, (size_t)snprintf(line, sizeof(line), "%s\t%s\t%d\t%llu\t%llu\t%s\n", strands[grp >> 2], contexts[grp & 3], cyc + 1, (u64)me, (u64)d, r));
            }
        for (int x = 0; x < 4; x++) {
            char r[32];
            ratio(tot[x][0], tot[x][1], r, sizeof(r));
            o.append(line, (size_t)snprintf(line, sizeof(line), "# total\t%s\t%llu\t%llu\t%s\n", contexts[x], (u64)tot[x][0], (u64)tot[x][1], r));
        }
        o.append(line, (size_t)snprintf(line, sizeof(line), "# calls beyond cycle %d: %llu\n", BSX_MBIAS_CYCLES, (u64)over));
        return meth_write_text(path, o);
    });
}

extern "C" int bsx_meth_combine_cpg(bsx_meth *m)
{
    if (!m) return BSX_ERR_ARG;
    HIP_TRY(hipSetDevice(m->device));
    m->changes = meth_next_stamp();
    hipLaunchKernelGGL(k_meth_cpg, dim3(4096), dim3(256), 0, m->stream, m->dev(), m->d_rev.p, m->d_pdr.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(m->stream));
    return BSX_OK;
}

extern "C" int bsx_meth_valid_mappings(bsx_meth *m, uint64_t *n)
{
    if (!m || !n) return BSX_ERR_ARG;
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipMemcpy(n, m->d_counts.p + CNT_VALID, 8, hipMemcpyDeviceToHost));
    return BSX_OK;
}

// ---- the reports: count, scan, size, emit (the host side of the ordered compaction) ----
// The rows of one report over n_items items, in blocks of 1 024: `count` launches the rule's count kernel over nblk blocks into d_blk[nblk + 1] (the last
// one zeroed here), their exclusive scan d_blk_start ends in the number of rows, `reserve` makes room for that many (not called for none) and `emit`
// launches the rule's emit kernel.  *n_rows and last_rows are 0 on every early way out and the number of rows when the rows are in place.
template <class CountFn, class ReserveFn, class EmitFn>
static int meth_compact(bsx_meth *m, u64 n_items, uint32_t *n_rows, uint32_t &last_rows, CountFn count, ReserveFn reserve, EmitFn emit)
{
    *n_rows = 0; last_rows = 0;
    const size_t nblk = (size_t)((n_items + 1023) / 1024);
    if (!nblk) return BSX_OK;
    HIP_TRY(m->d_blk.reserve((nblk + 1) * 4)); HIP_TRY(m->d_blk_start.reserve((nblk + 1) * 4));
    HIP_TRY(hipMemsetAsync(m->d_blk.p + nblk, 0, 4, m->stream));
    count((unsigned)nblk);
    HIP_TRY(hipGetLastError());
    int rc = meth_scan_u32(m, m->d_blk.p, m->d_blk_start.p, nblk + 1);
    if (rc) return rc;
    uint32_t rows = 0;
    HIP_TRY(hipMemcpyAsync(&rows, m->d_blk_start.p + nblk, 4, hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    if (rows) {
        rc = reserve((size_t)rows);
        if (rc) return rc;
        emit((unsigned)nblk);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(m->stream));
    }
    *n_rows = rows; last_rows = rows;
    return BSX_OK;
}

extern "C" int bsx_meth_report_chr(bsx_meth *m, uint32_t chr, uint32_t min_depth, int meth0, uint32_t *n_rows, uint64_t *n_covered, uint64_t *sum_depth)
{
    if (!m || chr >= m->n_chr || !n_rows) return BSX_ERR_ARG;
    HIP_TRY(hipSetDevice(m->device));
    const u64 g0 = m->chr_off[chr], n = m->chr_off[chr + 1] - g0;
    if (n_covered) *n_covered = 0;
    if (sum_depth) *sum_depth = 0;
    const MethDev M = m->dev();
    const RowRule R{min_depth, m->ctx_mask, meth0, m->snp};
    u64 *const nc_nd = m->d_counts.p + CNT_NC;  // CNT_NC and CNT_ND: k_meth_count adds to them
    *n_rows = 0; m->last_rows = 0;
    HIP_TRY(hipMemsetAsync(nc_nd, 0, 16, m->stream));
    const int rc = meth_compact(m, n, n_rows, m->last_rows,
        [&](unsigned nblk) { hipLaunchKernelGGL(k_meth_count, dim3(nblk), dim3(256), 0, m->stream, M, g0, n, R, m->d_blk.p, nc_nd, m->d_rev.p); },
        [&](size_t rows) -> int {
            for (DevBuf<uint32_t> &b : m->d_out) HIP_TRY(b.reserve(rows * 4));
            if (m->snp) for (DevBuf<uint32_t> &b : m->d_out_rev) HIP_TRY(b.reserve(rows * 4));
            HIP_TRY(m->d_ctx.reserve(rows * 8));
            return BSX_OK;
        },
        [&](unsigned nblk) {
            hipLaunchKernelGGL(k_meth_emit, dim3(nblk), dim3(256), 0, m->stream, M, g0, n, R, m->d_blk_start.p, m->d_out[0].p, m->d_out[1].p, m->d_out[2].p, m->d_ctx.p,
                               m->d_out_rev[0].p, m->d_out_rev[1].p, m->d_rev.p);
        });
    if (rc || !n) return rc;
    u64 cnt[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(cnt, nc_nd, 16, hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    if (n_covered) *n_covered = cnt[0];
    if (sum_depth) *sum_depth = cnt[1];
    return BSX_OK;
}

extern "C" int bsx_meth_fetch_rows(bsx_meth *m, uint32_t *pos, uint32_t *depth, uint32_t *meth)
{
    if (!m || !pos || !depth || !meth) return BSX_ERR_ARG;
    HIP_TRY(hipSetDevice(m->device));
    if (!m->last_rows) return BSX_OK;
    uint32_t *const out[3] = {pos, depth, meth};
    for (int k = 0; k < 3; k++) HIP_TRY(hipMemcpy(out[k], m->d_out[k].p, (size_t)m->last_rows * 4, hipMemcpyDeviceToHost));
    return BSX_OK;
}

extern "C" int bsx_meth_fetch_rows_snp(bsx_meth *m, uint32_t *rev_g, uint32_t *rev_ga)
{
    if (!m || !rev_g || !rev_ga) return BSX_ERR_ARG;
    if (!m->snp) { g_bsx_err = "the C/T-SNP mode is off (bsx_meth_set_ct_snp)"; return BSX_ERR_STATE; }
    HIP_TRY(hipSetDevice(m->device));
    if (!m->last_rows) return BSX_OK;
    HIP_TRY(hipMemcpy(rev_g, m->d_out_rev[0].p, (size_t)m->last_rows * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(rev_ga, m->d_out_rev[1].p, (size_t)m->last_rows * 4, hipMemcpyDeviceToHost));
    return BSX_OK;
}

// ---- per-read calls ----
extern "C" int bsx_meth_set_nonconv(bsx_meth *m, uint32_t n)
{
    if (!m) return BSX_ERR_ARG;
    m->nonconv = n;
    return BSX_OK;
}

extern "C" int bsx_meth_nonconv_dropped(bsx_meth *m, uint64_t *n)
{
    if (!m || !n) return BSX_ERR_ARG;
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipMemcpy(n, m->d_counts.p + CNT_DROPPED, 8, hipMemcpyDeviceToHost));
    return BSX_OK;
}

extern "C" int bsx_meth_set_read_stats(bsx_meth *m, int on)
{
    if (!m) return BSX_ERR_ARG;
    if (m->index_base) { g_bsx_err = "bsx_meth_set_read_stats after alignments have been added"; return BSX_ERR_STATE; }
    HIP_TRY(hipSetDevice(m->device));
    if (!on) m->d_hist.reset();
    else if (!m->d_hist.p) HIP_TRY(m->d_hist.zeroed(RS_CELLS * 8, m->stream));
    return BSX_OK;
}

extern "C" int bsx_meth_read_stats_fetch(bsx_meth *m, uint64_t *cg, uint64_t *ch, uint64_t *totals)
{
    if (!m || !cg || !ch || !totals) return BSX_ERR_ARG;
    if (!m->d_hist.p) { g_bsx_err = "the read histogram is off (bsx_meth_set_read_stats)"; return BSX_ERR_STATE; }
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipMemcpy(cg, m->d_hist.p, (size_t)RS_CG * RS_CG * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(ch, m->d_hist.p + RS_CG * RS_CG, (size_t)RS_CH * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(totals, m->d_hist.p + RS_LDS_CELLS, 4 * 8, hipMemcpyDeviceToHost));
    return BSX_OK;
}

extern "C" int bsx_meth_write_read_stats(bsx_meth *m, const char *path)
{
    if (!m || !path) return BSX_ERR_ARG;
    return guarded(path, "writing", [&]() -> int {
        std::vector<uint64_t> cg((size_t)RS_CG * RS_CG), ch(RS_CH);
        uint64_t tot[4] = {0, 0, 0, 0};
        const int rc = bsx_meth_read_stats_fetch(m, cg.data(), ch.data(), tot);
        if (rc) return rc;
        std::string o = "kind\tcalls\tmeth\treads\n";
        char line[96];
        for (int n = 0; n < RS_CG; n++)
            for (int me = 0; me <= n; me++)
                if (cg[(size_t)n * RS_CG + me]) o.append(line, (size_t)snprintf(line, sizeof(line), "CG\t%d\t%d\t%llu\n", n, me, (u64)cg[(size_t)n * RS_CG + me]));
        o.append(line, (size_t)snprintf(line, sizeof(line), "CG\t>%d\t.\t%llu\n", BSX_RS_CG_MAX, (u64)tot[1]));
        for (int k = 0; k < BSX_RS_CH_MAX; k++) o.append(line, (size_t)snprintf(line, sizeof(line), "CH\t.\t%d\t%llu\n", k, (u64)ch[k]));
        o.append(line, (size_t)snprintf(line, sizeof(line), "CH\t.\t%d+\t%llu\n", BSX_RS_CH_MAX, (u64)ch[BSX_RS_CH_MAX]));
        o.append(line, (size_t)snprintf(line, sizeof(line), "# reads\t%llu\n# CH calls\t%llu\n# CH methylated\t%llu\n", (u64)tot[0], (u64)tot[2], (u64)tot[3]));
        if (tot[2]) o.append(line, (size_t)snprintf(line, sizeof(line), "# CH ratio\t%.5f\n", (double)tot[3] / (double)tot[2]));
        else o += "# CH ratio\tNA\n";
        return meth_write_text(path, o);
    });
}

static const char *const PDR_OFF = "PDR is off (bsx_meth_set_pdr)";

extern "C" int bsx_meth_set_pdr(bsx_meth *m, uint32_t min_cpg)
{
    if (!m) return BSX_ERR_ARG;
    if ((min_cpg != 0) == (m->d_pdr.p != nullptr)) { m->min_cpg = min_cpg; return BSX_OK;}  // another threshold at any time: the cells are the same
    if (m->index_base) { g_bsx_err = "bsx_meth_set_pdr on or off after alignments have been added"; return BSX_ERR_STATE; }
    HIP_TRY(hipSetDevice(m->device));
    if (!min_cpg) m->d_pdr.reset();
    else HIP_TRY(m->d_pdr.zeroed((size_t)(m->chr_off.back() + 16) * 8, m->stream));
    m->min_cpg = min_cpg;
    return BSX_OK;
}

extern "C" int bsx_meth_pdr_report_chr(bsx_meth *m, uint32_t chr, uint32_t min_reads, uint32_t *n_rows)
{
    if (!m || chr >= m->n_chr || !n_rows || !min_reads) return BSX_ERR_ARG;
    if (!m->d_pdr.p) { g_bsx_err = PDR_OFF; return BSX_ERR_STATE; }
    HIP_TRY(hipSetDevice(m->device));
    const u64 g0 = m->chr_off[chr], n = m->chr_off[chr + 1] - g0;
    return meth_compact(m, n, n_rows, m->pdr_last_rows,
        [&](unsigned nblk) { hipLaunchKernelGGL(k_pdr_count, dim3(nblk), dim3(256), 0, m->stream, (const u64 *)m->d_pdr.p, g0, n, min_reads, m->d_blk.p); },
        [&](size_t rows) -> int {
            for (DevBuf<uint32_t> &b : m->d_pdr_out) HIP_TRY(b.reserve(rows * 4));
            HIP_TRY(m->d_pdr_letter.reserve(rows));
            return BSX_OK;
        },
        [&](unsigned nblk) {
            hipLaunchKernelGGL(k_pdr_emit, dim3(nblk), dim3(256), 0, m->stream, (const uint8_t *)m->d_ref.p, (const u64 *)m->d_pdr.p, g0, n, min_reads,
                               (const uint32_t *)m->d_blk_start.p, m->d_pdr_out[0].p, m->d_pdr_out[1].p, m->d_pdr_out[2].p, m->d_pdr_letter.p);
        });
}

extern "C" int bsx_meth_pdr_fetch_rows(bsx_meth *m, uint32_t *pos0, uint32_t *reads, uint32_t *discordant)
{
    if (!m || !pos0 || !reads || !discordant) return BSX_ERR_ARG;
    if (!m->d_pdr.p) { g_bsx_err = PDR_OFF; return BSX_ERR_STATE; }
    HIP_TRY(hipSetDevice(m->device));
    if (!m->pdr_last_rows) return BSX_OK;
    uint32_t *const out[3] = {pos0, reads, discordant};
    for (int k = 0; k < 3; k++) HIP_TRY(hipMemcpy(out[k], m->d_pdr_out[k].p, (size_t)m->pdr_last_rows * 4, hipMemcpyDeviceToHost));
    return BSX_OK;
}

// ---- epiallele patterns ----
static const char *const EPI_OFF = "the epiallele tally is off (bsx_meth_set_epi)";

extern "C" int bsx_meth_set_epi(bsx_meth *m, int on)
{
    if (!m) return BSX_ERR_ARG;
    if ((on != 0) == (m->epi != 0)) return BSX_OK;
    if (m->index_base) { g_bsx_err = "bsx_meth_set_epi on or off after alignments have been added"; return BSX_ERR_STATE; }
    HIP_TRY(hipSetDevice(m->device));
    if (!on) meth_epi_drop_index(m);
    m->epi = on != 0;  // the index and the cells are built by the first call that needs them
    return BSX_OK;
}

extern "C" int bsx_meth_n_cpg(bsx_meth *m, uint32_t chr, uint64_t *n)
{
    if (!m || chr >= m->n_chr || !n) return BSX_ERR_ARG;
    if (!m->epi) { g_bsx_err = EPI_OFF; return BSX_ERR_STATE; }
    HIP_TRY(hipSetDevice(m->device));
    const int rc = meth_epi_index(m);
    if (rc) return rc;
    *n = m->cpg_first[chr + 1] - m->cpg_first[chr];
    return BSX_OK;
}

extern "C" int bsx_meth_epi_report_chr(bsx_meth *m, uint32_t chr, uint32_t min_reads, uint32_t *n_rows)
{
    if (!m || chr >= m->n_chr || !n_rows || !min_reads) return BSX_ERR_ARG;
    if (!m->epi) { g_bsx_err = EPI_OFF; return BSX_ERR_STATE; }
    HIP_TRY(hipSetDevice(m->device));
    const int rc = meth_epi_index(m);
    if (rc) return rc;
    const u64 o0 = m->cpg_first[chr], n_cpg = m->cpg_first[chr + 1] - o0, n = n_cpg >= 4 ? n_cpg - 3 : 0;  // the chromosome's windows
    return meth_compact(m, n, n_rows, m->epi_last_rows,
        [&](unsigned nblk) { hipLaunchKernelGGL(k_epi_count, dim3(nblk), dim3(256), 0, m->stream, (const uint32_t *)m->d_epi.p, o0, n, min_reads, m->d_blk.p); },
        [&](size_t rows) -> int {
            HIP_TRY(m->d_epi_out[0].reserve(rows * 16)); HIP_TRY(m->d_epi_out[1].reserve(rows * 64));
            return BSX_OK;
        },
        [&](unsigned nblk) {
            hipLaunchKernelGGL(k_epi_emit, dim3(nblk), dim3(256), 0, m->stream, (const uint32_t *)m->d_epi.p, (const uint32_t *)m->d_cpg_pos.p, o0, n, min_reads,
                               (const uint32_t *)m->d_blk_start.p, m->d_epi_out[0].p, m->d_epi_out[1].p);
        });
}

extern "C" int bsx_meth_epi_fetch_rows(bsx_meth *m, uint32_t *pos0, uint32_t *counts)
{
    if (!m || !pos0 || !counts) return BSX_ERR_ARG;
    if (!m->epi) { g_bsx_err = EPI_OFF; return BSX_ERR_STATE; }
    HIP_TRY(hipSetDevice(m->device));
    if (!m->epi_last_rows) return BSX_OK;
    HIP_TRY(hipMemcpy(pos0, m->d_epi_out[0].p, (size_t)m->epi_last_rows * 16, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(counts, m->d_epi_out[1].p, (size_t)m->epi_last_rows * 64, hipMemcpyDeviceToHost));
    return BSX_OK;
}

// ---- host side for whole files: the reference's per-line Python is the slow part of the tool once the pile-up is on the GPU ----
// The parsers (BSP / SAM lines, BAM records, FASTA, BED) are plain C++ in bsx_meth_parse.h and the row formatters in bsx_meth_text.h and bsx_meth_epi.h,
// where the host sanitizers reach them.
using bsx_meth_parse::ParsedChunk;

extern "C" int bsx_meth_add_file(bsx_meth *m, const char *path, int sam, const char *const *chr_names, int unique, int pair, uint32_t trim_fillin, uint64_t *n_lines)
{
    if (!m || !path || (!chr_names && m->names.size() != m->n_chr)) return BSX_ERR_ARG;
    return guarded(path, "reading", [&]() -> int {
        Mapping map;
        if (n_lines) *n_lines = 0;
        const int rc_open = map.open(path);
        if (rc_open != BSX_OK || !map.len) return rc_open;
        std::unordered_map<std::string, uint32_t> cid;
        for (uint32_t c = 0; c < m->n_chr; c++) cid.emplace(chr_names ? std::string(chr_names[c]) : m->names[c], c);
        u64 lines = 0;
        int rc_add = BSX_OK;
        auto add = [&](ParsedChunk &pc) {  // alignments keep the file's order
            if (pc.chr.size() > 0xffffffffull) { rc_add = BSX_ERR_LIMIT; return 1; }
            pc.seq.push_back(0);
            rc_add = bsx_meth_add(m, (uint32_t)pc.chr.size(), pc.chr.data(), pc.pos.data(), pc.strand.data(), pc.insert.data(), pc.cut.data(), pc.seq.data(),
                                  (const uint64_t *)pc.off.data(), trim_fillin);
            return rc_add != BSX_OK ? 1 : 0;
        };
        if (sam == 2) {  // BAM, a window of inflated blocks at a time (BSX_BAM_WINDOW bytes, default 256 MB)
            int bad = 0;
            const size_t window = getenv("BSX_BAM_WINDOW") ? (size_t)std::max(1ll, atoll(getenv("BSX_BAM_WINDOW"))) : ((size_t)256 << 20);
            const int rcs = bsx_meth_parse::stream_bam(map.base, map.len, cid, unique, pair, window, lines, bad, add);
            if (n_lines) *n_lines = lines;
            if (rc_add != BSX_OK) return rc_add;
            if (rcs) { g_bsx_err = std::string("not a readable BAM file: ") + path; return BSX_ERR_IO; }
            if (bad == 2) { g_bsx_err = "alignment record without strand information"; return BSX_ERR_ARG; }
            return BSX_OK;
        }
        // pieces of ~256 MB (bounded host memory), each cut into per-thread chunks at line starts
        const int rcs = bsx_meth_parse::stream_text(map.base, map.len, sam, cid, unique, pair, (size_t)256 << 20, lines, add);
        if (n_lines) *n_lines = lines;
        if (rc_add != BSX_OK) return rc_add;
        if (rcs == 2) { g_bsx_err = "alignment line without strand information"; return BSX_ERR_ARG; }
        return rcs ? BSX_ERR_IO : BSX_OK;
    });
}

// the table of methratio.py:130-151 for the chromosomes in `order` (the reference sorts the names), same arithmetic and formats
static int write_table(bsx_meth *m, const char *path, uint32_t n_order, const uint32_t *order, const char *const *chr_names, uint32_t min_depth, int meth0,
                       uint64_t *n_covered, uint64_t *sum_depth)
{
    std::vector<uint32_t> sorted_order;
    if (!order) { sorted_order = sorted_chromosomes(m, chr_names); order = sorted_order.data(); n_order = m->n_chr; }
    OutFile out(path);
    if (!out.f) return out.cannot_write();
    const bool snp = m->snp != 0;  // C/T-SNP mode: the 12-column table of later BSMAP releases
    fputs(snp ? "chr\tpos\tstrand\tcontext\tratio\teff_CT_count\tC_count\tCT_count\trev_G_count\trev_GA_count\tCI_lower\tCI_upper\n"
              : "chr\tpos\tstrand\tcontext\tratio\ttotal_C\tmethy_C\tCI_lower\tCI_upper\n", out.f);
    u64 nc = 0, nd = 0;
    int rc = BSX_OK;
    std::vector<uint32_t> pos, dep, met, rvg, rvga; std::vector<u64> ctx;
    for (uint32_t k = 0; k < n_order && rc == BSX_OK; k++) {
        const uint32_t c = order[k];
        if (c >= m->n_chr) { rc = BSX_ERR_ARG; break; }
        uint32_t rows = 0; uint64_t cov = 0, sd_ = 0;
        rc = bsx_meth_report_chr(m, c, min_depth, meth0, &rows, &cov, &sd_);
        if (rc) break;
        nc += cov; nd += sd_;
        if (!rows) continue;
        pos.resize(rows); dep.resize(rows); met.resize(rows); ctx.resize(rows);
        rc = bsx_meth_fetch_rows(m, pos.data(), dep.data(), met.data());
        if (rc) break;
        if (snp) {
            rvg.resize(rows); rvga.resize(rows);
            rc = bsx_meth_fetch_rows_snp(m, rvg.data(), rvga.data());
            if (rc) break;
        }
        if (hipMemcpy(ctx.data(), m->d_ctx.p, (size_t)rows * 8, hipMemcpyDeviceToHost) != hipSuccess) { rc = BSX_ERR_DEVICE; break; }
        const char *name = chr_names ? chr_names[c] : m->names[c].c_str();
        format_rows(out.f, rows, snp ? 72 : 56, [&](size_t i, std::string &o) { bsx_meth_text::append_table_row(o, name, pos[i], dep[i], met[i], ctx[i], snp, snp ? rvg[i] : 0u, snp ? rvga[i] : 0u); });
    }
    if (rc == BSX_OK) rc = out.finish();
    if (n_covered) *n_covered = nc;
    if (sum_depth) *sum_depth = nd;
    return rc;
}

extern "C" int bsx_meth_write_table(bsx_meth *m, const char *path, uint32_t n_order, const uint32_t *order, const char *const *chr_names, uint32_t min_depth, int meth0,
                                    uint64_t *n_covered, uint64_t *sum_depth)
{
    if (!m || !path || (!chr_names && m->names.size() != m->n_chr)) return BSX_ERR_ARG;
    return guarded(path, "writing", [&] { return write_table(m, path, n_order, order, chr_names, min_depth, meth0, n_covered, sum_depth); });
}

// the reference FASTA through bsx_meth_parse::parse_fasta (methratio.py:67-77); `chroms_csv` is the -c filter
extern "C" int bsx_meth_create_from_fasta(const char *path, const char *chroms_csv, int rm_dup, int device, bsx_meth **out)
{
    if (!path || !out) return BSX_ERR_ARG;
    std::vector<std::string> names;
    std::vector<std::vector<char>> seqs;
    const int rc_parse = guarded(path, "reading", [&]() -> int {
        Mapping map;
        const int rc_open = map.open(path);
        if (rc_open != BSX_OK) return rc_open;
        if (!map.len) return BSX_ERR_IO;
        if (bsx_meth_parse::parse_fasta(map.base, map.len, chroms_csv, names, seqs)) { g_bsx_err = "no sequence selected from the reference file"; return BSX_ERR_ARG; }
        return BSX_OK;
    });
    if (rc_parse) return rc_parse;
    std::vector<uint64_t> lens;
    for (const std::vector<char> &q : seqs) lens.push_back(q.size());
    bsx_meth *m = nullptr;
    int rc = bsx_meth_create((uint32_t)names.size(), lens.data(), rm_dup, device, &m);
    if (rc) return rc;
    for (size_t i = 0; i < names.size() && rc == BSX_OK; i++) {
        m->names.push_back(names[i]);
        if (!seqs[i].empty() && hipMemcpy(m->d_ref.p + m->chr_off[i], seqs[i].data(), seqs[i].size(), hipMemcpyHostToDevice) != hipSuccess) rc = BSX_ERR_DEVICE;
        std::vector<char>().swap(seqs[i]);
    }
    if (rc) { bsx_meth_destroy(m); return rc; }
    *out = m;
    return BSX_OK;
}

extern "C" uint32_t bsx_meth_n_chr(const bsx_meth *m) { return m ? m->n_chr : 0; }
extern "C" const char *bsx_meth_chr_name(const bsx_meth *m, uint32_t c) { return (m && c < m->names.size()) ? m->names[c].c_str() : ""; }

// ---- pooled methylation per interval and per bin ----
static constexpr size_t REGION_CHUNK = (size_t)1 << 22;  // a launch takes intervals until it holds this many of them or of their tiles

extern "C" uint32_t bsx_meth_region_tile(void) { return bsx_meth_tiles::TILE; }

// The host side of every interval kernel: clip, cut into launches and tiles, zero the sums, launch, copy back.  `launch(wide, tiles, n_tiles, iv_chr,
// iv_start, sums)` starts the kernel on m's stream: with blocks of 16 waves where `wide` says that the launch is mostly long intervals, of 4 otherwise.
template <class Launch>
static int meth_tiled(bsx_meth *m, uint32_t n, const uint32_t *chr, const uint32_t *start, const uint32_t *end, uint64_t *sums, Launch launch)
{
    std::vector<uint32_t> cs(n), ce(n);  // the clipped intervals
    for (uint32_t i = 0; i < n; i++) {
        if (chr[i] >= m->n_chr || start[i] > end[i]) return BSX_ERR_ARG;
        const u64 clen = m->chr_off[chr[i] + 1] - m->chr_off[chr[i]];
        ce[i] = (uint32_t)std::min<u64>(end[i], clen);
        cs[i] = std::min(start[i], ce[i]);
    }
    HIP_TRY(hipSetDevice(m->device));
    // launches: [a, b) of the intervals each
    const auto clipped_len = [&](uint32_t i) { return ce[i] - cs[i]; };
    const std::vector<uint32_t> cut_at = bsx_meth_tiles::launches(n, clipped_len, REGION_CHUNK);
    size_t max_iv = 0, max_tiles = 0;
    for (size_t q = 0; q + 1 < cut_at.size(); q++) {
        size_t nt = 0;
        for (uint32_t i = cut_at[q]; i < cut_at[q + 1]; i++) nt += (size_t)bsx_meth_tiles::n_tiles(clipped_len(i));
        max_iv = std::max<size_t>(max_iv, cut_at[q + 1] - cut_at[q]); max_tiles = std::max(max_tiles, nt);
    }
    DevBuf<bsx_meth_tiles::Tile> d_tiles;
    DevBuf<uint32_t> d_chr, d_start;
    DevBuf<u64> d_sums;
    if (d_tiles.reserve(max_tiles * sizeof(bsx_meth_tiles::Tile)) != hipSuccess || d_chr.reserve(max_iv * 4) != hipSuccess || d_start.reserve(max_iv * 4) != hipSuccess ||
        d_sums.reserve(max_iv * 40) != hipSuccess) {
        g_bsx_err = "bsx_meth_regions: no device memory for the intervals"; return BSX_ERR_NOMEM;
    }
    std::vector<bsx_meth_tiles::Tile> tiles;
    for (size_t q = 0; q + 1 < cut_at.size(); q++) {
        const uint32_t a = cut_at[q], b = cut_at[q + 1];
        tiles.clear();
        for (uint32_t i = a; i < b; i++) bsx_meth_tiles::cut(i - a, ce[i] - cs[i], tiles);
        HIP_TRY(hipMemsetAsync(d_sums.p, 0, (size_t)(b - a) * 40, m->stream));
        if (!tiles.empty()) {
            HIP_TRY(hipMemcpyAsync(d_tiles.p, tiles.data(), tiles.size() * sizeof(bsx_meth_tiles::Tile), hipMemcpyHostToDevice, m->stream));
            HIP_TRY(hipMemcpyAsync(d_chr.p, chr + a, (size_t)(b - a) * 4, hipMemcpyHostToDevice, m->stream));
            HIP_TRY(hipMemcpyAsync(d_start.p, cs.data() + a, (size_t)(b - a) * 4, hipMemcpyHostToDevice, m->stream));
            const uint32_t nt = (uint32_t)tiles.size();
            launch(bsx_meth_tiles::wide(a, b, clipped_len), (const bsx_meth_tiles::Tile *)d_tiles.p, nt, (const uint32_t *)d_chr.p, (const uint32_t *)d_start.p, d_sums.p);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipMemcpyAsync(sums + (size_t)a * 5, d_sums.p, (size_t)(b - a) * 40, hipMemcpyDeviceToHost, m->stream));
        HIP_TRY(hipStreamSynchronize(m->stream));  // (the host vectors are reused by the next launch)
    }
    return BSX_OK;
}

static int meth_regions(bsx_meth *m, uint32_t n, const uint32_t *chr, const uint32_t *start, const uint32_t *end, uint32_t min_depth, uint64_t *sums)
{
    const MethDev M = m->dev();
    const RowRule R{min_depth, m->ctx_mask, 1, m->snp};
    return meth_tiled(m, n, chr, start, end, sums, [&](bool wide, const bsx_meth_tiles::Tile *tiles, uint32_t nt, const uint32_t *iv_chr, const uint32_t *iv_start, u64 *d_sums) {
        const unsigned waves = wide ? 16 : 4;
        auto kernel = m->snp ? (wide ? k_meth_regions<true, 16> : k_meth_regions<true, 4>) : (wide ? k_meth_regions<false, 16> : k_meth_regions<false, 4>);
        hipLaunchKernelGGL(kernel, dim3((nt + waves - 1) / waves), dim3(waves * 64), 0, m->stream, M, R, (const u64 *)m->d_rev.p, tiles, nt, iv_chr, iv_start, d_sums);
    });
}

extern "C" int bsx_meth_regions(bsx_meth *m, uint32_t n, const uint32_t *chr, const uint32_t *start, const uint32_t *end, uint32_t min_depth, uint64_t *sums)
{
    if (!m || (n && (!chr || !start || !end || !sums))) return BSX_ERR_ARG;
    if (!n) return BSX_OK;
    try {
        return meth_regions(m, n, chr, start, end, min_depth, sums);
    } catch (const std::bad_alloc &) {
        g_bsx_err = "bsx_meth_regions: out of host memory"; return BSX_ERR_NOMEM;
    }
}

extern "C" int bsx_meth_bins(bsx_meth *m, uint32_t chr, uint32_t bin, uint32_t min_depth, uint64_t n_bins_cap, uint64_t *sums, uint64_t *n_bins)
{
    if (!m || !n_bins || chr >= m->n_chr || !bin) return BSX_ERR_ARG;
    const u64 g0 = m->chr_off[chr], n = m->chr_off[chr + 1] - g0, need = n / bin + 1;
    *n_bins = need;
    if (!sums || n_bins_cap < need) return BSX_ERR_ARG;
    HIP_TRY(hipSetDevice(m->device));
    DevBuf<u64> d_bins;
    if (d_bins.reserve((size_t)need * 40) != hipSuccess) { g_bsx_err = "bsx_meth_bins: no device memory for the bins"; return BSX_ERR_NOMEM; }
    HIP_TRY(hipMemsetAsync(d_bins.p, 0, (size_t)need * 40, m->stream));
    if (n) {
        // positions per block: 1 024 below B = 16 (the block's bin table is LDS), 4 096 from there on (fewer adds on the cells that wide bins share)
        const uint32_t rounds = bin < 16 ? 4 : 16;
        const u64 P = (u64)rounds * 256;
        const size_t lds = (size_t)std::min<u64>(P, (P - 1) / bin + 2) * 40;
        const MethDev M = m->dev();
        const RowRule R{min_depth, m->ctx_mask, 1, m->snp};
        if (m->snp) hipLaunchKernelGGL(k_meth_bins<true>, dim3((unsigned)((n + P - 1) / P)), dim3(256), lds, m->stream, M, g0, n, R, m->d_rev.p, bin, rounds, d_bins.p);
        else hipLaunchKernelGGL(k_meth_bins<false>, dim3((unsigned)((n + P - 1) / P)), dim3(256), lds, m->stream, M, g0, n, R, m->d_rev.p, bin, rounds, d_bins.p);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemcpyAsync(sums, d_bins.p, (size_t)need * 40, hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    return BSX_OK;
}

namespace {

int write_wig(bsx_meth *m, const char *path, uint32_t bin, uint32_t min_depth)
{
    OutFile out(path);
    if (!out.f) return out.cannot_write();
    fputs("track type=wiggle_0\n", out.f);
    std::vector<uint64_t> sums;
    for (const uint32_t c : sorted_chromosomes(m)) {
        fprintf(out.f, "variableStep chrom=%s span=%u\n", m->names[c].c_str(), bin);
        const u64 need = (m->chr_off[c + 1] - m->chr_off[c]) / bin + 1;
        sums.resize((size_t)need * 5);
        uint64_t nb = 0;
        const int rc = bsx_meth_bins(m, c, bin, min_depth, need, sums.data(), &nb);
        if (rc) return rc;
        format_rows(out.f, (size_t)nb, 8, [&](size_t j, std::string &o) { bsx_meth_text::append_wig_line(o, j, bin, &sums[j * 5]); });
    }
    return out.finish();
}

// the records of a BED file on the handle's sequences, under the rules of bsx_meth_write_regions
int read_bed(bsx_meth *m, const char *bed_path, bsx_meth_parse::BedRecords &bed)
{
    Mapping map;
    const int rc_open = map.open(bed_path);
    if (rc_open != BSX_OK) return rc_open;
    std::unordered_map<std::string, uint32_t> cid;
    std::vector<bsx_meth_parse::u64> lens;
    for (uint32_t c = 0; c < m->n_chr; c++) { cid.emplace(m->names[c], c); lens.push_back(m->chr_off[c + 1] - m->chr_off[c]); }
    const u64 bad = map.len ? bsx_meth_parse::parse_bed(map.base, map.len, cid, lens, bed) : 0;
    if (bad) { g_bsx_err = std::string(bed_path) + ": line " + std::to_string(bad) + ": not a BED record (name, start <= end as numbers)"; return BSX_ERR_IO; }
    if (bed.chr.size() > 0xffffffffull) { g_bsx_err = std::string(bed_path) + ": more than 2^32 - 1 records"; return BSX_ERR_LIMIT; }
    return BSX_OK;
}

int write_regions(bsx_meth *m, const char *bed_path, const char *out_path, uint32_t min_depth, uint64_t *n_written, uint64_t *n_dropped)
{
    bsx_meth_parse::BedRecords bed;
    const int rc_bed = read_bed(m, bed_path, bed);
    if (rc_bed) return rc_bed;
    const size_t n = bed.chr.size();
    std::vector<uint64_t> sums(n * 5 + 1);
    const int rc = bsx_meth_regions(m, (uint32_t)n, bed.chr.data(), bed.start.data(), bed.end.data(), min_depth, sums.data());
    if (rc) return rc;
    OutFile out(out_path);
    if (!out.f) return out.cannot_write();
    fputs("chr\tstart\tend\tname\tn_C\tmethy_C\ttotal_C\teff_CT\tratio\tCI_lower\tCI_upper\n", out.f);
    format_rows(out.f, n, 64, [&](size_t i, std::string &o) {
        bsx_meth_text::append_region_row(o, m->names[bed.chr[i]].c_str(), bed.start[i], bed.end[i], bed.label[i], &sums[i * 5]);
    });
    const int rc_close = out.finish();
    if (rc_close) return rc_close;
    if (n_written) *n_written = n;
    if (n_dropped) *n_dropped = bed.dropped;
    return BSX_OK;
}

int write_pdr(bsx_meth *m, const char *path, uint32_t min_reads, uint64_t *n_rows)
{
    OutFile out(path);
    if (!out.f) return out.cannot_write();
    fputs("chr\tpos\tstrand\treads\tdiscordant\tPDR\n", out.f);
    std::vector<uint32_t> pos, reads, disc;
    std::vector<uint8_t> letter;
    uint64_t total = 0;
    for (const uint32_t c : sorted_chromosomes(m)) {
        uint32_t rows = 0;
        int rc = bsx_meth_pdr_report_chr(m, c, min_reads, &rows);
        if (rc) return rc;
        if (!rows) continue;
        pos.resize(rows); reads.resize(rows); disc.resize(rows); letter.resize(rows);
        rc = bsx_meth_pdr_fetch_rows(m, pos.data(), reads.data(), disc.data());
        if (rc) return rc;
        if (hipMemcpy(letter.data(), m->d_pdr_letter.p, rows, hipMemcpyDeviceToHost) != hipSuccess) return BSX_ERR_DEVICE;
        const char *name = m->names[c].c_str();
        format_rows(out.f, rows, 40, [&](size_t i, std::string &o) { bsx_meth_text::append_pdr_row(o, name, pos[i], letter[i], reads[i], disc[i]); });
        total += rows;
    }
    const int rc_close = out.finish();
    if (rc_close) return rc_close;
    if (n_rows) *n_rows = total;
    return BSX_OK;
}

int write_epi(bsx_meth *m, const char *path, uint32_t min_reads, uint64_t *n_rows)
{
    OutFile out(path);
    if (!out.f) return out.cannot_write();
    fputs(bsx_meth_epi::header().c_str(), out.f);
    std::vector<uint32_t> pos, counts;
    uint64_t total = 0;
    for (const uint32_t c : sorted_chromosomes(m)) {
        uint32_t rows = 0;
        int rc = bsx_meth_epi_report_chr(m, c, min_reads, &rows);
        if (rc) return rc;
        if (!rows) continue;
        pos.resize((size_t)rows * 4); counts.resize((size_t)rows * 16);
        rc = bsx_meth_epi_fetch_rows(m, pos.data(), counts.data());
        if (rc) return rc;
        const char *name = m->names[c].c_str();
        format_rows(out.f, rows, 128, [&](size_t i, std::string &o) { bsx_meth_epi::append_row(o, name, &pos[i * 4], &counts[i * 16]); });
        total += rows;
    }
    const int rc_close = out.finish();
    if (rc_close) return rc_close;
    if (n_rows) *n_rows = total;
    return BSX_OK;
}

}  // namespace

extern "C" int bsx_meth_write_epi(bsx_meth *m, const char *path, uint32_t min_reads, uint64_t *n_rows)
{
    if (!m || !path || !min_reads || m->names.size() != m->n_chr) return BSX_ERR_ARG;
    if (n_rows) *n_rows = 0;
    if (!m->epi) { g_bsx_err = EPI_OFF; return BSX_ERR_STATE; }
    return guarded(path, "writing", [&] { return write_epi(m, path, min_reads, n_rows); });
}

extern "C" int bsx_meth_write_pdr(bsx_meth *m, const char *path, uint32_t min_reads, uint64_t *n_rows)
{
    if (!m || !path || !min_reads || m->names.size() != m->n_chr) return BSX_ERR_ARG;
    if (n_rows) *n_rows = 0;
    if (!m->d_pdr.p) { g_bsx_err = PDR_OFF; return BSX_ERR_STATE; }
    return guarded(path, "writing", [&] { return write_pdr(m, path, min_reads, n_rows); });
}

extern "C" int bsx_meth_write_wig(bsx_meth *m, const char *path, uint32_t bin, uint32_t min_depth)
{
    if (!m || !path || !bin || m->names.size() != m->n_chr) return BSX_ERR_ARG;
    return guarded(path, "writing", [&] { return write_wig(m, path, bin, min_depth); });
}

extern "C" int bsx_meth_write_regions(bsx_meth *m, const char *bed_path, const char *out_path, uint32_t min_depth, uint64_t *n_written, uint64_t *n_dropped)
{
    if (!m || !bed_path || !out_path || m->names.size() != m->n_chr) return BSX_ERR_ARG;
    if (n_written) *n_written = 0;
    if (n_dropped) *n_dropped = 0;
    return guarded(out_path, "writing", [&] { return write_regions(m, bed_path, out_path, min_depth, n_written, n_dropped); });
}

// ---- two samples: differential methylation ----
// What every diff call checks first: two handles on one device over sequences of the same lengths, the C/T-SNP mode off in both, one context mask.  On
// BSX_OK the device is current and B's stream has been waited for: the kernels run on A's stream and read B's counters.
static int diff_pair(bsx_meth *a, bsx_meth *b)
{
    if (!a || !b || a->device != b->device || a->n_chr != b->n_chr || a->chr_off != b->chr_off) return BSX_ERR_ARG;
    if (a->snp || b->snp) { g_bsx_err = "a diff call needs the C/T-SNP mode off in both handles (bsx_meth_set_ct_snp)"; return BSX_ERR_STATE; }
    if (a->ctx_mask != b->ctx_mask) return BSX_ERR_ARG;
    HIP_TRY(hipSetDevice(a->device));
    if (b != a) HIP_TRY(hipStreamSynchronize(b->stream));
    return BSX_OK;
}

// B's counters under A's letters and offsets
static MethDev diff_dev_b(const bsx_meth *a, const bsx_meth *b)
{
    MethDev B = a->dev();
    B.depth = b->d_depth.p; B.meth = b->d_meth.p; B.first = nullptr;
    return B;
}

// p[n] of n rows or interval sums that lie on the device (k_meth_fisher), on m's stream
static void diff_fisher(bsx_meth *m, const uint4 *rows4, const u64 *sums5, size_t n, double *d_p)
{
    hipLaunchKernelGGL(k_meth_fisher, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, m->stream, rows4, sums5, (u64)n, d_p);
}

extern "C" int bsx_meth_diff_report_chr(bsx_meth *a, bsx_meth *b, uint32_t chr, uint32_t min_depth, uint32_t min_delta_permille, uint32_t *n_rows)
{
    if (!a || !b || !n_rows || chr >= a->n_chr || min_delta_permille > 1000) return BSX_ERR_ARG;
    const int rc_pair = diff_pair(a, b);
    if (rc_pair) return rc_pair;
    const u64 g0 = a->chr_off[chr], n = a->chr_off[chr + 1] - g0;
    const MethDev A = a->dev(), B = diff_dev_b(a, b);
    const RowRule R{min_depth, a->ctx_mask, 1, 0};
    size_t n_out = 0;
    return meth_compact(a, n, n_rows, a->diff_last_rows,
        [&](unsigned nblk) { hipLaunchKernelGGL(k_diff_count, dim3(nblk), dim3(256), 0, a->stream, A, B, g0, n, R, min_delta_permille, a->d_blk.p); },
        [&](size_t rows) -> int {
            HIP_TRY(a->d_diff_pos.reserve(rows * 4)); HIP_TRY(a->d_diff_counts.reserve(rows * 16)); HIP_TRY(a->d_diff_cls.reserve(rows)); HIP_TRY(a->d_diff_p.reserve(rows * 8));
            n_out = rows;
            return BSX_OK;
        },
        [&](unsigned nblk) {  // the rows, then on the same stream p of every row
            hipLaunchKernelGGL(k_diff_emit, dim3(nblk), dim3(256), 0, a->stream, A, B, g0, n, R, min_delta_permille, (const uint32_t *)a->d_blk_start.p, a->d_diff_pos.p,
                               a->d_diff_counts.p, a->d_diff_cls.p);
            diff_fisher(a, a->d_diff_counts.p, nullptr, n_out, a->d_diff_p.p);
        });
}

extern "C" int bsx_meth_diff_fetch_rows(bsx_meth *a, uint32_t *pos0, uint32_t *counts, double *p)
{
    if (!a || !pos0 || !counts || !p) return BSX_ERR_ARG;
    HIP_TRY(hipSetDevice(a->device));
    const size_t rows = a->diff_last_rows;
    if (!rows) return BSX_OK;
    HIP_TRY(hipMemcpy(pos0, a->d_diff_pos.p, rows * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(counts, a->d_diff_counts.p, rows * 16, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(p, a->d_diff_p.p, rows * 8, hipMemcpyDeviceToHost));
    return BSX_OK;
}

// sums[n][5] and p[n] of n intervals; the sums come back through meth_tiled, p is computed from them on the device in pieces of REGION_CHUNK
static int diff_regions(bsx_meth *a, bsx_meth *b, uint32_t n, const uint32_t *chr, const uint32_t *start, const uint32_t *end, uint32_t min_depth, uint64_t *sums, double *p)
{
    const MethDev A = a->dev(), B = diff_dev_b(a, b);
    const RowRule R{min_depth, a->ctx_mask, 1, 0};
    const int rc = meth_tiled(a, n, chr, start, end, sums, [&](bool wide, const bsx_meth_tiles::Tile *tiles, uint32_t nt, const uint32_t *iv_chr, const uint32_t *iv_start, u64 *d_sums) {
        if (wide) hipLaunchKernelGGL(k_meth_diff_regions<16>, dim3((nt + 15) / 16), dim3(1024), 0, a->stream, A, B, R, tiles, nt, iv_chr, iv_start, d_sums);
        else hipLaunchKernelGGL(k_meth_diff_regions<4>, dim3((nt + 3) / 4), dim3(256), 0, a->stream, A, B, R, tiles, nt, iv_chr, iv_start, d_sums);
    });
    if (rc) return rc;
    DevBuf<u64> d_sums;
    DevBuf<double> d_p;
    const size_t piece = std::min<size_t>(n, REGION_CHUNK);
    if (d_sums.reserve(piece * 40) != hipSuccess || d_p.reserve(piece * 8) != hipSuccess) { g_bsx_err = "bsx_meth_diff_regions: no device memory for the intervals"; return BSX_ERR_NOMEM; }
    for (size_t lo = 0; lo < n; lo += piece) {
        const size_t k = std::min(piece, (size_t)n - lo);
        HIP_TRY(hipMemcpyAsync(d_sums.p, sums + lo * 5, k * 40, hipMemcpyHostToDevice, a->stream));
        diff_fisher(a, nullptr, d_sums.p, k, d_p.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(p + lo, d_p.p, k * 8, hipMemcpyDeviceToHost, a->stream));
        HIP_TRY(hipStreamSynchronize(a->stream));
    }
    return BSX_OK;
}

extern "C" int bsx_meth_diff_regions(bsx_meth *a, bsx_meth *b, uint32_t n, const uint32_t *chr, const uint32_t *start, const uint32_t *end, uint32_t min_depth, uint64_t *sums,
                                     double *p)
{
    if (!a || !b || (n && (!chr || !start || !end || !sums || !p))) return BSX_ERR_ARG;
    const int rc_pair = diff_pair(a, b);
    if (rc_pair || !n) return rc_pair;
    try {
        return diff_regions(a, b, n, chr, start, end, min_depth, sums, p);
    } catch (const std::bad_alloc &) {
        g_bsx_err = "bsx_meth_diff_regions: out of host memory"; return BSX_ERR_NOMEM;
    }
}

// ---- q-values over all rows and de novo DMRs ----
static constexpr u64 BH_MAX_ROWS = 0xFFFFFFFFull;  // row indices are 32 bits wide

// q[n] of p[n], both on the device, on `stream`: keys and row indices, one radix sort of the pairs, r back to front, its running minimum, the scatter.
// The workspace (24 bytes a row and the sort's own) lives for the call.  n < 2^32.
static int meth_bh(hipStream_t stream, const double *d_p, size_t n, double *d_q)
{
    if (!n) return BSX_OK;
    DevBuf<u64> d_keys, d_skeys, d_nan;
    DevBuf<uint32_t> d_idx, d_sidx;
    DevBuf<char> d_temp;
    const auto no_memory = [] { g_bsx_err = "no device memory for the q-values' sort"; return BSX_ERR_NOMEM; };
    if (d_keys.reserve(n * 8) != hipSuccess || d_skeys.reserve(n * 8) != hipSuccess || d_idx.reserve(n * 4) != hipSuccess || d_sidx.reserve(n * 4) != hipSuccess ||
        d_nan.reserve(8) != hipSuccess)
        return no_memory();
    const unsigned grid = (unsigned)((n + 255) / 256);
    HIP_TRY(hipMemsetAsync(d_nan.p, 0, 8, stream));
    hipLaunchKernelGGL(k_bh_keys, dim3(grid), dim3(256), 0, stream, d_p, (u64)n, d_keys.p, d_idx.p, d_nan.p);
    HIP_TRY(hipGetLastError());
    size_t need_sort = 0, need_scan = 0;
    double *const d_r = (double *)d_keys.p;  // the unsorted keys are done with after the sort: r and its running minimum take their place
    HIP_TRY(rocprim::radix_sort_pairs(nullptr, need_sort, d_keys.p, d_skeys.p, d_idx.p, d_sidx.p, n, 0u, 64u, stream));
    HIP_TRY(rocprim::inclusive_scan(nullptr, need_scan, d_r, d_r, n, MinDouble(), stream));
    if (d_temp.reserve(std::max(need_sort, need_scan)) != hipSuccess) return no_memory();
    HIP_TRY(rocprim::radix_sort_pairs(d_temp.p, need_sort, d_keys.p, d_skeys.p, d_idx.p, d_sidx.p, n, 0u, 64u, stream));
    hipLaunchKernelGGL(k_bh_ratio, dim3(grid), dim3(256), 0, stream, (const u64 *)d_skeys.p, (u64)n, (const u64 *)d_nan.p, d_r);
    HIP_TRY(hipGetLastError());
    HIP_TRY(rocprim::inclusive_scan(d_temp.p, need_scan, d_r, d_r, n, MinDouble(), stream));
    hipLaunchKernelGGL(k_bh_scatter, dim3(grid), dim3(256), 0, stream, (const double *)d_r, (const uint32_t *)d_sidx.p, (u64)n, (const u64 *)d_nan.p, d_q);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream));  // ahead of the workspace's release
    return BSX_OK;
}

extern "C" int bsx_meth_bh(int device, const double *p, uint64_t n, double *q)
{
    if (n && (!p || !q)) return BSX_ERR_ARG;
    if (!n) return BSX_OK;
    if (n > BH_MAX_ROWS) { g_bsx_err = "bsx_meth_bh takes fewer than 2^32 values"; return BSX_ERR_LIMIT; }
    for (uint64_t i = 0; i < n; i++)
        if (!(p[i] >= 0.0 && p[i] <= 1.0) && p[i] == p[i]) { g_bsx_err = "bsx_meth_bh: a p-value outside 0 .. 1"; return BSX_ERR_ARG; }
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || nd <= 0) { g_bsx_err = "no HIP device visible; libbsx has no CPU fallback"; return BSX_ERR_NODEVICE; }
    if (device < 0 || device >= nd) return BSX_ERR_NODEVICE;
    HIP_TRY(hipSetDevice(device));
    DevBuf<double> d_p, d_q;
    if (d_p.reserve(n * 8) != hipSuccess || d_q.reserve(n * 8) != hipSuccess) { g_bsx_err = "bsx_meth_bh: no device memory for the values"; return BSX_ERR_NOMEM; }
    HIP_TRY(hipMemcpy(d_p.p, p, n * 8, hipMemcpyHostToDevice));
    const int rc = meth_bh((hipStream_t)0, d_p.p, (size_t)n, d_q.p);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(q, d_q.p, n * 8, hipMemcpyDeviceToHost));
    return BSX_OK;
}

// the writer's sequence order: sorted names, or the ids' own order for a handle without names
static std::vector<uint32_t> diff_order(const bsx_meth *a)
{
    if (a->names.size() == a->n_chr) return sorted_chromosomes(a);
    std::vector<uint32_t> o(a->n_chr);
    for (uint32_t c = 0; c < a->n_chr; c++) o[c] = c;
    return o;
}

// Fills the store.  The blocks of all sequences stand behind one another in d_blk, in the writer's order: one count launch per sequence, ONE scan over all
// blocks, whose results are row numbers of the whole store, and one emit launch per sequence that writes at them; then p and q of all rows at once.
static int diff_report_all(bsx_meth *a, bsx_meth *b, uint32_t min_depth, uint64_t *n_rows)
{
    a->store_valid = false;
    const uint32_t n_chr = a->n_chr;
    std::vector<uint32_t> order = diff_order(a), row_start((size_t)n_chr + 1, 0);
    std::vector<size_t> blk_off((size_t)n_chr + 1, 0);
    for (uint32_t k = 0; k < n_chr; k++) blk_off[k + 1] = blk_off[k] + (size_t)((a->chr_off[order[k] + 1] - a->chr_off[order[k]] + 1023) / 1024);
    const size_t nblk = blk_off[n_chr];
    const MethDev A = a->dev(), B = diff_dev_b(a, b);
    const RowRule R{min_depth, a->ctx_mask, 1, 0};
    size_t rows = 0;
    if (nblk) {
        HIP_TRY(a->d_blk.reserve((nblk + 1) * 4)); HIP_TRY(a->d_blk_start.reserve((nblk + 1) * 4));
        HIP_TRY(hipMemsetAsync(a->d_blk.p + nblk, 0, 4, a->stream));
        for (uint32_t k = 0; k < n_chr; k++) {
            const unsigned blocks = (unsigned)(blk_off[k + 1] - blk_off[k]);
            const u64 g0 = a->chr_off[order[k]];
            if (blocks) hipLaunchKernelGGL(k_diff_count, dim3(blocks), dim3(256), 0, a->stream, A, B, g0, a->chr_off[order[k] + 1] - g0, R, 0u, a->d_blk.p + blk_off[k]);
        }
        HIP_TRY(hipGetLastError());
        const int rc = meth_scan_u32(a, a->d_blk.p, a->d_blk_start.p, nblk + 1);
        if (rc) return rc;
        std::vector<uint32_t> starts(nblk + 1);
        HIP_TRY(hipMemcpyAsync(starts.data(), a->d_blk_start.p, (nblk + 1) * 4, hipMemcpyDeviceToHost, a->stream));
        HIP_TRY(hipStreamSynchronize(a->stream));
        for (size_t i = 0; i < nblk; i++)  // a block holds at most 1 024 rows: a sum that has passed 2^32 shows as a step down
            if (starts[i + 1] < starts[i]) { g_bsx_err = "bsx_meth_diff_report_all: the store takes fewer than 2^32 rows"; return BSX_ERR_NOMEM; }
        for (uint32_t k = 0; k <= n_chr; k++) row_start[k] = starts[blk_off[k]];
        rows = starts[nblk];
    }
    const auto no_memory = [] { g_bsx_err = "bsx_meth_diff_report_all: no device memory for the store"; return BSX_ERR_NOMEM; };
    if (a->d_store_row_start.reserve(((size_t)n_chr + 1) * 4) != hipSuccess || a->d_store_order.reserve((size_t)n_chr * 4) != hipSuccess) return no_memory();
    if (rows) {
        if (a->d_store_pos.reserve(rows * 4) != hipSuccess || a->d_store_counts.reserve(rows * 16) != hipSuccess || a->d_store_cls.reserve(rows) != hipSuccess ||
            a->d_store_p.reserve(rows * 8) != hipSuccess || a->d_store_q.reserve(rows * 8) != hipSuccess)
            return no_memory();
        for (uint32_t k = 0; k < n_chr; k++) {
            if (row_start[k + 1] == row_start[k]) continue;
            const u64 g0 = a->chr_off[order[k]];
            hipLaunchKernelGGL(k_diff_emit, dim3((unsigned)(blk_off[k + 1] - blk_off[k])), dim3(256), 0, a->stream, A, B, g0, a->chr_off[order[k] + 1] - g0, R, 0u,
                               (const uint32_t *)(a->d_blk_start.p + blk_off[k]), a->d_store_pos.p, a->d_store_counts.p, a->d_store_cls.p);
        }
        diff_fisher(a, a->d_store_counts.p, nullptr, rows, a->d_store_p.p);
        HIP_TRY(hipGetLastError());
        const int rc = meth_bh(a->stream, a->d_store_p.p, rows, a->d_store_q.p);
        if (rc) return rc;
    }
    HIP_TRY(hipMemcpyAsync(a->d_store_row_start.p, row_start.data(), ((size_t)n_chr + 1) * 4, hipMemcpyHostToDevice, a->stream));
    HIP_TRY(hipMemcpyAsync(a->d_store_order.p, order.data(), (size_t)n_chr * 4, hipMemcpyHostToDevice, a->stream));
    HIP_TRY(hipStreamSynchronize(a->stream));
    a->store_row_start.swap(row_start); a->store_order.swap(order);
    a->store_min_depth = min_depth; a->store_changes_a = a->changes; a->store_changes_b = b->changes;
    a->store_valid = true;
    *n_rows = rows;
    return BSX_OK;
}

static bool diff_store_stands(const bsx_meth *a, const bsx_meth *b, uint32_t min_depth)
{
    return a->store_valid && a->store_min_depth == min_depth && a->store_changes_a == a->changes && a->store_changes_b == b->changes;
}

// the store for (b, min_depth): the one that stands, or a new one
static int diff_store_ensure(bsx_meth *a, bsx_meth *b, uint32_t min_depth)
{
    uint64_t rows = 0;
    return diff_store_stands(a, b, min_depth) ? BSX_OK : diff_report_all(a, b, min_depth, &rows);
}

extern "C" int bsx_meth_diff_report_all(bsx_meth *a, bsx_meth *b, uint32_t min_depth, uint64_t *n_rows)
{
    if (!a || !b || !n_rows) return BSX_ERR_ARG;
    *n_rows = 0;
    const int rc_pair = diff_pair(a, b);
    if (rc_pair) return rc_pair;
    try {
        return diff_report_all(a, b, min_depth, n_rows);
    } catch (const std::bad_alloc &) {
        g_bsx_err = "bsx_meth_diff_report_all: out of host memory"; return BSX_ERR_NOMEM;
    }
}

extern "C" int bsx_meth_diff_fetch_all(bsx_meth *a, uint32_t *row_start, uint32_t *pos0, uint32_t *counts, uint8_t *cls, double *p, double *q)
{
    if (!a || !row_start || !pos0 || !counts || !cls || !p || !q) return BSX_ERR_ARG;
    if (!a->store_valid) { g_bsx_err = "bsx_meth_diff_fetch_all without a store (bsx_meth_diff_report_all)"; return BSX_ERR_STATE; }
    HIP_TRY(hipSetDevice(a->device));
    memcpy(row_start, a->store_row_start.data(), a->store_row_start.size() * 4);
    const size_t rows = a->store_row_start.back();
    if (!rows) return BSX_OK;
    HIP_TRY(hipMemcpy(pos0, a->d_store_pos.p, rows * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(counts, a->d_store_counts.p, rows * 16, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(cls, a->d_store_cls.p, rows, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(p, a->d_store_p.p, rows * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(q, a->d_store_q.p, rows * 8, hipMemcpyDeviceToHost));
    return BSX_OK;
}

// The DMRs over the store that stands: candidates (CandRule), run heads among them (HeadRule), a thread per run; the host drops the runs below min_sites
// and sends the spans through diff_regions for their sums and p.
static int diff_dmrs(bsx_meth *a, bsx_meth *b, uint32_t min_depth, double max_q, uint32_t permille, uint32_t max_gap, uint32_t min_sites, uint32_t *n_dmr)
{
    a->dmr_runs.clear(); a->dmr_sums.clear(); a->dmr_p.clear();
    *n_dmr = 0;
    const u64 rows = a->store_row_start.back();
    const StoreDev S{a->d_store_row_start.p, a->d_store_pos.p, a->d_store_counts.p, a->d_store_q.p, a->n_chr};
    DevBuf<uint32_t> d_key, d_pos, d_head;
    DevBuf<uint4> d_runs;
    uint32_t n_cand = 0, n_runs = 0, last = 0;
    int rc = meth_compact(a, rows, &n_cand, last,
        [&](unsigned nblk) { hipLaunchKernelGGL(k_cand_count, dim3(nblk), dim3(256), 0, a->stream, S, rows, max_q, permille, a->d_blk.p); },
        [&](size_t n) -> int { HIP_TRY(d_key.reserve(n * 4)); HIP_TRY(d_pos.reserve(n * 4)); return BSX_OK; },
        [&](unsigned nblk) { hipLaunchKernelGGL(k_cand_emit, dim3(nblk), dim3(256), 0, a->stream, S, rows, max_q, permille, (const uint32_t *)a->d_blk_start.p, d_key.p, d_pos.p); });
    if (rc) return rc;
    rc = meth_compact(a, n_cand, &n_runs, last,
        [&](unsigned nblk) { hipLaunchKernelGGL(k_head_count, dim3(nblk), dim3(256), 0, a->stream, (const uint32_t *)d_key.p, (const uint32_t *)d_pos.p, (u64)n_cand, max_gap, a->d_blk.p); },
        [&](size_t n) -> int { HIP_TRY(d_head.reserve(n * 4)); HIP_TRY(d_runs.reserve(n * 16)); return BSX_OK; },
        [&](unsigned nblk) {
            hipLaunchKernelGGL(k_head_emit, dim3(nblk), dim3(256), 0, a->stream, (const uint32_t *)d_key.p, (const uint32_t *)d_pos.p, (u64)n_cand, max_gap,
                               (const uint32_t *)a->d_blk_start.p, d_head.p);
        });
    if (rc || !n_runs) return rc;
    hipLaunchKernelGGL(k_dmr_runs, dim3((n_runs + 255) / 256), dim3(256), 0, a->stream, (const uint32_t *)d_head.p, n_runs, n_cand, (const uint32_t *)d_key.p,
                       (const uint32_t *)d_pos.p, (const uint32_t *)a->d_store_order.p, d_runs.p);
    HIP_TRY(hipGetLastError());
    std::vector<uint32_t> runs((size_t)n_runs * 4);
    HIP_TRY(hipMemcpyAsync(runs.data(), d_runs.p, (size_t)n_runs * 16, hipMemcpyDeviceToHost, a->stream));
    HIP_TRY(hipStreamSynchronize(a->stream));
    const size_t kept = bsx_meth_diff::keep_runs(runs.data(), n_runs, min_sites);
    runs.resize(kept * 4);
    if (!kept) return BSX_OK;
    std::vector<uint32_t> chr(kept), start(kept), end(kept);
    for (size_t i = 0; i < kept; i++) { chr[i] = runs[i * 4]; start[i] = runs[i * 4 + 1]; end[i] = runs[i * 4 + 2]; }
    std::vector<uint64_t> sums(kept * 5);
    std::vector<double> p(kept);
    rc = diff_regions(a, b, (uint32_t)kept, chr.data(), start.data(), end.data(), min_depth, sums.data(), p.data());
    if (rc) return rc;
    a->dmr_runs.swap(runs); a->dmr_sums.swap(sums); a->dmr_p.swap(p);
    *n_dmr = (uint32_t)kept;
    return BSX_OK;
}

static const char *const NO_STORE = "no store of bsx_meth_diff_report_all stands for this pair and min_depth";

extern "C" int bsx_meth_diff_dmrs(bsx_meth *a, bsx_meth *b, uint32_t min_depth, const double *max_q, uint32_t min_delta_permille, uint32_t max_gap, uint32_t min_sites,
                                  uint32_t *n_dmr)
{
    if (!a || !b || !max_q || !n_dmr || min_delta_permille > 1000 || !min_sites || !(*max_q >= 0.0 && *max_q <= 1.0)) return BSX_ERR_ARG;
    *n_dmr = 0;
    const int rc_pair = diff_pair(a, b);
    if (rc_pair) return rc_pair;
    if (!diff_store_stands(a, b, min_depth)) { g_bsx_err = NO_STORE; return BSX_ERR_STATE; }
    try {
        return diff_dmrs(a, b, min_depth, *max_q, min_delta_permille, max_gap, min_sites, n_dmr);
    } catch (const std::bad_alloc &) {
        g_bsx_err = "bsx_meth_diff_dmrs: out of host memory"; return BSX_ERR_NOMEM;
    }
}

extern "C" int bsx_meth_diff_fetch_dmrs(bsx_meth *a, uint32_t *chr, uint32_t *start, uint32_t *end, uint32_t *n_sig, uint64_t *sums, double *p)
{
    if (!a) return BSX_ERR_ARG;
    const size_t n = a->dmr_p.size();
    if (n && (!chr || !start || !end || !n_sig || !sums || !p)) return BSX_ERR_ARG;
    for (size_t i = 0; i < n; i++) { chr[i] = a->dmr_runs[i * 4]; start[i] = a->dmr_runs[i * 4 + 1]; end[i] = a->dmr_runs[i * 4 + 2]; n_sig[i] = a->dmr_runs[i * 4 + 3]; }
    if (n) { memcpy(sums, a->dmr_sums.data(), n * 40); memcpy(p, a->dmr_p.data(), n * 8); }
    return BSX_OK;
}

namespace {

int write_diff(bsx_meth *a, bsx_meth *b, const char *path, uint32_t min_depth, uint32_t min_delta_permille, const double *max_p, uint64_t *n_rows)
{
    OutFile out(path);
    if (!out.f) return out.cannot_write();
    fputs(bsx_meth_diff::POS_HEADER, out.f);
    std::vector<uint32_t> pos, counts;
    std::vector<uint8_t> cls;
    std::vector<double> p;
    uint64_t total = 0;
    for (const uint32_t c : sorted_chromosomes(a)) {
        uint32_t rows = 0;
        int rc = bsx_meth_diff_report_chr(a, b, c, min_depth, min_delta_permille, &rows);
        if (rc) return rc;
        if (!rows) continue;
        pos.resize(rows); counts.resize((size_t)rows * 4); cls.resize(rows); p.resize(rows);
        rc = bsx_meth_diff_fetch_rows(a, pos.data(), counts.data(), p.data());
        if (rc) return rc;
        if (hipMemcpy(cls.data(), a->d_diff_cls.p, rows, hipMemcpyDeviceToHost) != hipSuccess) return BSX_ERR_DEVICE;
        const char *name = a->names[c].c_str();
        format_rows(out.f, rows, 72, [&](size_t i, std::string &o) { if (!max_p || p[i] <= *max_p) bsx_meth_diff::append_pos_row(o, name, pos[i], cls[i], &counts[i * 4], p[i]); });
        for (size_t i = 0; i < rows; i++) total += !max_p || p[i] <= *max_p;
    }
    const int rc_close = out.finish();
    if (rc_close) return rc_close;
    if (n_rows) *n_rows = total;
    return BSX_OK;
}

// fdr: with the q column, Benjamini-Hochberg over the intervals with a common site (bsx_meth_bh)
int write_diff_regions(bsx_meth *a, bsx_meth *b, const char *bed_path, const char *out_path, uint32_t min_depth, bool fdr, uint64_t *n_written, uint64_t *n_dropped)
{
    bsx_meth_parse::BedRecords bed;
    const int rc_bed = read_bed(a, bed_path, bed);
    if (rc_bed) return rc_bed;
    const size_t n = bed.chr.size();
    std::vector<uint64_t> sums(n * 5 + 1);
    std::vector<double> p(n + 1);
    const int rc = bsx_meth_diff_regions(a, b, (uint32_t)n, bed.chr.data(), bed.start.data(), bed.end.data(), min_depth, sums.data(), p.data());
    if (rc) return rc;
    std::vector<double> q(fdr ? n + 1 : 0);
    if (fdr) { const int rc_q = bsx_meth_bh(a->device, p.data(), n, q.data()); if (rc_q) return rc_q; }
    OutFile out(out_path);
    if (!out.f) return out.cannot_write();
    fputs(fdr ? bsx_meth_diff::REGION_FDR_HEADER : bsx_meth_diff::REGION_HEADER, out.f);
    format_rows(out.f, n, 80, [&](size_t i, std::string &o) {
        bsx_meth_diff::append_interval_row(o, a->names[bed.chr[i]].c_str(), bed.start[i], bed.end[i], &bed.label[i], &sums[i * 5], p[i]);
        if (fdr) bsx_meth_diff::append_q(o, q[i]);
    });
    const int rc_close = out.finish();
    if (rc_close) return rc_close;
    if (n_written) *n_written = n;
    if (n_dropped) *n_dropped = bed.dropped;
    return BSX_OK;
}

// the bins of every sequence as intervals [j bin, min((j + 1) bin, length)) of bsx_meth_diff_regions, REGION_CHUNK of them per call
int write_diff_bins(bsx_meth *a, bsx_meth *b, const char *path, uint32_t bin, uint32_t min_depth, uint64_t *n_rows)
{
    OutFile out(path);
    if (!out.f) return out.cannot_write();
    fputs(bsx_meth_diff::BIN_HEADER, out.f);
    std::vector<uint32_t> chr, start, end;
    std::vector<uint64_t> sums;
    std::vector<double> p;
    uint64_t total = 0;
    for (const uint32_t c : sorted_chromosomes(a)) {
        const u64 len = a->chr_off[c + 1] - a->chr_off[c], n_bins = (len + bin - 1) / bin;
        const char *name = a->names[c].c_str();
        for (u64 j0 = 0; j0 < n_bins; j0 += REGION_CHUNK) {
            const size_t k = (size_t)std::min<u64>(REGION_CHUNK, n_bins - j0);
            chr.assign(k, c); start.resize(k); end.resize(k); sums.resize(k * 5); p.resize(k);
            for (size_t j = 0; j < k; j++) { start[j] = (uint32_t)((j0 + j) * bin); end[j] = (uint32_t)std::min<u64>((j0 + j + 1) * bin, len); }
            const int rc = bsx_meth_diff_regions(a, b, (uint32_t)k, chr.data(), start.data(), end.data(), min_depth, sums.data(), p.data());
            if (rc) return rc;
            format_rows(out.f, k, 16, [&](size_t j, std::string &o) { if (sums[j * 5]) bsx_meth_diff::append_interval_row(o, name, start[j], end[j], nullptr, &sums[j * 5], p[j]); });
            for (size_t j = 0; j < k; j++) total += sums[j * 5] != 0;
        }
    }
    const int rc_close = out.finish();
    if (rc_close) return rc_close;
    if (n_rows) *n_rows = total;
    return BSX_OK;
}

// The position file with q: formatted from the store (every common site with its p and the q of the whole family), a sequence at a time; the delta rule,
// max_p and max_q choose among the fetched rows what is written and change no printed value.
int write_diff_fdr(bsx_meth *a, bsx_meth *b, const char *path, uint32_t min_depth, uint32_t min_delta_permille, const double *max_p, const double *max_q, uint64_t *n_rows)
{
    const int rc_store = diff_store_ensure(a, b, min_depth);
    if (rc_store) return rc_store;
    OutFile out(path);
    if (!out.f) return out.cannot_write();
    fputs(bsx_meth_diff::POS_FDR_HEADER, out.f);
    std::vector<uint32_t> pos, counts;
    std::vector<uint8_t> cls, listed;
    std::vector<double> p, q;
    uint64_t total = 0;
    for (uint32_t k = 0; k < a->n_chr; k++) {
        const size_t lo = a->store_row_start[k], rows = a->store_row_start[k + 1] - lo;
        if (!rows) continue;
        pos.resize(rows); counts.resize(rows * 4); cls.resize(rows); p.resize(rows); q.resize(rows);
        HIP_TRY(hipMemcpy(pos.data(), a->d_store_pos.p + lo, rows * 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(counts.data(), a->d_store_counts.p + lo, rows * 16, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(cls.data(), a->d_store_cls.p + lo, rows, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(p.data(), a->d_store_p.p + lo, rows * 8, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(q.data(), a->d_store_q.p + lo, rows * 8, hipMemcpyDeviceToHost));
        const char *name = a->names[a->store_order[k]].c_str();
        listed.resize(rows);  // decided once per row: the count and the file cannot disagree
        for (size_t i = 0; i < rows; i++) {
            const uint32_t *c = &counts[i * 4];
            listed[i] = bsx_meth_diff::delta_keeps(c[0], c[1], c[2], c[3], min_delta_permille) && (!max_p || p[i] <= *max_p) && (!max_q || q[i] <= *max_q);
            total += listed[i];
        }
        format_rows(out.f, rows, 84, [&](size_t i, std::string &o) {
            if (!listed[i]) return;
            bsx_meth_diff::append_pos_row(o, name, pos[i], cls[i], &counts[i * 4], p[i]);
            bsx_meth_diff::append_q(o, q[i]);
        });
    }
    const int rc_close = out.finish();
    if (rc_close) return rc_close;
    if (n_rows) *n_rows = total;
    return BSX_OK;
}

int write_dmrs(bsx_meth *a, bsx_meth *b, const char *path, uint32_t min_depth, double max_q, uint32_t min_delta_permille, uint32_t max_gap, uint32_t min_sites,
               uint64_t *n_rows)
{
    int rc = diff_store_ensure(a, b, min_depth);
    if (rc) return rc;
    uint32_t n = 0;
    rc = diff_dmrs(a, b, min_depth, max_q, min_delta_permille, max_gap, min_sites, &n);
    if (rc) return rc;
    OutFile out(path);
    if (!out.f) return out.cannot_write();
    fputs(bsx_meth_diff::DMR_HEADER, out.f);
    format_rows(out.f, n, 96, [&](size_t i, std::string &o) {
        const uint32_t *r = &a->dmr_runs[i * 4];
        bsx_meth_diff::append_dmr_row(o, a->names[r[0]].c_str(), r[1], r[2], r[3], &a->dmr_sums[i * 5], a->dmr_p[i]);
    });
    const int rc_close = out.finish();
    if (rc_close) return rc_close;
    if (n_rows) *n_rows = n;
    return BSX_OK;
}

}  // namespace

extern "C" int bsx_meth_write_diff(bsx_meth *a, bsx_meth *b, const char *path, uint32_t min_depth, uint32_t min_delta_permille, const double *max_p, uint64_t *n_rows)
{
    if (!a || !b || !path || min_delta_permille > 1000 || a->names.size() != a->n_chr) return BSX_ERR_ARG;
    if (n_rows) *n_rows = 0;
    const int rc_pair = diff_pair(a, b);  // ahead of the file: a pair that cannot be compared leaves nothing behind
    if (rc_pair) return rc_pair;
    return guarded(path, "writing", [&] { return write_diff(a, b, path, min_depth, min_delta_permille, max_p, n_rows); });
}

extern "C" int bsx_meth_write_diff_regions(bsx_meth *a, bsx_meth *b, const char *bed_path, const char *out_path, uint32_t min_depth, uint64_t *n_written, uint64_t *n_dropped)
{
    if (!a || !b || !bed_path || !out_path || a->names.size() != a->n_chr) return BSX_ERR_ARG;
    if (n_written) *n_written = 0;
    if (n_dropped) *n_dropped = 0;
    const int rc_pair = diff_pair(a, b);
    if (rc_pair) return rc_pair;
    return guarded(out_path, "writing", [&] { return write_diff_regions(a, b, bed_path, out_path, min_depth, false, n_written, n_dropped); });
}

extern "C" int bsx_meth_write_diff_bins(bsx_meth *a, bsx_meth *b, const char *path, uint32_t bin, uint32_t min_depth, uint64_t *n_rows)
{
    if (!a || !b || !path || !bin || a->names.size() != a->n_chr) return BSX_ERR_ARG;
    if (n_rows) *n_rows = 0;
    const int rc_pair = diff_pair(a, b);
    if (rc_pair) return rc_pair;
    return guarded(path, "writing", [&] { return write_diff_bins(a, b, path, bin, min_depth, n_rows); });
}

extern "C" int bsx_meth_write_diff_fdr(bsx_meth *a, bsx_meth *b, const char *path, uint32_t min_depth, uint32_t min_delta_permille, const double *max_p, const double *max_q,
                                       uint64_t *n_rows)
{
    if (!a || !b || !path || !n_rows || min_delta_permille > 1000 || a->names.size() != a->n_chr) return BSX_ERR_ARG;
    for (const double *limit : {max_p, max_q}) if (limit && !(*limit >= 0.0 && *limit <= 1.0)) return BSX_ERR_ARG;  // (a NaN fails both comparisons)
    *n_rows = 0;
    const int rc_pair = diff_pair(a, b);
    if (rc_pair) return rc_pair;
    return guarded(path, "writing", [&] { return write_diff_fdr(a, b, path, min_depth, min_delta_permille, max_p, max_q, n_rows); });
}

extern "C" int bsx_meth_write_diff_regions_fdr(bsx_meth *a, bsx_meth *b, const char *bed_path, const char *out_path, uint32_t min_depth, uint64_t *n_written, uint64_t *n_dropped)
{
    if (!a || !b || !bed_path || !out_path || a->names.size() != a->n_chr) return BSX_ERR_ARG;
    if (n_written) *n_written = 0;
    if (n_dropped) *n_dropped = 0;
    const int rc_pair = diff_pair(a, b);
    if (rc_pair) return rc_pair;
    return guarded(out_path, "writing", [&] { return write_diff_regions(a, b, bed_path, out_path, min_depth, true, n_written, n_dropped); });
}

extern "C" int bsx_meth_write_dmrs(bsx_meth *a, bsx_meth *b, const char *path, uint32_t min_depth, const double *max_q, uint32_t min_delta_permille, uint32_t max_gap,
                                   uint32_t min_sites, uint64_t *n_rows)
{
    if (!a || !b || !path || !max_q || !n_rows || min_delta_permille > 1000 || !min_sites || !(*max_q >= 0.0 && *max_q <= 1.0) || a->names.size() != a->n_chr) return BSX_ERR_ARG;
    *n_rows = 0;
    const int rc_pair = diff_pair(a, b);
    if (rc_pair) return rc_pair;
    return guarded(path, "writing", [&] { return write_dmrs(a, b, path, min_depth, *max_q, min_delta_permille, max_gap, min_sites, n_rows); });
}
