// bsx_rows.h — the LDS row of a member of k_hscan_same's WGBS groups of 129-160 nt reads without the work counters (hs_group<5, false, false>, bsx_align.hip),
// in the order in which its words are evaluated: 0, 4, 3, 2, 1 (same_exit).  Host and device: tests/harness/rows_check.cpp drives the same functions on the CPU.
//
//   quarter 0:  X0 Y0 M0 T     T = threshold | plain << 16 | offset class d << 17 (plain: no N in words 0-3, they take the two-operation form)
//   quarter 1:  X4 Y4 M4 M1
//   quarter 2:  X3 Y3 M3 X2
//   quarter 3:  Y2 M2 X1 Y1
//   quarter 4:  task, first list ordinal, -, -
//
// The first half (quarters 0 and 1) is all that the first two evaluated words need, and hs_group requests it a read ahead; the second half (quarters 2 and 3)
// is requested only once a chunk of the read is still alive behind the second evaluated word.  The planes of words 3, 2, 1 are nine dwords: the ninth, the
// not-N plane of word 1, fills the free dword of quarter 1 — only a read with an N looks at it, so a plain read that gets to its last word needs no third request.
// X, Y: low and high bit planes of the read's letters, M: its not-N plane (bsx_dev.h).
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BSX_ROWS_HD __host__ __device__
#else
#define BSX_ROWS_HD
#endif

#define BSX_ROW_DWORDS 20
#define BSX_ROW_TASK 16
#define BSX_ROW_ORD 17

// the read word that is evaluated i-th, i = 0 .. 4
BSX_ROWS_HD inline int bsx_row_eval_word(int i) { return i == 0 ? 0 : 5 - i; }

// px, py, pm: the five words of the read's planes; t: the T dword
BSX_ROWS_HD inline void bsx_row_pack(uint32_t *row, const uint32_t *px, const uint32_t *py, const uint32_t *pm, uint32_t t)
{
    row[0] = px[0]; row[1] = py[0]; row[2] = pm[0]; row[3] = t;
    row[4] = px[4]; row[5] = py[4]; row[6] = pm[4]; row[7] = pm[1];
    row[8] = px[3]; row[9] = py[3]; row[10] = pm[3]; row[11] = px[2];
    row[12] = py[2]; row[13] = pm[2]; row[14] = px[1]; row[15] = py[1];
}

// the T dword of a row, from its first half
template <class Q> BSX_ROWS_HD inline uint32_t bsx_row_t(const Q &q0) { return q0.w; }

// the planes of the i-th evaluated word.  i = 0, 1 read quarters 0 and 1 only; i = 2, 3, 4 read quarters 2 and 3, and the M of i = 4 (word 1) quarter 1.
// (i is a constant wherever this is inlined.)  Q: four dwords x, y, z, w
template <class Q> BSX_ROWS_HD inline void bsx_row_word(int i, const Q &q0, const Q &q1, const Q &q2, const Q &q3, uint32_t &X, uint32_t &Y, uint32_t &M)
{
    switch (i) {
    case 0: X = q0.x; Y = q0.y; M = q0.z; break;
    case 1: X = q1.x; Y = q1.y; M = q1.z; break;
    case 2: X = q2.x; Y = q2.y; M = q2.z; break;
    case 3: X = q2.w; Y = q3.x; M = q3.y; break;
    default: X = q3.z; Y = q3.w; M = q1.w; break;
    }
}

// Host model of the ways a read leaves the HG_C = 4 chunks of a step (hs_eval_lean, HG_JOINT).  cnt[u][l][i]: the mismatches of chunk u's candidate l in the i-th
// evaluated word; valid[u]: the lanes of chunk u that hold a candidate.  A chunk is alive behind a word while one of its candidates is within the threshold.
//   mode 0, chunk-major: a chunk takes its words one after the other and is left behind the first word that no candidate survives;
//   mode 1, joint: word i of all chunks that are still alive, and the read is left for the step once no chunk is — a chunk that is not alive takes no further part;
//   mode 2, joint: the same, but a chunk that is not alive is evaluated all the same, and ignored, as long as another one is alive.
//   mode 3, joint, the shipped form (HG_JOINT = 3): where every lane of every chunk holds a candidate, one test per word — is the smallest of a lane's four counts
//           within the threshold in any lane — and the chunks' own ballots only behind the last word; elsewhere mode 2.  The smallest of four counts is within the
//           threshold iff one of them is, so the test is the OR of mode 2's four ballots, and a chunk that mode 2 ignores has no lane left behind the last word.
// All write keep[u] = the lanes within the threshold behind the last word (0 where the chunk was left early) and return the words evaluated, summed over the chunks.
BSX_ROWS_HD inline uint32_t bsx_rows_exit_model(int mode, const uint8_t (*cnt)[64][5], const uint64_t *valid, uint32_t thr, uint64_t *keep)
{
    uint32_t words = 0, tot[4][64];
    uint64_t al[4];
    for (int u = 0; u < 4; u++) { al[u] = valid[u]; for (int l = 0; l < 64; l++) tot[u][l] = 0; }
    if (mode == 3 && (valid[0] & valid[1] & valid[2] & valid[3]) == ~0ull) {
        for (int i = 0; i < 5; i++) {
            bool any = false;
            for (int l = 0; l < 64; l++) {
                uint32_t mn = 0xffffffffu;
                for (int u = 0; u < 4; u++) { tot[u][l] += cnt[u][l][i]; if (tot[u][l] < mn) mn = tot[u][l]; }
                any = any || mn <= thr;
            }
            words += 4;
            if (!any) { for (int u = 0; u < 4; u++) keep[u] = 0; return words; }
        }
        for (int u = 0; u < 4; u++) { keep[u] = 0; for (int l = 0; l < 64; l++) if (tot[u][l] <= thr) keep[u] |= 1ull << l; }
        return words;
    }
    if (mode == 3) mode = 2;
    for (int a = 0; a < (mode ? 5 : 4); a++) {
        if (mode && !(al[0] | al[1] | al[2] | al[3])) break;
        for (int b = 0; b < (mode ? 4 : 5); b++) {
            const int i = mode ? a : b, u = mode ? b : a;
            if (!al[u] && mode != 2) continue;
            uint64_t m = 0;
            for (int l = 0; l < 64; l++) { tot[u][l] += cnt[u][l][i]; if (tot[u][l] <= thr) m |= 1ull << l; }
            al[u] &= m;
            words++;
        }
    }
    for (int u = 0; u < 4; u++) keep[u] = al[u];
    return words;
}
