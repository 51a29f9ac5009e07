// bsx_rows.h: the LDS row of k_hscan_same's groups of 129-160 nt reads in the order of evaluation (0, 4, 3, 2, 1), packed and read back half by half, over random
// and directed reads — planes, thresholds and N masks, a last word of 1 .. 32 letters (1 and 16 directed) — against the mismatch counts of bsx_plane_mismatch and
// bsx_plane_mismatch_full on the unpacked planes; and the host model of the ways a read leaves the four chunks of a step (bsx_rows_exit_model): the joint forms
// keep exactly the candidates that the chunk-major form keeps, with their whole counts, the skipping form in the same number of words, and the shipped form
// (HG_JOINT = 3: one test per word on the smallest of a lane's four counts in full steps) leaves where the form with four ballots leaves.
#include <cstdio>
#include <cstdint>
#include <cstring>
#include "../../bsmap_amd/csrc/bsx_dev.h"
#include "../../bsmap_amd/csrc/bsx_rows.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 16); }

struct Q4 { uint32_t x, y, z, w; };
static const uint32_t POISON = 0xdeadbeefu;

#define FAIL(...) do { printf("FAIL %s: ", what); printf(__VA_ARGS__); printf("\n"); return false; } while (0)

// one read (its planes; last: the letters of word 4; n_at: a word that holds an N at letter n_bit, or -1) against `frames` random reference frames
static bool check_read(const char *what, uint32_t last, int n_at, int n_bit, uint32_t thr, uint32_t d, int frames)
{
    uint32_t px[8], py[8], pm[8];
    for (int j = 0; j < 8; j++) { px[j] = py[j] = pm[j] = 0; }
    uint32_t inner = 0xFFFFFFFFu;
    for (int j = 0; j < 5; j++) {
        pm[j] = j < 4 ? 0xFFFFFFFFu : (last == 32 ? 0xFFFFFFFFu : ~(0xFFFFFFFFu >> last));   // (first letter in bit 31)
        if (j == n_at) pm[j] &= ~(0x80000000u >> n_bit);
        px[j] = rnd() & pm[j]; py[j] = rnd() & pm[j];   // (a letter that is N or behind the read's end has both planes clear)
        if (j < 4) inner &= pm[j];
    }
    const bool plain = inner == 0xFFFFFFFFu;
    const uint32_t t = thr | (plain ? 0x10000u : 0u) | (d << 17);
    uint32_t row[BSX_ROW_DWORDS + 1];
    for (int i = 0; i <= BSX_ROW_DWORDS; i++) row[i] = POISON;
    bsx_row_pack(row, px, py, pm, t);
    for (int i = 16; i <= BSX_ROW_DWORDS; i++) if (row[i] != POISON) FAIL("the pack wrote dword %d", i);
    // the first half alone serves the first two evaluated words, the threshold, the plain flag and the class
    Q4 q0, q1, q2 = {POISON, POISON, POISON, POISON}, q3 = q2;
    memcpy(&q0, row, 16); memcpy(&q1, row + 4, 16);
    if (bsx_row_t(q0) != t || (bsx_row_t(q0) & 0xffffu) != thr || ((bsx_row_t(q0) >> 16) & 1u) != (plain ? 1u : 0u) || (bsx_row_t(q0) >> 17) != d) FAIL("T");
    if (bsx_row_eval_word(0) != 0 || bsx_row_eval_word(1) != 4 || bsx_row_eval_word(2) != 3 || bsx_row_eval_word(3) != 2 || bsx_row_eval_word(4) != 1) FAIL("order");
    for (int f = 0; f < frames; f++) {
        uint32_t rlo[5], rhi[5];
        for (int j = 0; j < 5; j++) {
            rlo[j] = rnd(); rhi[j] = rnd();
            if (f & 1) { rlo[j] = px[j] ^ (rnd() & rnd() & rnd()); rhi[j] = py[j] ^ (rnd() & rnd() & rnd()); }   // (a near copy of the read: small counts)
        }
        for (int half = 0; half < 2; half++) {
            if (half == 1) { memcpy(&q2, row + 8, 16); memcpy(&q3, row + 12, 16); }
            for (int i = half ? 2 : 0; i < (half ? 5 : 2); i++) {
                const int j = bsx_row_eval_word(i);
                uint32_t X, Y, M;
                bsx_row_word(i, q0, q1, q2, q3, X, Y, M);
                if (X != px[j] || Y != py[j] || M != pm[j]) FAIL("evaluated word %d (read word %d): planes %08x %08x %08x, packed from %08x %08x %08x", i, j, X, Y, M, px[j], py[j], pm[j]);
                // the count as the kernel forms it (two operations for words 0-3 of a plain read, three otherwise) and as the unpacked planes give it
                const uint32_t got = (plain && j < 4) ? bsx_plane_mismatch_full(rlo[j], rhi[j], X, Y) : bsx_plane_mismatch(rlo[j], rhi[j], X, Y, M);
                const uint32_t want = bsx_plane_mismatch(rlo[j], rhi[j], px[j], py[j], pm[j]);
                if (__builtin_popcount(got) != __builtin_popcount(want) || got != want) FAIL("evaluated word %d (read word %d): mismatches %08x, unpacked %08x", i, j, got, want);
                if (pm[j] == 0xFFFFFFFFu && bsx_plane_mismatch_full(rlo[j], rhi[j], px[j], py[j]) != want) FAIL("word %d: the two-operation form", j);
            }
        }
        q2 = {POISON, POISON, POISON, POISON}; q3 = q2;
    }
    return true;
}

// counts of four chunks: kind 0 random, 1 most chunks fail early, 2 one chunk holds a survivor, 3 every chunk holds one, 4 partial chunks
static bool check_model(const char *what, int kind, uint32_t thr)
{
    static uint8_t cnt[4][64][5];
    uint64_t valid[4], keep[4][4];
    for (int u = 0; u < 4; u++) {
        valid[u] = ~0ull;
        if (kind == 4) valid[u] = u == 0 ? ~0ull : u == 1 ? (rnd() | ((uint64_t)rnd() << 32)) : u == 2 ? 1ull << 63 : 0ull;
        for (int l = 0; l < 64; l++)
            for (int i = 0; i < 5; i++) {
                uint32_t c = rnd() % (kind == 1 ? 2 * thr + 4 : thr + 2);
                if (kind == 0) c = rnd() % 9;
                cnt[u][l][i] = (uint8_t)(c > 32 ? 32 : c);
            }
        if ((kind == 2 && u == (int)(rnd() & 3)) || kind == 3 || kind == 4) { const int l = kind == 4 && u == 2 ? 63 : (int)(rnd() & 63); for (int i = 0; i < 5; i++) cnt[u][l][i] = 0; cnt[u][l][rnd() % 5] = (uint8_t)thr; }
    }
    uint32_t words[4];
    for (int m = 0; m < 4; m++) words[m] = bsx_rows_exit_model(m, cnt, valid, thr, keep[m]);
    // what the result is: the candidates within the threshold over all five words
    for (int u = 0; u < 4; u++) {
        uint64_t want = 0;
        for (int l = 0; l < 64; l++) { uint32_t s = 0; for (int i = 0; i < 5; i++) s += cnt[u][l][i]; if (s <= thr && ((valid[u] >> l) & 1)) want |= 1ull << l; }
        for (int m = 0; m < 4; m++) if (keep[m][u] != want) FAIL("mode %d chunk %d keeps %016llx, within the threshold %016llx", m, u, (unsigned long long)keep[m][u], (unsigned long long)want);
    }
    if (words[1] != words[0]) FAIL("the skipping joint form took %u words, chunk-major %u", words[1], words[0]);
    if (words[2] < words[0] || words[2] > 20) FAIL("the ignoring joint form took %u words, chunk-major %u", words[2], words[0]);
    if (words[3] != words[2]) FAIL("the shipped form (one test on the smallest count) took %u words, the ignoring joint form %u", words[3], words[2]);   // (the same exits, word for word)
    return true;
}

int main()
{
    int n = 0;
    // directed: a last word of 1 and of 16 letters (129 and 144 nt), plain and with an N in every word, at both ends of the word; thresholds 0, 2, 6 and the largest; classes 0-2
    const uint32_t lasts[] = {1, 16, 32, 31}, thrs[] = {0, 2, 6, 15, 0xffffu};
    for (uint32_t last : lasts)
        for (uint32_t thr : thrs)
            for (uint32_t d = 0; d < 3; d++)
                for (int n_at = -1; n_at < 5; n_at++)
                    for (int n_bit : {0, 31}) {
                        if (n_at == 4 && (uint32_t)n_bit >= last) continue;
                        if (!check_read("directed", last, n_at, n_bit, thr, d, 8)) return 1;
                        n++;
                    }
    for (int r = 0; r < 20000; r++) {
        const uint32_t last = 1 + rnd() % 32;
        const int n_at = (rnd() & 1) ? -1 : (int)(rnd() % 5);
        int n_bit = (int)(rnd() % 32);
        if (n_at == 4) n_bit %= (int)last;
        if (!check_read("random", last, n_at, n_bit, rnd() % 16, rnd() % 3, 4)) return 1;
        n++;
    }
    int nm = 0;
    for (int r = 0; r < 20000; r++) {
        if (!check_model("model", r % 5, thrs[rnd() & 3])) return 1;
        nm++;
    }
    printf("ok %d rows, %d steps of the exit model\n", n, nm);
    return 0;
}
