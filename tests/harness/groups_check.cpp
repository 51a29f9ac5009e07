// bsx_group_cut (bsx_groups.h): the rule by which k_task_groups cuts a sorted run of tasks of one window and congruence class into groups, over random and
// directed runs: every task in exactly one group, sizes 1 .. Rg, members within 32 D of the frame and congruent to it, rows sorted by d with d = 0 in row 0,
// ceil(N / Rg) groups of near-equal size for a run that one frame holds, no group of one from such a run, at most N turns.
#include <algorithm>
#include <cstdio>
#include <cstdint>
#include <vector>
#include "../../bsmap_amd/csrc/bsx_groups.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 16); }

// offs: signed offsets of one class, any order.  stride / hstride: as the kernel calls it (keys of four words) and as plain arrays.
static bool check(std::vector<int32_t> offs, uint32_t D, uint32_t Rg, uint32_t stride, std::vector<uint32_t> *sizes_out, const char *what)
{
    std::sort(offs.begin(), offs.end());
    const uint32_t n = (uint32_t)offs.size();
    std::vector<uint32_t> key((size_t)n * stride + 1, 0xdeadbeefu), head((size_t)n + 1, 0xdeadbeefu);
    for (uint32_t i = 0; i < n; i++) key[(size_t)i * stride] = (uint32_t)offs[i] ^ 0x80000000u;
    const uint32_t turns = bsx_group_cut(key.data(), stride, n, D, Rg, head.data(), 1u);
#define FAIL(...) do { printf("FAIL %s n %u D %u Rg %u: ", what, n, D, Rg); printf(__VA_ARGS__); printf("\n"); return false; } while (0)
    if (head[n] != 0xdeadbeefu) FAIL("wrote behind the run");
    if (turns > n) FAIL("%u turns", turns);
    std::vector<uint32_t> sizes;
    uint32_t p = 0;
    while (p < n) {
        const uint32_t k = head[p];
        if (k < 1 || k > Rg || p + k > n) FAIL("group at %u of %u tasks", p, k);
        for (uint32_t j = 1; j < k; j++) if (head[p + j] != 0) FAIL("task %u is in the group at %u and starts one of %u", p + j, p, head[p + j]);   // (every task in exactly one group)
        uint32_t d_prev = 0;
        for (uint32_t j = 0; j < k; j++) {
            const int64_t dh = (int64_t)offs[p + j] - (int64_t)offs[p];
            if (dh < 0 || dh > 32 * (int64_t)D || (dh & 31)) FAIL("task %u: offset %d in the frame %d", p + j, offs[p + j], offs[p]);
            const uint32_t d = (uint32_t)(dh / 32);
            if (j == 0 ? d != 0 : d < d_prev) FAIL("rows of the group at %u are not sorted by d", p);
            d_prev = d;
        }
        sizes.push_back(k);
        p += k;
    }
    if (sizes.size() != turns) FAIL("%zu groups, %u returned", sizes.size(), turns);
    if (n && (int64_t)offs[n - 1] - (int64_t)offs[0] <= 32 * (int64_t)D) {   // one frame could hold the whole run
        if (sizes.size() != (n + Rg - 1) / Rg) FAIL("%zu groups of a run that one frame holds", sizes.size());
        const uint32_t lo = *std::min_element(sizes.begin(), sizes.end()), hi = *std::max_element(sizes.begin(), sizes.end());
        if (hi - lo > 1) FAIL("sizes %u .. %u", lo, hi);
        if (n >= 2 && Rg >= 2 && lo < 2) FAIL("a group of one");
    }
#undef FAIL
    if (sizes_out) *sizes_out = sizes;
    return true;
}

int main()
{
    long checked = 0;
    const uint32_t Ns[] = {1, 2, 63, 64, 65, 127, 128, 129, 1024}, Rgs[] = {1, 16, 64}, Ds[] = {0, 1, 2};
    for (uint32_t n : Ns)
        for (uint32_t Rg : Rgs)
            for (uint32_t D : Ds)
                for (uint32_t classes = 1; classes <= 5; classes++)
                    for (int rep = 0; rep < 8; rep++) {
                        // offsets of one congruence class: `classes` values of h >> 5 around zero (h is minus the seed's place in the read: mostly negative)
                        const int32_t low = (int32_t)(rnd() & 31u), first = -(int32_t)(rnd() % 5u);
                        std::vector<int32_t> offs(n);
                        for (uint32_t i = 0; i < n; i++) {
                            // rep 0-3 uniform over the classes, 4-5 nearly all in one class, 6 the classes in equal blocks, 7 one task in each class but the last
                            const uint32_t c = rep < 4 ? rnd() % classes : rep < 6 ? (rnd() % 16u ? classes - 1 : rnd() % classes) : rep == 6 ? i * classes / n : (i < classes ? i : classes - 1);
                            offs[i] = 32 * (first + (int32_t)c) + low - 32 * (rep & 1);
                        }
                        if (!check(offs, D, Rg, (rep & 1) ? 4u : 1u, nullptr, "random")) return 1;
                        checked++;
                    }
    // the cuts the text names
    std::vector<uint32_t> sz;
    if (!check(std::vector<int32_t>(70, -48), 0, 64, 4, &sz, "70") || sz != std::vector<uint32_t>{35, 35}) { printf("FAIL 70 tasks are not 35 + 35\n"); return 1; }
    if (!check(std::vector<int32_t>(65, -48), 2, 64, 4, &sz, "65") || sz != std::vector<uint32_t>{33, 32}) { printf("FAIL 65 tasks are not 33 + 32\n"); return 1; }
    if (!check(std::vector<int32_t>(17, 5), 0, 16, 1, &sz, "17") || sz != std::vector<uint32_t>{9, 8}) { printf("FAIL 17 tasks at Rg 16 are not 9 + 8\n"); return 1; }
    {   // 40 + 30 at offsets 32 apart, D = 2: one frame holds all 70
        std::vector<int32_t> o(40, -64); o.insert(o.end(), 30, -32);
        if (!check(o, 2, 64, 4, &sz, "40 + 30") || sz != std::vector<uint32_t>{35, 35}) { printf("FAIL 40 + 30\n"); return 1; }
        // ... D = 0: a class is a run of its own frame
        if (!check(o, 0, 64, 4, &sz, "40 + 30, D 0") || sz != std::vector<uint32_t>{40, 30}) { printf("FAIL 40 + 30 at D 0\n"); return 1; }
    }
    {   // the frame moves on: offsets 0, 32, 64, 96 with D = 2 — the first frame reaches 64, the task at 96 needs a later one
        std::vector<int32_t> o = {0, 32, 64, 96};
        if (!check(o, 2, 64, 1, &sz, "moving frame") || sz != std::vector<uint32_t>{3, 1}) { printf("FAIL moving frame\n"); return 1; }
    }
    {   // the extremes of the signed range do not wrap
        std::vector<int32_t> o = {INT32_MIN, INT32_MIN + 32, INT32_MAX - 63, INT32_MAX - 31};
        if (!check(o, 1, 64, 1, &sz, "extremes") || sz != std::vector<uint32_t>{2, 2}) { printf("FAIL extremes\n"); return 1; }
    }
    checked += 7;
    printf("ok %ld runs\n", checked);
    return 0;
}
