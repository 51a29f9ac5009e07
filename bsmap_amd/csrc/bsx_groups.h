// bsx_groups.h — how k_task_groups (bsx_align.hip) cuts a run of tasks into the groups of k_hscan_same.  Host and device: tests/harness/groups_check.cpp
// drives the same function on the CPU.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// A run: the tasks of one window (first entry, length, flags, tag filter) whose read offsets sub_h are congruent mod 32, sorted by offset as a signed number.
// off[i * stride] is task i's offset with the sign bit turned (unsigned order = signed order), ascending.  A group's frame is the smallest offset still pending, its
// members are the next tasks of the run — so a group is a piece of the sorted run, its rows sorted by d = (offset - frame) / 32 with a task of the frame itself at
// row 0 — with offset - frame in {0, 32, .., 32 D}, at most Rg of them.  The N tasks that the frame could hold are not cut into full groups and a rest but into
// ceil(N / Rg) groups of sizes that differ by one at most: the turn takes ceil(N / ceil(N / Rg)) of them (70 tasks at Rg = 64 give 35 + 35, 65 give 33 + 32; the
// tasks left over are again a set of one frame, of one group fewer: N = G Rg - r with 0 <= r < Rg leaves (G - 1) Rg - (r - r / G)).  The same fetches, evener waves,
// and no set of two or more tasks leaves a group of one.
// Writes head[i * hstride] = size of the group that starts at task i and 0 for every other task; returns the number of groups.
// Termination: a turn's N counts task p itself, so N >= 1, 1 <= ceil(N / G) <= Rg, and p grows by at least one per turn: at most n turns; the search inside a turn
// halves [lo, hi) every step.
__host__ __device__ inline uint32_t bsx_group_cut(const uint32_t *off, uint32_t stride, uint32_t n, uint32_t D, uint32_t Rg, uint32_t *head, uint32_t hstride)
{
    if (Rg == 0) Rg = 1;
    uint32_t groups = 0;
    for (uint32_t p = 0; p < n; groups++) {
        const uint32_t frame = off[(size_t)p * stride];
        uint32_t lo = p + 1, hi = n;   // the first task beyond the frame's reach, in (p, n]
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (off[(size_t)mid * stride] - frame <= 32u * D) lo = mid + 1; else hi = mid;
        }
        const uint32_t N = lo - p, G = (N + Rg - 1u) / Rg, k = (N + G - 1u) / G;
        head[(size_t)p * hstride] = k;
        for (uint32_t j = 1; j < k; j++) head[(size_t)(p + j) * hstride] = 0;
        p += k;
    }
    return groups;
}
