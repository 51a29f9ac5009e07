// Test harness (ours): the rules of bsmap_amd/csrc/bsx_meth_tiles.h on the CPU: how bsx_meth_regions cuts an interval into tiles, how meth_tiled cuts a
// call's intervals into launches, and which launches take the wide blocks.
//   tiles_check <len> [<len> ...]
//       first line "tile T"; then per length, as interval number 7, 8, ..: "interval <iv> len <len> tiles <n> formula <n_tiles(len)>" and one line
//       "<iv> <off> <len> <single 0|1>" per tile, in the order cut() appends them
//   tiles_check launches <chunk> [<len> ...]
//       one line "launches <cut_at[0]> <cut_at[1]> ..": launches(n, lens, chunk) over the lengths as the intervals 0, 1, ..
//   tiles_check wide [<len> ...]
//       one line "wide <0|1>": wide(0, n, lens) of a launch that holds exactly these intervals
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../bsmap_amd/csrc/bsx_meth_tiles.h"

namespace T = bsx_meth_tiles;

int main(int argc, char **argv)
{
    const bool launches = argc > 2 && !strcmp(argv[1], "launches"), wide = argc > 1 && !strcmp(argv[1], "wide");
    if (launches || wide) {
        std::vector<unsigned long long> lens;
        for (int a = launches ? 3 : 2; a < argc; a++) lens.push_back(strtoull(argv[a], nullptr, 10));
        const auto len_of = [&](uint32_t i) { return lens.at(i); };  // (at: a rule that asks for an interval outside the list ends the program)
        if (wide) {
            printf("wide %d\n", T::wide(0, (uint32_t)lens.size(), len_of) ? 1 : 0);
            return 0;
        }
        printf("launches");
        for (const uint32_t c : T::launches((uint32_t)lens.size(), len_of, (size_t)strtoull(argv[2], nullptr, 10))) printf(" %u", c);
        printf("\n");
        return 0;
    }
    printf("tile %u\n", T::TILE);
    std::vector<T::Tile> all;
    for (int a = 1; a < argc; a++) {
        const unsigned long long len = strtoull(argv[a], nullptr, 10);
        const size_t at = all.size();
        T::cut((uint32_t)(6 + a), len, all);  // appended behind the earlier intervals' tiles, as the library does
        printf("interval %d len %llu tiles %zu formula %llu\n", 6 + a, len, all.size() - at, (unsigned long long)T::n_tiles(len));
        for (size_t i = at; i < all.size(); i++) printf("%u %u %u %d\n", all[i].iv, all[i].off, all[i].len & ~T::SINGLE, (all[i].len & T::SINGLE) ? 1 : 0);
    }
    return 0;
}
