// Test harness (ours): the rule by which bsx_meth_regions cuts an interval into tiles (bsmap_amd/csrc/bsx_meth_tiles.h), on the CPU.
//   tiles_check <len> [<len> ...]
//       first line "tile T"; then per length, as interval number 7, 8, ..: "interval <iv> len <len> tiles <n> formula <n_tiles(len)>" and one line
//       "<iv> <off> <len> <single 0|1>" per tile, in the order cut() appends them
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../bsmap_amd/csrc/bsx_meth_tiles.h"

namespace T = bsx_meth_tiles;

int main(int argc, char **argv)
{
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
