// bsx_meth_tiles.h — how bsx_meth_regions cuts its intervals into tiles (bsx_meth.hip: k_meth_regions walks one tile per wave).
// Plain C++, no HIP: tests/harness/tiles_check.cpp states the rule's properties on the CPU (tests/test_methratio_regions_cpu.py).
//
// An interval of `len` positions becomes ceil(len / TILE) tiles: [0, TILE), [TILE, 2 TILE), ..., the last one holding what is left.  The tiles of an
// interval are disjoint, cover it, and none is longer than TILE; an empty interval has no tile (its sums stay the zeroes they were set to).  A tile that
// is its interval's only one is marked `single`: its wave owns the interval's five cells and writes them with plain stores; the tiles of a longer
// interval add to the cells with atomics.  So no interval, whatever its length, is walked by one wave alone.
#pragma once
#include <cstdint>
#include <vector>

namespace bsx_meth_tiles {

constexpr uint32_t TILE = 2048;                 // positions per tile: 32 strides of a 64-lane wave
constexpr uint32_t SINGLE = 0x80000000u;        // flag in Tile::len

struct Tile {
    uint32_t iv;    // index of the interval (within the launch)
    uint32_t off;   // first position of the tile, counted from the interval's start
    uint32_t len;   // 1..TILE positions; | SINGLE when the interval has no other tile
};

inline uint64_t n_tiles(uint64_t len) { return (len + TILE - 1) / TILE; }

// appends the tiles of interval `iv` of `len` positions (len < 2^32: coordinates are 32-bit)
inline void cut(uint32_t iv, uint64_t len, std::vector<Tile> &out)
{
    if (len <= TILE) {
        if (len) out.push_back(Tile{iv, 0, (uint32_t)len | SINGLE});
        return;
    }
    for (uint64_t off = 0; off < len; off += TILE) out.push_back(Tile{iv, (uint32_t)off, (uint32_t)(len - off < TILE ? len - off : TILE)});
}

}  // namespace bsx_meth_tiles
