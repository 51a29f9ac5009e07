// bsx_meth_tiles.h — how bsx_meth_regions cuts its intervals into tiles (bsx_meth.hip: k_meth_regions walks one tile per wave), and how meth_tiled
// cuts a call's intervals into launches and chooses each launch's block width.
// Plain C++, no HIP: tests/harness/tiles_check.cpp states the rules' properties on the CPU (tests/test_methratio_regions_cpu.py).
//
// An interval of `len` positions becomes ceil(len / TILE) tiles: [0, TILE), [TILE, 2 TILE), ..., the last one holding what is left.  The tiles of an
// interval are disjoint, cover it, and none is longer than TILE; an empty interval has no tile (its sums stay the zeroes they were set to).  A tile that
// is its interval's only one is marked `single`: its wave owns the interval's five cells and writes them with plain stores; the tiles of a longer
// interval add to the cells with atomics.  So no interval, whatever its length, is walked by one wave alone.
#pragma once
#include <cstddef>
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

// ---- the launches of a call (bsx_meth.hip: meth_tiled) ----
// Cuts n intervals of lens[i] positions (clipped: < 2^32 each) into launches [cut_at[q], cut_at[q + 1]) that partition [0, n) in order, none of them
// empty; cut_at starts with 0 and ends with n.  A launch takes intervals while it holds fewer than `chunk` intervals and fewer than `chunk` tiles: so it
// holds at most `chunk` intervals, its tiles without its last interval are fewer than `chunk`, and an interval of more tiles than `chunk` is still placed,
// alone or as its launch's last.  An empty interval has no tile: a launch may consist of nothing else.  chunk >= 1.
template <class Len>
inline std::vector<uint32_t> launches(uint32_t n, const Len &lens, size_t chunk)
{
    std::vector<uint32_t> cut_at(1, 0);
    for (uint32_t a = 0; a < n;) {
        uint32_t b = a;
        size_t nt = 0;
        while (b < n && (size_t)(b - a) < chunk && nt < chunk) nt += (size_t)n_tiles(lens(b)), b++;
        cut_at.push_back(b);
        a = b;
    }
    return cut_at;
}

// The launch of the intervals [a, b) takes the wide blocks where more than half of its tiles belong to intervals of LONG_TILES tiles and more.
constexpr uint32_t LONG_TILES = 64;
template <class Len>
inline bool wide(uint32_t a, uint32_t b, const Len &lens)
{
    size_t n_long = 0, n_all = 0;
    for (uint32_t i = a; i < b; i++) { const size_t k = (size_t)n_tiles(lens(i)); n_all += k; if (k >= LONG_TILES) n_long += k; }
    return 2 * n_long > n_all;
}

}  // namespace bsx_meth_tiles
