// hx_mix_tiles.h -- the order in which the symmetric mixing-matrix product (launch_gemm_sym, hx_gemm.h) visits its block tiles.
// Host code without HIP headers: tests/csrc/test_mix_tiles.cpp pins it.
#pragma once
#include <algorithm>
#include <vector>

namespace hx {

struct MixTile {
    int x, y;  // row block <= column block; (-1, -1) = padding entry (the layout of int2)
};

// The tiles (i <= j) of the upper triangle of nb x nb row blocks.  Work-groups go to the 8 XCDs round-robin (blockIdx % 8), and an
// XCD runs 64 of them at a time (32 CUs x 2).  The upper triangle is cut into super-tiles of 8 x 4 block tiles (12 row blocks of T
// for 32 tiles), the super-tiles are dealt to the XCDs (largest first, to the least loaded) and every XCD walks its own list: the tiles
// that run side by side on an XCD share their rows of T through its L2 instead of each streaming 2 x 9.5 MB from memory.
// (-1, -1) pads the shorter lists.
inline std::vector<MixTile> mix_tile_order(int nb)
{
    constexpr int SR = 8, SC = 4, NX = 8;
    std::vector<std::vector<MixTile>> supers;
    for (int I = 0; I < nb; I += SR)
        for (int J = I / SC * SC; J < nb; J += SC) {
            std::vector<MixTile> m;
            for (int i = I; i < std::min(I + SR, nb); ++i)
                for (int j = std::max(J, i); j < std::min(J + SC, nb); ++j) m.push_back(MixTile{i, j});
            if (!m.empty()) supers.push_back(m);
        }
    std::stable_sort(supers.begin(), supers.end(), [](const std::vector<MixTile> &a, const std::vector<MixTile> &b) { return a.size() > b.size(); });
    std::vector<std::vector<MixTile>> per(NX);
    for (const auto &m : supers) {
        int x = 0;
        for (int q = 1; q < NX; ++q)
            if (per[q].size() < per[x].size()) x = q;
        per[x].insert(per[x].end(), m.begin(), m.end());
    }
    size_t longest = 0;
    for (const auto &l : per) longest = std::max(longest, l.size());
    std::vector<MixTile> tiles(longest * NX, MixTile{-1, -1});
    for (int x = 0; x < NX; ++x)
        for (size_t k = 0; k < per[x].size(); ++k) tiles[k * NX + x] = per[x][k];
    return tiles;
}

}  // namespace hx
