// The tile order of the symmetric mixing-matrix product (hx_mix_tiles.h), on the host.
// Build: g++ -O2 -std=c++17 test_mix_tiles.cpp
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../../heracles_amd/csrc/hx_mix_tiles.h"
using hx::MixTile;

static int failures = 0;
#define CHECK(cond, ...)                      \
    do {                                      \
        if (!(cond)) {                        \
            ++failures;                       \
            printf("FAIL nb %d: ", nb);       \
            printf(__VA_ARGS__);              \
            printf(" (%s)\n", #cond);         \
        }                                     \
    } while (0)

// FNV-1a over the entries in order, x then y, four bytes each from the low one
static uint64_t fnv1a64(const std::vector<MixTile> &tiles)
{
    uint64_t h = 0xcbf29ce484222325ULL;
    for (const MixTile &t : tiles)
        for (int v : {t.x, t.y})
            for (int s = 0; s < 32; s += 8) h = (h ^ (((uint32_t)v >> s) & 0xff)) * 0x100000001b3ULL;
    return h;
}

static void check(int nb)
{
    constexpr int NX = 8, SUPER = 32;  // XCDs; tiles of the largest super-tile (8 x 4)
    const std::vector<MixTile> tiles = hx::mix_tile_order(nb);
    CHECK(tiles.size() % NX == 0, "%zu entries", tiles.size());
    std::vector<int> seen((size_t)nb * nb, 0);
    int real[NX] = {0}, bad = 0;
    bool padded[NX] = {false};
    for (size_t e = 0; e < tiles.size(); ++e) {
        const int i = tiles[e].x, j = tiles[e].y, x = (int)(e % NX);
        if (i == -1 && j == -1) {
            padded[x] = true;
            continue;
        }
        if (!(0 <= i && i <= j && j < nb)) {
            ++bad;
            continue;
        }
        ++seen[(size_t)i * nb + j];
        ++real[x];
        CHECK(!padded[x], "entry %zu (%d, %d) of XCD %d stands behind a padding entry", e, i, j, x);
    }
    CHECK(bad == 0, "%d entries are neither a tile of the upper triangle nor (-1, -1)", bad);
    for (int i = 0; i < nb; ++i)
        for (int j = i; j < nb; ++j) CHECK(seen[(size_t)i * nb + j] == 1, "tile (%d, %d) occurs %d times", i, j, seen[(size_t)i * nb + j]);
    int lo = real[0], hi = real[0];
    for (int x = 1; x < NX; ++x) {
        lo = real[x] < lo ? real[x] : lo;
        hi = real[x] > hi ? real[x] : hi;
    }
    CHECK(hi - lo <= SUPER, "the XCDs' lists hold %d to %d tiles", lo, hi);
}

// the order itself, recorded from the loop as it stood inside mix_ctx_init (hx_mixmat.hip) before it became a function: it decides which
// tiles share their rows through an XCD's L2, so a change would be a silent change of speed
static void check_order(int nb, size_t entries, uint64_t hash)
{
    const std::vector<MixTile> tiles = hx::mix_tile_order(nb);
    CHECK(tiles.size() == entries, "%zu entries, recorded %zu", tiles.size(), entries);
    CHECK(fnv1a64(tiles) == hash, "hash 0x%016llx, recorded 0x%016llx", (unsigned long long)fnv1a64(tiles), (unsigned long long)hash);
}

int main()
{
    for (int nb : {1, 2, 3, 4, 5, 8, 9, 12, 33, 49}) check(nb);
    check_order(9, 208, 0x5270fec3313d307dULL);
    check_order(49, 1248, 0xe28ca4304f2dbb4dULL);  // (L = 6144: 1225 tiles)
    printf(failures ? "%d FAILURES\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
