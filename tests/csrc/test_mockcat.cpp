// Host run of heracles_amd/csrc/hx_mockcat.h, the code the kernels of hx_mockcat.hip run.  Reads one request per line from stdin and
// answers each on one line of stdout; tests/test_mockcat_host.py compares the answers with tests/mockcat_reference.py.
//   c <lam as hex double> <pixel> <realisation> <seed>             ->  the count
//   p <nside> <pixel> <index> <realisation> <seed>                 ->  lon lat (17 significant digits)
//   x <nside> <pixel>                                              ->  face ix iy
//   v <pixel> <index> <column> <realisation> <seed>                ->  the noise normal
// g++ -O2 -std=c++17 tests/csrc/test_mockcat.cpp
#include <cinttypes>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../../heracles_amd/csrc/hx_mockcat.h"

int main()
{
    char line[256];
    while (std::fgets(line, sizeof line, stdin)) {
        char lamtext[64];
        long long nside, pixel, index, column;
        unsigned long long realisation, seed;
        if (std::sscanf(line, "c %63s %lld %llu %llu", lamtext, &pixel, &realisation, &seed) == 4) {
            const double lam = std::strtod(lamtext, nullptr);
            if (!hxmock::lambda_valid(lam)) {
                std::printf("invalid\n");
                continue;
            }
            std::printf("%lld\n", hxmock::poisson_count(lam, (uint32_t)pixel, (uint32_t)realisation, (uint32_t)(seed & 0xffffffffull), (uint32_t)(seed >> 32)));
        } else if (std::sscanf(line, "p %lld %lld %lld %llu %llu", &nside, &pixel, &index, &realisation, &seed) == 5) {
            double lon, lat;
            hxmock::point_lonlat(nside, (uint32_t)pixel, (uint32_t)index, (uint32_t)realisation, (uint32_t)(seed & 0xffffffffull), (uint32_t)(seed >> 32), &lon, &lat);
            std::printf("%.17g %.17g\n", lon, lat);
        } else if (std::sscanf(line, "x %lld %lld", &nside, &pixel) == 2) {
            int face;
            long long ix, iy;
            hxmock::ring2xyf(nside, pixel, &face, &ix, &iy);
            std::printf("%d %lld %lld\n", face, ix, iy);
        } else if (std::sscanf(line, "v %lld %lld %lld %llu %llu", &pixel, &index, &column, &realisation, &seed) == 5) {
            std::printf("%.17g\n", hxmock::value_noise((uint32_t)pixel, (uint32_t)index, (uint32_t)column, (uint32_t)realisation, (uint32_t)(seed & 0xffffffffull),
                                                      (uint32_t)(seed >> 32)));
        } else {
            std::printf("?\n");
            return 2;
        }
    }
    return 0;
}
