// Host run of heracles_amd/csrc/hx_jkregions.h, the code hx_jkregions.hip runs.  Reads one request per line from stdin and answers
// each on one line of stdout; tests/test_jkregions_host.py compares the answers with tests/jkregions_reference.py.
//   q <w as hex double> <wmax as hex double>       ->  the integer weight
//   k <t as hex double>                            ->  the 64-bit order key
//   t <Q> <n1> <n>                                 ->  floor(Q n1 / n)
//   g <E> <q> <T>                                  ->  1 if the pixel goes left, else 0
//   c <count> <m> <n1> <n>                         ->  the clamped count
//   v <nside> <pixel>                              ->  x y z of the pixel centre (17 significant digits)
//   e <xx> <xy> <xz> <yy> <yz> <zz> (hex doubles)  ->  the principal axis
//   m <ten moments as hex doubles>                 ->  the six covariance entries
// g++ -O2 -std=c++17 tests/csrc/test_jkregions.cpp
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../heracles_amd/csrc/hx_jkregions.h"

static int doubles(const char *text, double *out, int n)
{
    char *end;
    for (int k = 0; k < n; ++k) {
        out[k] = std::strtod(text, &end);
        if (end == text) return k;
        text = end;
    }
    return n;
}

int main()
{
    char line[1024];
    while (std::fgets(line, sizeof line, stdin)) {
        unsigned long long a, b, c, d;
        long long nside, pixel;
        double x[10];
        if (line[0] == 'q' && doubles(line + 1, x, 2) == 2) {
            std::printf("%" PRIu64 "\n", hxjk::quantise(x[0], x[1]));
        } else if (line[0] == 'k' && doubles(line + 1, x, 1) == 1) {
            std::printf("%" PRIu64 "\n", hxjk::order_key(x[0]));
        } else if (std::sscanf(line, "t %llu %llu %llu", &a, &b, &c) == 3) {
            std::printf("%" PRIu64 "\n", hxjk::split_target(a, (uint32_t)b, (uint32_t)c));
        } else if (std::sscanf(line, "g %llu %llu %llu", &a, &b, &c) == 3) {
            std::printf("%d\n", hxjk::goes_left(a, b, c) ? 1 : 0);
        } else if (std::sscanf(line, "c %llu %llu %llu %llu", &a, &b, &c, &d) == 4) {
            std::printf("%u\n", hxjk::clamp_count((uint32_t)a, (uint32_t)b, (uint32_t)c, (uint32_t)d));
        } else if (std::sscanf(line, "v %lld %lld", &nside, &pixel) == 2) {
            hxjk::pix2vec_ring(nside, pixel, &x[0], &x[1], &x[2]);
            std::printf("%.17g %.17g %.17g\n", x[0], x[1], x[2]);
        } else if (line[0] == 'e' && doubles(line + 1, x, 6) == 6) {
            double axis[3];
            hxjk::principal_axis(x, axis);
            std::printf("%.17g %.17g %.17g\n", axis[0], axis[1], axis[2]);
        } else if (line[0] == 'm' && doubles(line + 1, x, 10) == 10) {
            double C[6];
            hxjk::covariance(x, C);
            std::printf("%.17g %.17g %.17g %.17g %.17g %.17g\n", C[0], C[1], C[2], C[3], C[4], C[5]);
        } else {
            std::printf("?\n");
            return 2;
        }
    }
    return 0;
}
