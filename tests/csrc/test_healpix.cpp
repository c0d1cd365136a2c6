// Host run of heracles_amd/csrc/hx_healpix.h, the pixel geometry every kernel shares.  Reads one request per line from stdin and
// answers each on one line of stdout; tests/test_healpix_host.py compares the answers with the references of the tests.  <pixels> is
// the word "all" or a list of pixels; the answer holds the numbers of every pixel one after the other.
//   p <nside> <pixels>   ->  ir j first n face ix iy back: pix2ring, first and n of ring_info(ir), ring2xyf, xyf2ring of that
//   n <order> <pixels>   ->  ring2nest(p) nest2ring(p)
//   v <nside> <pixels>   ->  x y z of pix2vec_ring (17 significant digits)
//   q <values>           ->  isqrt_ll
// g++ -O2 -std=c++17 tests/csrc/test_healpix.cpp
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../heracles_amd/csrc/hx_healpix.h"

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd, tok;
        long long first = 0;
        std::vector<long long> pix;
        in >> cmd;
        if (cmd != "q") in >> first;  // nside, or the order
        while (in >> tok) {
            if (tok == "all" && cmd != "q") {
                const long long nside = cmd == "n" ? 1ll << first : first;
                for (long long p = 0; p < 12 * nside * nside; ++p) pix.push_back(p);
            } else {
                pix.push_back(std::stoll(tok));
            }
        }
        for (const long long p : pix) {
            if (cmd == "p") {
                long long ir, j, ix, iy;
                int face;
                hxpix::pix2ring(first, p, &ir, &j);
                const hxpix::Ring r = hxpix::ring_info(first, ir);
                hxpix::ring2xyf(first, p, &face, &ix, &iy);
                std::printf("%lld %lld %lld %lld %d %lld %lld %lld ", ir, j, r.first, r.n, face, ix, iy, hxpix::xyf2ring(first, face, ix, iy));
            } else if (cmd == "n") {
                std::printf("%lld %lld ", hxpix::ring2nest((int)first, p), hxpix::nest2ring((int)first, p));
            } else if (cmd == "v") {
                double x, y, z;
                hxpix::pix2vec_ring(first, p, &x, &y, &z);
                std::printf("%.17g %.17g %.17g ", x, y, z);
            } else if (cmd == "q") {
                std::printf("%lld ", hxpix::isqrt_ll(p));
            } else {
                std::printf("?\n");
                return 2;
            }
        }
        std::printf("\n");
    }
    return 0;
}
