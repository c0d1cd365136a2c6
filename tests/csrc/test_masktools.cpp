// Host run of heracles_amd/csrc/hx_masktools.h, the code hx_masktools.hip runs.  Reads one request per line from stdin and answers
// each on one line of stdout; tests/test_masktools_host.py compares the answers with tests/masktools_reference.py.  Doubles travel as
// hex floats in both directions.
//   B <nside>                                      ->  the number of pixels whose ring_vec(ring_info(pix2ring)) is not, bit for bit,
//                                                      pix2vec_ring, or whose ring does not hold them (0 is right)
//   h <ux uy uz vx vy vz>                          ->  chord_h
//   a <degrees>                                    ->  angle_h
//   w <nside> <lon> <lat> <radius>                 ->  lo hi, then k0 count for each ring lo .. hi: the rings and windows of the disc
//   d <nside> <ndisc> <lon lat radius> ...         ->  the pixels the discs clear (ascending), by rings, windows and the rule
//   s <nside> <max_distance> <count> <pixels> ...  ->  H of every pixel for the mask with these pixels masked, then ';', then the
//                                                      number of h evaluations of every pixel
//   t <kind> <x>                                   ->  taper(kind, x)
//   T <kind> <H> <hcap>                            ->  taper_of_h
// g++ -O2 -std=c++17 tests/csrc/test_masktools.cpp
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../heracles_amd/csrc/hx_masktools.h"

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd, tok;
        in >> cmd;
        std::vector<double> x;
        while (in >> tok) x.push_back(std::strtod(tok.c_str(), nullptr));
        if (cmd == "B" && x.size() == 1) {
            const long long nside = (long long)x[0], npix = 12 * nside * nside;
            long long bad = 0;
            for (long long p = 0; p < npix; ++p) {
                long long ir, j;
                double a[3], b[3];
                hxmask::pix2ring(nside, p, &ir, &j);
                const hxmask::Ring r = hxmask::ring_info(nside, ir);
                hxmask::ring_vec(r, j, &a[0], &a[1], &a[2]);
                hxjk::pix2vec_ring(nside, p, &b[0], &b[1], &b[2]);
                if (ir < 1 || ir > 4 * nside - 1 || j < 0 || j >= r.n || r.first + j != p || !same_bits(a[0], b[0]) || !same_bits(a[1], b[1]) || !same_bits(a[2], b[2])) ++bad;
            }
            std::printf("%lld\n", bad);
        } else if (cmd == "h" && x.size() == 6) {
            std::printf("%a\n", hxmask::chord_h(x[0], x[1], x[2], x[3], x[4], x[5]));
        } else if (cmd == "a" && x.size() == 1) {
            std::printf("%a\n", hxmask::angle_h(x[0]));
        } else if (cmd == "w" && x.size() == 4) {
            const long long nside = (long long)x[0];
            const hxmask::Disc d = hxmask::make_disc(x[1], x[2], x[3]);
            long long lo, hi;
            hxmask::disc_rings(nside, d, &lo, &hi);
            std::printf("%lld %lld", lo, hi);
            for (long long ir = lo; ir <= hi; ++ir) {
                const hxmask::Window w = hxmask::disc_window(hxmask::ring_info(nside, ir), d);
                std::printf(" %lld %lld", w.k0, w.count);
            }
            std::printf("\n");
        } else if (cmd == "d" && x.size() >= 2 && x.size() == 2 + 3 * (size_t)x[1]) {
            const long long nside = (long long)x[0], npix = 12 * nside * nside;
            std::vector<char> hit((size_t)npix, 0);
            for (size_t k = 0; k < (size_t)x[1]; ++k) {
                if (!hxmask::disc_valid(x[2 + 3 * k], x[3 + 3 * k], x[4 + 3 * k])) {
                    std::printf("invalid %zu\n", k);
                    return 3;
                }
                const hxmask::Disc d = hxmask::make_disc(x[2 + 3 * k], x[3 + 3 * k], x[4 + 3 * k]);
                long long lo, hi;
                hxmask::disc_rings(nside, d, &lo, &hi);
                for (long long ir = lo; ir <= hi; ++ir) {
                    const hxmask::Ring r = hxmask::ring_info(nside, ir);
                    const hxmask::Window w = hxmask::disc_window(r, d);
                    for (long long i = 0; i < w.count; ++i) {
                        const long long j = hxmask::wrap_index(w.k0 + i, r.n);
                        if (hxmask::disc_hit(r, j, d)) hit[(size_t)(r.first + j)] = 1;
                    }
                }
            }
            for (long long p = 0; p < npix; ++p)
                if (hit[(size_t)p]) std::printf("%lld ", p);
            std::printf("\n");
        } else if (cmd == "s" && x.size() >= 3 && x.size() == 3 + (size_t)x[2]) {
            const long long nside = (long long)x[0], npix = 12 * nside * nside;
            std::vector<double> mask((size_t)npix, 1.0);
            for (size_t k = 0; k < (size_t)x[2]; ++k) mask[(size_t)x[3 + k]] = 0.0;
            std::vector<uint32_t> left((size_t)npix), right((size_t)npix), first((size_t)(4 * nside)), last((size_t)(4 * nside));
            first[0] = last[0] = hxmask::NONE;
            for (long long ir = 1; ir <= 4 * nside - 1; ++ir)
                hxmask::ring_neighbours(mask.data(), hxmask::ring_info(nside, ir), left.data(), right.data(), &first[(size_t)ir], &last[(size_t)ir]);
            const hxmask::Neighbours nb = {left.data(), right.data(), first.data(), last.data()};
            const double cap = hxmask::angle_h(x[1]);
            std::vector<unsigned long long> evals((size_t)npix, 0);
            for (long long p = 0; p < npix; ++p)
                std::printf("%a ", hxmask::is_masked(mask[(size_t)p]) ? 0.0 : hxmask::nearest_h(nside, p, cap, nb, &evals[(size_t)p]));
            std::printf(";");
            for (long long p = 0; p < npix; ++p) std::printf(" %llu", evals[(size_t)p]);
            std::printf("\n");
        } else if (cmd == "t" && x.size() == 2) {
            std::printf("%a\n", hxmask::taper((int)x[0], x[1]));
        } else if (cmd == "T" && x.size() == 3) {
            std::printf("%a\n", hxmask::taper_of_h((int)x[0], x[1], x[2]));
        } else {
            std::printf("?\n");
            return 2;
        }
    }
    return 0;
}
