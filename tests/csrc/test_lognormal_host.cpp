// Host run of heracles_amd/csrc/hx_lognormal.h, the scalar code k_cl_nearest_psd runs: the round-robin ordering meets every pair once
// per sweep, the rotation zeroes a_pq to rounding and is a rotation, and a sweep loop built from both diagonalises a matrix.
// g++ -O2 -std=c++17 tests/csrc/test_lognormal_host.cpp   (also built with -fsanitize=address,undefined)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../heracles_amd/csrc/hx_lognormal.h"

using namespace hxlogn;

static int fails = 0;
#define CHECK(cond)                                             \
    do {                                                        \
        if (!(cond)) {                                          \
            std::printf("FAIL line %d: %s\n", __LINE__, #cond); \
            ++fails;                                            \
        }                                                       \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static double uniform()  // splitmix64 -> (-1, 1)
{
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (double)(z >> 11) * 0x1p-52 - 1.0;
}

static void pairing(int n)
{
    std::vector<int> met((size_t)n * n, 0);
    const int steps = rr_steps(n), pairs = rr_pairs(n);
    CHECK(steps == (n % 2 ? n : n - 1) && pairs == (n + 1) / 2);
    for (int step = 0; step < steps; ++step) {
        std::vector<int> used((size_t)n, 0);
        int valid = 0;
        for (int k = 0; k < pairs; ++k) {
            int p = -1, q = -1;
            if (!rr_pair(n, step, k, &p, &q)) continue;
            ++valid;
            CHECK(0 <= p && p < q && q < n);
            if (!(0 <= p && p < q && q < n)) continue;
            ++met[(size_t)p * n + q];
            CHECK(used[p] == 0 && used[q] == 0);  // the pairs of a step are disjoint
            used[p] = used[q] = 1;
        }
        CHECK(valid == n / 2);
    }
    for (int p = 0; p < n; ++p)
        for (int q = p + 1; q < n; ++q) CHECK(met[(size_t)p * n + q] == 1);
}

static void rotation(double app, double aqq, double apq)
{
    const Rotation r = jacobi_rotation(app, aqq, apq);
    const long double c = r.c, s = r.s;
    CHECK(std::fabs((double)(c * c + s * s - 1.0L)) <= 2 * 0x1p-52);
    CHECK(std::fabs(r.t) <= 1.0 && r.c > 0.0);
    // a'_pq = (c^2 - s^2) a_pq + c s (a_pp - a_qq), in long double, against the size of the block
    const long double off = (c * c - s * s) * (long double)apq + c * s * ((long double)app - (long double)aqq);
    const double scale = std::fabs(app) + std::fabs(aqq) + std::fabs(apq);
    CHECK(std::fabs((double)off) <= 4 * 0x1p-52 * scale);
    // the diagonal the kernel writes is the rotated diagonal
    const long double pp = c * c * app - 2 * c * s * apq + s * s * aqq, qq = s * s * app + 2 * c * s * apq + c * c * aqq;
    CHECK(std::fabs((double)(pp - ((long double)app - (long double)r.t * apq))) <= 8 * 0x1p-52 * scale);
    CHECK(std::fabs((double)(qq - ((long double)aqq + (long double)r.t * apq))) <= 8 * 0x1p-52 * scale);
}

// the kernel's sweep on the host: A -> diagonal, V its eigenvectors; returns the sweeps used (-1: cap)
static int sweeps(int n, std::vector<double> &A, std::vector<double> &V)
{
    for (int sweep = 0; sweep < 40; ++sweep) {
        for (int step = 0; step < rr_steps(n); ++step)
            for (int k = 0; k < rr_pairs(n); ++k) {
                int p, q;
                if (!rr_pair(n, step, k, &p, &q)) continue;
                const double app = A[(size_t)p * n + p], aqq = A[(size_t)q * n + q], apq = A[(size_t)p * n + q];
                const Rotation r = jacobi_rotation(app, aqq, apq);
                for (int j = 0; j < n; ++j) {
                    const double x = A[(size_t)p * n + j], y = A[(size_t)q * n + j];
                    A[(size_t)p * n + j] = r.c * x - r.s * y;
                    A[(size_t)q * n + j] = r.s * x + r.c * y;
                }
                for (int i = 0; i < n; ++i) {
                    const double x = A[(size_t)i * n + p], y = A[(size_t)i * n + q];
                    A[(size_t)i * n + p] = r.c * x - r.s * y;
                    A[(size_t)i * n + q] = r.s * x + r.c * y;
                    const double u = V[(size_t)i * n + p], w = V[(size_t)i * n + q];
                    V[(size_t)i * n + p] = r.c * u - r.s * w;
                    V[(size_t)i * n + q] = r.s * u + r.c * w;
                }
                if (apq != 0.0) {
                    A[(size_t)p * n + p] = app - r.t * apq;
                    A[(size_t)q * n + q] = aqq + r.t * apq;
                    A[(size_t)p * n + q] = A[(size_t)q * n + p] = 0.0;
                }
            }
        double off = 0.0;
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j)
                if (i != j) off = std::fmax(off, std::fabs(A[(size_t)i * n + j]));
        if (off <= 0x1p-50) return sweep + 1;
    }
    return -1;
}

static void diagonalise(int n)
{
    // a correlation-like matrix with an indefinite direction: unit diagonal, off-diagonals in (-1, 1)
    std::vector<double> A((size_t)n * n), A0, V((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i) {
        V[(size_t)i * n + i] = 1.0;
        A[(size_t)i * n + i] = 1.0;
        for (int j = i + 1; j < n; ++j) A[(size_t)i * n + j] = A[(size_t)j * n + i] = 0.9 * uniform();
    }
    A0 = A;
    const int used = sweeps(n, A, V);
    CHECK(used > 0);
    std::printf("n = %d: %d sweeps\n", n, used);
    // V L V^T = A0 and V^T V = 1 to rounding
    double worst = 0.0, orth = 0.0;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            long double s = 0.0L, o = 0.0L;
            for (int k = 0; k < n; ++k) {
                s += (long double)V[(size_t)i * n + k] * A[(size_t)k * n + k] * V[(size_t)j * n + k];
                o += (long double)V[(size_t)k * n + i] * V[(size_t)k * n + j];
            }
            worst = std::fmax(worst, std::fabs((double)(s - A0[(size_t)i * n + j])));
            orth = std::fmax(orth, std::fabs((double)(o - (i == j ? 1.0L : 0.0L))));
        }
    CHECK(worst <= 1e-13 * n);
    CHECK(orth <= 1e-13 * n);
}

int main()
{
    for (int n : {1, 2, 3, 7, 64}) pairing(n);
    for (int n = 4; n <= 33; ++n) pairing(n);

    rotation(1.0, 1.0, 0.5);     // tau = 0: t = 1
    rotation(1.0, 2.0, 1e-300);  // tau overflows towards t = 0
    rotation(2.0, 1.0, -1e-17);
    rotation(-3.0, 5.0, 4.0);
    rotation(1.0, 1.0 + 0x1p-52, 0x1p-30);
    for (int i = 0; i < 20000; ++i) {
        const double scale = std::ldexp(1.0, (int)(20 * uniform()));
        rotation(scale * uniform(), scale * uniform(), scale * uniform() * std::ldexp(1.0, (int)(-30 * std::fabs(uniform()))));
    }
    const Rotation id = jacobi_rotation(1.0, 2.0, 0.0);
    CHECK(id.c == 1.0 && id.s == 0.0 && id.t == 0.0);

    for (int n : {2, 3, 7, 33, 64}) diagonalise(n);

    if (fails) return 1;
    std::printf("ok\n");
    return 0;
}
