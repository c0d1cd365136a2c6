"""The checker behind tests/test_gpu_mixmat_spin.py, pinned for spin weights other than 0 and 2: the oracle's 3j recursion at
l ~ 4096 against the exact big-integer Racah sum, and its mixing matrices against sympy's exact 3j symbols.  No GPU."""

import numpy as np


def _racah_3j(j1, j2, j3, m1, m2):
    """Exact Wigner 3j (j1 j2 j3; m1 m2 -(m1+m2)) from Racah's single sum as an alternating sum of products of three binomials
    (exact big integers), rounded once at the end (50 digits); restated from tests/test_oracle_golden.py."""
    from math import comb

    import mpmath

    m3 = -(m1 + m2)
    if j3 < abs(j1 - j2) or j3 > j1 + j2 or abs(m1) > j1 or abs(m2) > j2 or abs(m3) > j3:
        return 0.0
    a, b, c = j1 + j2 - j3, j1 - j2 + j3, -j1 + j2 + j3
    k0 = max(0, j2 - j3 - m1, j1 - j3 + m2)
    k1 = min(a, j1 - m1, j2 + m2)
    S = 0
    A, B, Cc = comb(a, k0), comb(b, j1 - m1 - k0), comb(c, j2 + m2 - k0)
    for k in range(k0, k1 + 1):
        t = A * B * Cc
        S += -t if k & 1 else t
        if k < k1:
            A = A * (a - k) // (k + 1)
            n = j1 - m1 - k
            B = B * n // (b - n + 1)
            n = j2 + m2 - k
            Cc = Cc * n // (c - n + 1)
    with mpmath.workdps(50):
        F = mpmath.factorial
        sq = (F(j1 + m1) * F(j1 - m1) * F(j2 + m2) * F(j2 - m2) * F(j3 + m3) * F(j3 - m3)) / (F(j1 + j2 + j3 + 1) * F(a) * F(b) * F(c))
        v = mpmath.sqrt(sq) * mpmath.mpf(abs(S))
        sign = (-1 if (j1 - j2 - m3) & 1 else 1) * (-1 if S < 0 else 1)
        return float(sign * v)


def test_racah_restatement_agrees_with_sympy():
    from sympy import N
    from sympy.physics.wigner import wigner_3j

    for j1, j2, j3, m1, m2 in [(3, 3, 2, 1, -1), (12, 9, 7, 3, -3), (30, 28, 11, -1, 1), (25, 31, 6, 3, -3), (17, 17, 1, 1, -1)]:
        ref = float(N(wigner_3j(j1, j2, j3, m1, m2, -(m1 + m2)), 30))
        assert abs(_racah_3j(j1, j2, j3, m1, m2) - ref) <= 1e-15 * max(1.0, abs(ref))


def test_wigner3j_recursion_for_other_spins_at_lmax4096(oracle):
    """The bound of test_oracle_golden.py::test_wigner3j_recursion_at_config4_and_bench_sizes (5e-13 of the largest symbol of the
    l3 range) for the magnetic numbers of spin-1 and spin-3 fields, where the blocks of the L = 4096 GPU test lie."""
    worst = 0.0
    for l1, l2 in [(4096, 4096), (4096, 3896), (4073, 2048), (4096, 3), (4091, 37)]:
        lo, hi = abs(l1 - l2), l1 + l2
        picks = sorted({lo, lo + 1, (lo + hi) // 2, (lo + hi) // 2 + 1, min(hi, 4096) - 1, min(hi, 4096), hi})
        for m1, m2 in ((1, -1), (3, -3), (-1, 1)):
            jmin, w = oracle.wigner3j_l3(l1, l2, m1, m2)
            scale = np.abs(w).max()
            for l3 in picks:
                if l3 < jmin:
                    continue
                worst = max(worst, abs(w[l3 - jmin] - _racah_3j(l1, l2, l3, m1, m2)) / scale)
    print("worst 3j error / largest symbol:", worst)
    assert worst < 5e-13, worst


def test_oracle_mixmat_other_spins_vs_sympy(oracle):
    """oracle.mixmat(cl, spin=(s1, s2)) = (2 l2 + 1)/(4 pi) sum_l3 (2 l3 + 1) W_l3 (l1 l2 l3; s1 -s1 0)(l1 l2 l3; s2 -s2 0) at L = 16:
    every element with the exact Racah sum above, the rows 1, 3, 4, 10 and 16 also with sympy's symbols (a second a symbol each:
    all rows would take 15 s)."""
    from sympy import N
    from sympy.physics.wigner import wigner_3j

    L = 16
    rng = np.random.default_rng(16)
    cl = rng.uniform(0.5, 1.5, L + 1) / (1 + np.arange(L + 1)) ** 2
    w3 = {}

    def w(exact, l1, l2, l3, m):
        if l1 < abs(m) or l2 < abs(m):
            return 0.0
        key = (exact, l1, l2, l3, m)
        if key not in w3:
            w3[key] = _racah_3j(l1, l2, l3, m, -m) if exact == "racah" else float(N(wigner_3j(l1, l2, l3, m, -m, 0), 30))
        return w3[key]

    for s1, s2 in [(0, 1), (1, -1), (3, -2)]:
        got = oracle.mixmat(cl, spin=(s1, s2))
        for exact, rows in (("racah", range(L + 1)), ("sympy", (1, 3, 4, 10, 16))):
            for l1 in rows:
                ref = np.zeros(L + 1)
                for l2 in range(L + 1):
                    for l3 in range(abs(l1 - l2), min(l1 + l2, L) + 1):
                        ref[l2] += (2 * l2 + 1) / (4 * np.pi) * (2 * l3 + 1) * cl[l3] * w(exact, l1, l2, l3, s1) * w(exact, l1, l2, l3, s2)
                assert l1 < max(abs(s1), abs(s2)) or np.abs(ref).max() > 0
                # (<= 17 terms, a few roundings of 1.1e-16 each)
                np.testing.assert_allclose(got[l1], ref, rtol=0, atol=4e-15 * max(1.0, np.abs(got).max()), err_msg=str((s1, s2, exact, l1)))
