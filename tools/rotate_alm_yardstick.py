#!/usr/bin/env python3
"""The FP64 yardstick of DESIGN.md 4.18 on the CPU: the upward recurrence of rotate_alm with float64 chains against the same in long
double (tests/rotation_reference.py), per (lmax, theta, column m), as a fraction of max |a'| of the column.  No GPU.

    python tools/rotate_alm_yardstick.py 2048 1.234:0,1024 0.02:0,1,1024,1900 1e-3:2
    python tools/rotate_alm_yardstick.py 6144 --lmin 6000 1.097:4096 0.02:4096 pi-1e-3:4096

An angle is a float or pi-<float>.  Input: random rows l >= lmin (zeros below), psi = 0.4, phi = -0.8."""

import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import rotation_reference as rr  # noqa: E402


def parse_angle(s):
    return float(np.pi - np.float64(s[3:])) if s.startswith("pi-") else float(s)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("lmax", type=int)
    ap.add_argument("cases", nargs="+", help="theta:m[,m...]")
    ap.add_argument("--lmin", type=int, default=0)
    args = ap.parse_args()
    psi, phi = 0.4, -0.8
    alm = rr.sparse_alm(np.random.default_rng(args.lmax), args.lmax, args.lmin)
    rows = rr.phased_rows(alm, args.lmax, psi, args.lmin)
    for case in args.cases:
        th, cols = case.split(":")
        theta = parse_angle(th)
        for m in (int(c) for c in cols.split(",")):
            t0 = time.time()
            ref = rr.rotate_column_ref(alm, args.lmax, m, psi, theta, phi, rows=rows)
            f64 = rr.rotate_column_ref(alm, args.lmax, m, psi, theta, phi, np.float64, rows=rows)
            err, scale = float(np.abs(f64 - ref).max()), float(np.abs(ref).max())
            print(f"lmax {args.lmax} theta {th} ({theta!r}) sin {np.sin(theta):.3e} m {m}: float64 chains - long double = {err / scale:.2e} of max |a'| = {scale:.3e}  ({time.time() - t0:.1f} s)", flush=True)


if __name__ == "__main__":
    main()
