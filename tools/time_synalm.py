"""hx_synalm at production size: spectra and alms resident in HBM, lmax 6144 (env LMAX), N = 1, 6 and 30 components (env NCOMPS).

Per N: the whole call (factor + flag read-back + generator) by the library's event timer, the generator kernel alone from the
library's `synalm` scope in calls of their own, the factor alone (hx_cl_cholesky into a device array); each warmed up, median and
min .. max of REPS.  The generator's store rate (16 N bytes per coefficient over its kernel time) is set against the copy probe of
hx_measure_peaks (which counts read + write bytes: a store-only kernel is compared with half of it and with the whole), and its draw
rate against the FP64 vector rate.  Results as JSON in OUT (default profiles/synalm.json).  DESIGN.md 4.15."""

import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

import heracles_amd as hx
from heracles_amd import _lib
from heracles_amd.mocks import TILE_COMP, TILE_COMP_SMALL, TILE_M

LMAX = int(os.environ.get("LMAX", "6144"))
NCOMPS = [int(x) for x in os.environ.get("NCOMPS", "1,6,30").split(",")]
REPS = int(os.environ.get("REPS", "7"))
OUT = os.environ.get("OUT", "profiles/synalm.json")


def spectra(ncomp, lmax):
    """C_l = B_l B_l^T / (l + 1)^2, packed (on the host once, then resident)."""
    rng = np.random.default_rng(ncomp)
    B = rng.standard_normal((lmax + 1, ncomp, ncomp + 2))
    C = np.einsum("lik,ljk->ijl", B, B) / (np.arange(lmax + 1) + 1.0) ** 2
    return np.ascontiguousarray(C[np.triu_indices(ncomp)])


def summary(xs):
    return {"median_ms": statistics.median(xs), "min_ms": min(xs), "max_ms": max(xs)}


def main():
    hx.init(0)
    L = _lib.load()
    peaks = _lib.measure_peaks()
    print("peaks:", peaks, flush=True)
    nlm = (LMAX + 1) * (LMAX + 2) // 2
    rows = []
    for n in NCOMPS:
        cl = torch.from_numpy(spectra(n, LMAX)).cuda()
        alms = torch.empty((n, nlm), dtype=torch.complex128, device="cuda")
        chol = torch.empty_like(cl)
        pc, pa, pl = _lib.ptr(cl), _lib.ptr(alms), _lib.ptr(chol)

        def call(seed):
            _lib.check(L.hx_synalm(n, LMAX, pc, ctypes.c_uint64(seed), 0, pa))

        call(1)  # warm-up: code objects, scratch
        whole, kernel, factor = [], [], []
        for r in range(REPS):
            with _lib.Timer() as t:
                call(2 + r)
            whole.append(t.ms)
        _lib.profile_enable(True)
        for r in range(REPS):
            _lib.profile_reset()
            call(2 + r)
            kernel.append(_lib.profile_get("synalm")[1])
        _lib.profile_enable(False)
        _lib.check(L.hx_cl_cholesky(n, LMAX, pc, pl))
        for r in range(REPS):
            with _lib.Timer() as t:
                _lib.check(L.hx_cl_cholesky(n, LMAX, pc, pl))
            factor.append(t.ms)
        k = statistics.median(kernel)
        out_bytes = 16.0 * n * nlm
        rb = TILE_COMP_SMALL if n <= TILE_COMP_SMALL else TILE_COMP
        draws = nlm * sum(min((b + 1) * rb, n) for b in range(-(-n // rb)))  # recomputed per register block
        row = {"ncomp": n, "lmax": LMAX, "call": summary(whole), "generator_kernel": summary(kernel), "factor_call": summary(factor),
               "output_gb": out_bytes / 1e9, "store_gbs": out_bytes / k / 1e6, "factor_read_gb": 8.0 * (n * (n + 1) // 2) * nlm / TILE_M / 1e9,
               "draws": draws, "draws_per_s": draws / k * 1e3, "ns_per_output_value": k * 1e6 / (n * nlm)}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del cl, alms, chol
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
    with open(OUT, "w") as f:
        json.dump({"peaks": peaks, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
