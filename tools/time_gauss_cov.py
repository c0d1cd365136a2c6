"""hx_gauss_cov_accumulate at production size: L = 2048 (env LMAX), logarithmic bins with 2l+1 weights (env NBINS = 32: that many
intervals from 2 to L + 1, edges rounded and duplicates dropped, which leaves 31 bins at the defaults), ONE coupling table, and the item list of the production data vector (10 bins x (POS, SHE): 475 blocks of the data vector, 113050 block pairs, 465
spectra) as it is when every field and bin has the same mask: every block pair is one two-term item of that table.

Timed, each warmed up, median and min .. max of REPS: the whole accumulate call (host checks and member lists, uploads, the three
kernels) by the library's event timer; its kernels alone from the `gauss_cov` scope; and, next to it, one build of the (0,0) table by
`MixmatContext(L, L, 2L)` into HBM.  The flops the call counted (hx_executed_flops) over the kernel time are set against the FP64
vector rate of hx_measure_peaks.  Results as JSON in OUT (default profiles/gauss_cov.json).  DESIGN.md 4.19."""

import itertools
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

import heracles_amd as hx
from heracles_amd import _lib
from heracles_amd.gausscov import ITEM, _accumulate, covariance_requests

LMAX = int(os.environ.get("LMAX", "2048"))
NBINS = int(os.environ.get("NBINS", "32"))
NZBIN = int(os.environ.get("NZBIN", "10"))
REPS = int(os.environ.get("REPS", "5"))
OUT = os.environ.get("OUT", "profiles/gauss_cov.json")


class _F:
    def __init__(self, spin, mask):
        self.spin, self.mask = spin, mask


def summary(xs):
    return {"median_ms": statistics.median(xs), "min_ms": min(xs), "max_ms": max(xs)}


def shared_mask_items(nl):
    """The production layout's request list with every table folded into one: one item per block pair, both terms."""
    maps = [("POS", i) for i in range(NZBIN)] + [("SHE", i) for i in range(NZBIN)]
    spin = {"POS": 0, "SHE": 2}
    cls = {(a, b, i, j): hx.Result(np.zeros(tuple(2 for f in (a, b) if f == "SHE") + (nl,)), spin=(spin[a], spin[b]), axis=-1)
           for (a, i), (b, j) in itertools.combinations_with_replacement(maps, 2)}
    req = covariance_requests(cls, {"POS": _F(0, "V"), "SHE": _F(2, "V")})
    terms = {}
    for blocks in req.tables.values():
        for u1, u2, s in blocks:
            terms.setdefault((u1, u2), []).extend(v for v in s if v >= 0)
    items = np.empty(len(terms), dtype=ITEM)
    for n, ((u1, u2), s) in enumerate(sorted(terms.items())):
        items[n] = (u1, u2, s)
    return items, len(req.units), len(req.spectra)


def main():
    hx.init(0)
    peaks = _lib.measure_peaks()
    print("peaks:", peaks, flush=True)
    nl = LMAX + 1
    t0 = time.perf_counter()
    items, nunits, nspec = shared_mask_items(nl)
    t_requests = time.perf_counter() - t0
    edges = np.unique(np.round(np.geomspace(2, nl, NBINS + 1)).astype(int))
    plan = hx.BinPlan(np.arange(nl), edges, "2l+1")
    items["row"] *= plan.nbins
    items["col"] *= plan.nbins
    N = nunits * plan.nbins
    gen = torch.Generator(device="cuda").manual_seed(LMAX)
    spec = 1.0 + torch.rand((nspec, nl), dtype=torch.float64, device="cuda", generator=gen)
    cov = torch.zeros((N, N), dtype=torch.float64, device="cuda")
    g00 = torch.empty((nl, nl), dtype=torch.float64, device="cuda")
    wcl = 1.0 / (1.0 + np.arange(2 * LMAX + 1)) ** 2
    build, whole, kernel = [], [], []
    with hx.MixmatContext(LMAX, LMAX, 2 * LMAX) as ctx:
        ctx(wcl, (0, 0), out=g00)  # warm-up: tables of the context, code objects
        for _ in range(REPS):
            with _lib.Timer() as t:
                ctx(wcl, (0, 0), out=g00)
            build.append(t.ms)

    def call():
        _accumulate(g00, spec, items, cov, plan)

    call()  # warm-up: code objects, the scratch of the folded table
    for _ in range(REPS):
        with _lib.Timer() as t:
            call()
        whole.append(t.ms)
    _lib.executed_flops(reset=True)
    call()
    flops = _lib.executed_flops(reset=True)[1]
    _lib.profile_enable(True)
    for _ in range(REPS):
        _lib.profile_reset()
        call()
        kernel.append(_lib.profile_get("gauss_cov")[1])
    _lib.profile_enable(False)
    k = statistics.median(kernel)
    row = {"lmax": LMAX, "nbins": int(plan.nbins), "items": int(len(items)), "units": nunits, "spectra": nspec, "N": N,
           "requests_s": t_requests, "table_build": summary(build), "call": summary(whole), "kernels": summary(kernel),
           "z_gib": (nspec + 1) * plan.nbins * nl * 8 / 2**30, "executed_gflop": flops / 1e9, "gflops": flops / k / 1e6,
           "fp64_valu_share": flops / k / 1e9 / peaks["fp64_valu_tflops"], "us_per_item": k * 1e3 / len(items)}
    print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
    with open(OUT, "w") as f:
        json.dump({"peaks": peaks, "rows": [row]}, f, indent=1)


if __name__ == "__main__":
    main()
