"""hx_mockcat_counts / hx_mockcat_points at production size: expected counts, counts and the catalogue resident in HBM, nside 4096
(env NSIDE), lambda = 2 in every pixel (env LAMBDA), zero and two value columns (env NVALS).

Per case: each whole call by the library's event timer, and each kernel from the library's scopes (`mockcat_counts`, `mockcat_scan`,
`mockcat_points`) in calls of their own; each warmed up, median and min .. max of REPS.  The point kernel's store rate (16 + 8 nval
bytes per point over its kernel time) is set against the copy probe of hx_measure_peaks (which counts read + write bytes: a
store-only kernel is compared with half of it), its points per second against the draws per second of k_synalm.
Results as JSON in OUT (default profiles/mockcat.json).  DESIGN.md 4.16."""

import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import heracles_amd as hx
from heracles_amd import _lib

NSIDE = int(os.environ.get("NSIDE", "4096"))
LAMBDA = float(os.environ.get("LAMBDA", "2"))
NVALS = [int(x) for x in os.environ.get("NVALS", "0,2").split(",")]
REPS = int(os.environ.get("REPS", "7"))
OUT = os.environ.get("OUT", "profiles/mockcat.json")


def summary(xs):
    return {"median_ms": statistics.median(xs), "min_ms": min(xs), "max_ms": max(xs)}


def main():
    hx.init(0)
    L = _lib.load()
    peaks = _lib.measure_peaks()
    print("peaks:", peaks, flush=True)
    npix = 12 * NSIDE * NSIDE
    lam = torch.full((npix,), LAMBDA, dtype=torch.float64, device="cuda")
    counts = torch.empty(npix, dtype=torch.int64, device="cuda")
    total = ctypes.c_int64(0)
    pl, pc = _lib.ptr(lam), _lib.ptr(counts)

    def count(seed):
        _lib.check(L.hx_mockcat_counts(NSIDE, 0, npix, pl, ctypes.c_uint64(seed), 0, pc, ctypes.byref(total)))

    count(1)  # warm-up: code objects
    whole, kernel = [], []
    for r in range(REPS):
        with _lib.Timer() as t:
            count(2 + r)
        whole.append(t.ms)
    _lib.profile_enable(True)
    for r in range(REPS):
        _lib.profile_reset()
        count(2 + r)
        kernel.append(_lib.profile_get("mockcat_counts")[1])
    _lib.profile_enable(False)
    k = statistics.median(kernel)
    out = {"peaks": peaks, "nside": NSIDE, "lambda": LAMBDA, "pixels": npix,
           "counts": {"call": summary(whole), "kernel": summary(kernel), "pixels_per_s": npix / k * 1e3}, "points": []}
    print(json.dumps(out["counts"]), flush=True)
    count(2)
    n = int(total.value)
    lon = torch.empty(n, dtype=torch.float64, device="cuda")
    lat = torch.empty(n, dtype=torch.float64, device="cuda")
    for nval in NVALS:
        maps = torch.zeros((nval, npix), dtype=torch.float64, device="cuda") if nval else None
        sigma = torch.full((nval,), 0.3, dtype=torch.float64) if nval else None
        values = torch.empty((nval, n), dtype=torch.float64, device="cuda") if nval else None
        args = (NSIDE, 0, npix, pc, ctypes.c_uint64(2), 0, nval, _lib.ptr(maps), _lib.ptr(sigma), _lib.ptr(lon), _lib.ptr(lat), _lib.ptr(values), None)

        def points():
            _lib.check(L.hx_mockcat_points(*args))

        points()
        whole, kernel, scan = [], [], []
        for r in range(REPS):
            with _lib.Timer() as t:
                points()
            whole.append(t.ms)
        _lib.profile_enable(True)
        for r in range(REPS):
            _lib.profile_reset()
            points()
            kernel.append(_lib.profile_get("mockcat_points")[1])
            scan.append(_lib.profile_get("mockcat_scan")[1])
        _lib.profile_enable(False)
        k = statistics.median(kernel)
        out_bytes = (16.0 + 8.0 * nval) * n
        row = {"nval": nval, "points": n, "call": summary(whole), "point_kernel": summary(kernel), "scan_kernels": summary(scan),
               "output_gb": out_bytes / 1e9, "store_gbs": out_bytes / k / 1e6, "store_share_of_half_copy_probe": out_bytes / k / 1e6 / (0.5 * peaks["hbm_copy_gbs"]),
               "points_per_s": n / k * 1e3, "philox_calls_per_s": n * (1 + nval) / k * 1e3}
        out["points"].append(row)
        print(json.dumps(row), flush=True)
        del maps, values
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
