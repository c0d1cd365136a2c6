"""Timing of FitsCatalog: a FITS table of the README's eight columns (47 bytes a row) read into HBM and mapped.

    python tools/time_fitscatalog.py [--rows 100000000] [--page 10000000] [--dir DIR] [--json out.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/time_fitscatalog.py --kernels [--rows 10000000]
    python tools/time_fitscatalog.py --stats DIR --json out.json       (adds the kernel times of that trace to out.json)

The file is written by tests/fits_table_cases.py (10^7 random rows, repeated), read once so that it sits in the page cache, and every
timed read after that is served from there.  Reports:
  - baseline: what a user without FitsCatalog does -- np.fromfile into the structured dtype, .astype('f8') per column, .cuda(),
    ArrayCatalog -- against iterating FitsCatalog over the same file: seconds, rows/s and their ratio;
  - end to end: map_catalogs (POS, SHE, WHT, nside 4096) from the FitsCatalog against map_catalogs from an ArrayCatalog of the same
    columns already in HBM (the floor that reading and decoding add to);
  - --kernels: both decode kernels (flag HX_FITS_DIRECT off / on) on one device-resident page, for a rocprofv3 kernel trace; their
    bytes (rows x 47 in, rows x 8 x 8 out) over the kernel time, as a fraction of the 8 TB/s HBM peak.
"""

import argparse
import csv
import ctypes as C
import glob
import json
import os
import sys
import tempfile
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import heracles_amd as hx  # noqa: E402
from fits_table_cases import EXAMPLE_COLUMNS, dtype_of, example_rows, write_example_file  # noqa: E402
from heracles_amd import _lib  # noqa: E402

NSIDE = 4096
HBM_PEAK = 8.0e12  # bytes/s (MI355X, HBM3E)
NAMES = [c[0] for c in EXAMPLE_COLUMNS]
DTYPE = dtype_of(EXAMPLE_COLUMNS)


def timed(fn):
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    _lib.synchronize()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def fields():
    m = hx.HipHealpixMapper(NSIDE, 2 * NSIDE, deconvolve=False)
    return {"POS": hx.Positions(m, "ra", "dec", "w", overdensity=False), "SHE": hx.Shears(m, "ra", "dec", "g1", "-g2", "w"),
            "WHT": hx.Weights(m, "ra", "dec", "w")}


def baseline(path, offset, n, page):
    """The route without FitsCatalog: the whole table through numpy on the host, column by column to HBM."""
    import torch

    rows = np.fromfile(path, dtype=DTYPE, count=n, offset=offset)
    cols = {name: torch.as_tensor(rows[name].astype("f8")).cuda() for name in NAMES}
    return hx.ArrayCatalog(cols, page_size=page)


def iterate(path, page):
    cat = hx.FitsCatalog(path, page_size=page)
    last = None
    for p in cat:
        last = p["ra"][-1:]  # (every page is decoded when it is yielded; nothing is kept)
    return cat, last


def run_kernels(n):
    """Five launches of each decode kernel on a page of n rows that is already in HBM."""
    import torch

    rows = example_rows(n)
    raw = torch.as_tensor(np.frombuffer(rows.tobytes(), dtype=np.uint8)).cuda()
    outs = [torch.empty(n, dtype=torch.float64, device="cuda") for _ in NAMES]
    ptrs = (C.c_void_p * len(outs))(*[_lib.ptr(o).value for o in outs])
    offsets = np.array([DTYPE.fields[c][1] for c in NAMES], dtype=np.int64)
    types = "".join(c[1] for c in EXAMPLE_COLUMNS).encode()
    L = _lib.load()
    res = {"rows": n, "bytes_in": n * DTYPE.itemsize, "bytes_out": 8 * n * len(NAMES), "event_ms": {}}
    for variant in ("tile", "direct", "tile", "direct"):  # alternating; the first round warms up
        _lib.profile_reset()
        _lib.profile_enable(True)
        for _ in range(5):
            _lib.check(L.hx_fits_unpack_columns(n, DTYPE.itemsize, len(outs), offsets.ctypes.data, types, None, None, _lib.ptr(raw), ptrs,
                                                variant == "direct"))
        calls, ms = _lib.profile_get("fits_columns_" + variant)
        _lib.profile_enable(False)
        res["event_ms"][variant] = ms / max(calls, 1)
    return res


def read_stats(directory):
    """{kernel: average ns} of the two decode kernels from a rocprofv3 --kernel-trace --stats run."""
    out = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                for variant in ("tile", "direct"):
                    if "k_fits_columns_" + variant in row["Name"]:
                        out[variant] = {"calls": int(row["Calls"]), "average_ns": float(row["AverageNs"]), "min_ns": float(row["MinNs"])}
    return out


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--page", type=int, default=10_000_000)
    ap.add_argument("--dir", default=None, help="where the table is written (default: a temporary directory)")
    ap.add_argument("--json", default=None)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--stats", default=None, help="directory of a rocprofv3 --kernel-trace --stats run of --kernels")
    args = ap.parse_args()
    res = {}
    if args.json and os.path.exists(args.json):
        with open(args.json) as fh:
            res = json.load(fh)
    if args.stats:
        k = res.setdefault("kernels", {})
        k["rocprof"] = read_stats(args.stats)
        for variant, s in k["rocprof"].items():
            rate = (k["bytes_in"] + k["bytes_out"]) / (s["average_ns"] * 1e-9)
            s["bytes_per_s"], s["fraction_of_hbm_peak"] = rate, rate / HBM_PEAK
    elif args.kernels:
        hx.init(0)
        res["kernels"] = {**res.get("kernels", {}), **run_kernels(min(args.rows, 10_000_000))}
    else:
        hx.init(0)
        warnings.simplefilter("ignore")
        n, page = args.rows, args.page
        with tempfile.TemporaryDirectory(dir=args.dir) as tmp:
            path = os.path.join(tmp, "catalog.fits")
            t0 = time.perf_counter()
            write_example_file(path, n)
            res.update(rows=n, page_size=page, row_bytes=DTYPE.itemsize, columns=NAMES, file_bytes=os.path.getsize(path),
                       write_s=time.perf_counter() - t0)
            offset = hx.FitsCatalog(path)._layout()[0]
            t0 = time.perf_counter()
            with open(path, "rb") as f:  # the first read: from here on the file is in the page cache
                while f.read(1 << 26):
                    pass
            res["first_read_s"] = time.perf_counter() - t0
            res["note"] = "every timed read is the second or a later one: served from the page cache"
            # reading into HBM: baseline and FitsCatalog in turn, twice (the first round warms both up)
            for rnd in range(2):
                cat, res["baseline_s"] = timed(lambda: baseline(path, offset, n, page))
                del cat
                torch.cuda.empty_cache()
                (cat, _), res["fitscatalog_s"] = timed(lambda: iterate(path, page))
                assert cat.bytes_read == n * DTYPE.itemsize
                del cat
                torch.cuda.empty_cache()
                res.setdefault("rounds", []).append({"baseline_s": res["baseline_s"], "fitscatalog_s": res["fitscatalog_s"]})
            res["baseline_rows_per_s"], res["fitscatalog_rows_per_s"] = n / res["baseline_s"], n / res["fitscatalog_s"]
            res["fitscatalog_over_baseline"] = res["baseline_s"] / res["fitscatalog_s"]
            res["fitscatalog_file_bytes_per_s"] = n * DTYPE.itemsize / res["fitscatalog_s"]
            # end to end
            flds = fields()
            dev = baseline(path, offset, n, page)
            for rnd in range(2):
                out, res["map_from_device_columns_s"] = timed(lambda: hx.map_catalogs(flds, {1: dev}, device="cuda"))
                del out
                out, res["map_from_fitscatalog_s"] = timed(lambda: hx.map_catalogs(flds, {1: hx.FitsCatalog(path, page_size=page)}, device="cuda"))
                del out
            res["reading_and_decoding_add_s"] = res["map_from_fitscatalog_s"] - res["map_from_device_columns_s"]
    print(json.dumps(res, indent=1))
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
