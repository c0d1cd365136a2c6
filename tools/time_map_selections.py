"""Timing of map_catalogs for the views of one catalogue: 13 disjoint TOM_BIN_ID==k bins, POS + SHE + WHT, nside 4096 (DESIGN.md
section 4.8, selections).

    python tools/time_map_selections.py [--rows 100000000] [--bins 13] [--json out.json]

Reports:
  - kernel time by family (hx profile: catmap_prepare / catmap_sort / catmap_add / catmap_finish) of the one-pass path, device columns;
  - wall seconds and rows/s of the one-pass path and of the per-view path (each view mapped as its own catalogue of its rows, the way a
    caller without views does it), from device columns and from host columns in pages of 10^7.
"""

import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import heracles_amd as hx  # noqa: E402
from heracles_amd import _lib  # noqa: E402

NSIDE = 4096
FAMILIES = ("catmap_prepare", "catmap_sort", "catmap_add", "catmap_finish")


def columns(n, bins, seed=3):
    rng = np.random.default_rng(seed)
    return {"lon": rng.uniform(0.0, 360.0, n), "lat": np.degrees(np.arcsin(rng.uniform(-1.0, 1.0, n))), "w": rng.uniform(0.5, 1.5, n),
            "e1": rng.uniform(-0.5, 0.5, n), "e2": rng.uniform(-0.5, 0.5, n), "TOM_BIN_ID": rng.integers(0, bins, n).astype(np.float64)}


def fields(m):
    return {"POS": hx.Positions(m, "lon", "lat", "w", overdensity=False), "SHE": hx.Shears(m, "lon", "lat", "e1", "-e2", "w"),
            "WHT": hx.Weights(m, "lon", "lat", "w")}


def timed(fn):
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    _lib.synchronize()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def one_pass(flds, base, bins):
    return hx.map_catalogs(flds, {k: base[f"TOM_BIN_ID=={k}"] for k in range(bins)}, device="cuda")


def per_view(flds, cols, page_size, bins):
    """Each bin as its own catalogue, mapped one after the other (its maps dropped before the next: only one bin's maps live)."""
    for k in range(bins):
        keep = cols["TOM_BIN_ID"] == k
        sub = {c: v[keep] for c, v in cols.items()}
        if hasattr(keep, "data_ptr"):
            sub = {c: v.contiguous() for c, v in sub.items()}
        out = hx.map_catalogs(flds, {k: hx.ArrayCatalog(sub, page_size=page_size)}, device="cuda")
        del out, sub


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--bins", type=int, default=13)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    hx.init(0)
    warnings.simplefilter("ignore")
    n, bins = args.rows, args.bins
    flds = fields(hx.HipHealpixMapper(NSIDE, 2 * NSIDE, deconvolve=False))
    host = columns(n, bins)
    dev = {k: torch.as_tensor(v, device="cuda") for k, v in host.items()}
    res = {"nside": NSIDE, "rows": n, "bins": bins, "fields": list(flds)}

    # each path once as a warm-up, then timed; the host one pass runs first, before any large device allocation
    page = 10_000_000
    hbase = hx.ArrayCatalog(host, page_size=page)
    dbase = hx.ArrayCatalog(dev, page_size=n)
    for name, fn in (("one_pass_host", lambda: one_pass(flds, hbase, bins)), ("one_pass_device", lambda: one_pass(flds, dbase, bins))):
        for rep in range(2):
            torch.cuda.empty_cache()
            if rep and name == "one_pass_device":
                _lib.profile_reset()
                _lib.profile_enable(True)
            out, t = timed(fn)
            _lib.profile_enable(False)
            del out
        res[name + "_s"] = t
    res["kernel_ms"] = {f: _lib.profile_get(f)[1] for f in FAMILIES}
    torch.cuda.empty_cache()
    _, res["per_view_device_s"] = timed(lambda: per_view(flds, dev, n, bins))
    torch.cuda.empty_cache()
    _, res["per_view_host_s"] = timed(lambda: per_view(flds, host, page, bins))
    # the host one pass again, after the device runs and their allocations (the order of the first version of this tool)
    torch.cuda.empty_cache()
    out, res["one_pass_host_after_device_runs_s"] = timed(lambda: one_pass(flds, hbase, bins))
    del out
    for k in ("one_pass_device", "per_view_device", "one_pass_host", "per_view_host"):
        res[k + "_rows_per_s"] = n / res[k + "_s"]
    res["ratio_device"] = res["one_pass_device_s"] / res["per_view_device_s"]
    res["ratio_host"] = res["one_pass_host_s"] / res["per_view_host_s"]
    print(json.dumps(res, indent=1))
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
