"""Timing of map_catalogs at nside 4096: POS, SHE and WHT from one catalogue (catalogue ingest).

    python tools/time_map_catalogs.py [--rows 100000000] [--rows2 200000000] [--json out.json]

Reports, for --rows rows (and --rows2 if given and host memory allows):
  - kernel time per 10^8 rows by kernel family (hx profile: catmap_prepare / catmap_sort / catmap_add / catmap_finish), device columns;
  - the same job as separate per-field map_values calls on device maps (ang2pix / map_sort / map_add), in the same process: the
    shared sort must take less kernel time;
  - rows/s with host numpy columns at page_size 10^6 and 10^7, with the used column bytes / measured H2D rate (the PCIe floor) and
    the fraction of the wall time it is;
  - rows/s with device columns;
  - the reference's way (numpy map from create(), HipHealpixMapper.map_values per page and field, numpy moments) on 10^7 rows.
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
COLS = ("lon", "lat", "w", "e1", "e2")


def columns(n, seed=3):
    rng = np.random.default_rng(seed)
    c = {"lon": rng.uniform(0.0, 360.0, n), "lat": np.degrees(np.arcsin(rng.uniform(-1.0, 1.0, n))), "w": rng.uniform(0.5, 1.5, n),
         "e1": rng.uniform(-0.5, 0.5, n), "e2": rng.uniform(-0.5, 0.5, n)}
    c["w"][rng.random(n) < 0.01] = 0.0
    return c


def fields(m):
    return {"POS": hx.Positions(m, "lon", "lat", "w"), "SHE": hx.Shears(m, "lon", "lat", "e1", "e2", "w"), "WHT": hx.Weights(m, "lon", "lat", "w")}


def timed(fn):
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    _lib.synchronize()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def profile(names, fn):
    _lib.profile_reset()
    _lib.profile_enable(True)
    try:
        fn()
        _lib.synchronize()
    finally:
        _lib.profile_enable(False)
    return {k: _lib.profile_get(k)[1] for k in names}


def h2d_rate():
    import torch

    a = np.random.default_rng(0).standard_normal(1 << 27)  # 1 GiB
    d = torch.empty(a.size, dtype=torch.float64, device="cuda")
    _lib.copy(d, a)
    _, t = timed(lambda: _lib.copy(d, a))
    return a.nbytes / t / 1e9


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--rows2", type=int, default=0)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    hx.init(0)
    m = hx.HipHealpixMapper(NSIDE, 2 * NSIDE, deconvolve=False)
    vis = np.ones(12 * NSIDE**2)
    res = {"nside": NSIDE, "fields": ["POS", "SHE", "WHT"], "h2d_gbs": h2d_rate()}
    warnings.simplefilter("ignore")
    for n in [args.rows] + ([args.rows2] if args.rows2 else []):
        r = {}
        host = columns(n)
        dev = {k: torch.as_tensor(v, device="cuda") for k, v in host.items()}
        dvis = torch.as_tensor(vis, device="cuda")
        run_dev = lambda: hx.map_catalogs(fields(m), {0: hx.ArrayCatalog(dev, page_size=10_000_000, visibility=dvis)}, device="cuda")
        run_dev()  # warm-up (allocations, code objects)
        kinds = ("catmap_prepare", "catmap_sort", "catmap_add", "catmap_finish")
        prof = profile(kinds, run_dev)
        r["shared_kernel_ms_per_1e8"] = {k: v * 1e8 / n for k, v in prof.items()}
        # (the finish pass normalises the maps, which the separate calls below do not do: compared without it)
        r["shared_kernel_ms_per_1e8"]["total"] = sum(v for k, v in prof.items() if k != "catmap_finish") * 1e8 / n
        _, t = timed(run_dev)
        r["device_columns_rows_per_s"] = n / t
        # separate per-field hx_map_values on device maps, pages of 10^7, same process
        npix = 12 * NSIDE**2

        def separate():
            maps = [torch.zeros(npix, dtype=torch.float64, device="cuda"), torch.zeros((2, npix), dtype=torch.float64, device="cuda"),
                    torch.zeros(npix, dtype=torch.float64, device="cuda")]
            for s in range(0, n, 10_000_000):
                sl = slice(s, s + 10_000_000)
                lon, lat, w = dev["lon"][sl], dev["lat"][sl], dev["w"][sl]
                m.map_values(lon, lat, maps[0], w)
                keep = w != 0
                kl, kb, kw = lon[keep], lat[keep], w[keep]
                m.map_values(kl, kb, maps[1], torch.stack([dev["e1"][sl][keep] * kw, dev["e2"][sl][keep] * kw]))
                m.map_values(kl, kb, maps[2], kw)

        separate()
        sep = profile(("ang2pix", "map_sort", "map_add"), separate)
        r["separate_kernel_ms_per_1e8"] = {k: v * 1e8 / n for k, v in sep.items()}
        r["separate_kernel_ms_per_1e8"]["total"] = sum(sep.values()) * 1e8 / n
        r["shared_below_separate"] = r["shared_kernel_ms_per_1e8"]["total"] < r["separate_kernel_ms_per_1e8"]["total"]
        del dev
        torch.cuda.empty_cache()
        used = n * 8 * len(COLS)
        for ps in (1_000_000, 10_000_000):
            run_host = lambda: hx.map_catalogs(fields(m), {0: hx.ArrayCatalog(host, page_size=ps, visibility=vis)}, device="cuda")
            _, t = timed(run_host)
            floor = used / (res["h2d_gbs"] * 1e9)
            r[f"host_columns_page{ps}"] = {"rows_per_s": n / t, "wall_s": t, "column_bytes": used, "pcie_floor_s": floor,
                                           "pcie_fraction": floor / t}
        if n == args.rows:
            nref = min(n, 10_000_000)
            sub = {k: v[:nref] for k, v in host.items()}

            def reference_way():
                pos, she, wht = m.create(spin=0), m.create(2, spin=2), m.create(spin=0)
                stats = [0.0] * 6
                for s in range(0, nref, 1_000_000):
                    pg = {k: v[s : s + 1_000_000] for k, v in sub.items()}
                    m.map_values(pg["lon"], pg["lat"], pos, pg["w"])
                    keep = pg["w"] != 0
                    pg = {k: v[keep] for k, v in pg.items()}
                    w = pg["w"]
                    m.map_values(pg["lon"], pg["lat"], she, np.r_[[w * pg["e1"], w * pg["e2"]]])
                    m.map_values(pg["lon"], pg["lat"], wht, w)
                    stats = [stats[0] + w.sum(), stats[1] + (w**2).sum(), stats[2] + ((w * pg["e1"]) ** 2 + (w * pg["e2"]) ** 2).sum(),
                             stats[3], stats[4], stats[5]]
                return pos, she, wht

            _, t = timed(reference_way)
            r["reference_way_1e7"] = {"rows": nref, "wall_s": t, "rows_per_s": nref / t}
        res[str(n)] = r
        del host
    print(json.dumps(res, indent=1))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
