"""catalog_alms against the per-page route it replaces, on device columns: Positions + Shears + Weights (4 components) of one
catalogue at the bench's band limit.

  new   hx.catalog_alms(fields, {0: ArrayCatalog of CUDA columns}, device="cuda"): every page is spread into resident grids, one
        finishing transform per field.
  page  what there was before: per page and field, the (theta, phi) and w v rows formed with torch on the device and one
        PointSHT.adjoint_synthesis call (the transform behind HipDiscreteMapper.map_values, which itself takes host arrays only: the
        device call leaves the PCIe copies of that method out, in favour of this route), the alms added up on the device; the moments
        with torch sums.

Both routes are warmed up once, then timed alternately, `--repeats` times each, a host clock around work that ends in a device
synchronise.  `--route new|page` runs one route only (for a kernel trace in a run of its own).  Results: one JSON object on stdout and
in `--out`.

    python tools/time_catalog_alms.py [--rows 1e8] [--page 1e7] [--lmax 6144] [--repeats 5] [--out profiles/catalog_alms.json]
"""
import argparse
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import heracles_amd as hx  # noqa: E402


def columns(n, seed=1):
    g = torch.Generator(device="cuda").manual_seed(seed)
    u = lambda: torch.rand(n, dtype=torch.float64, device="cuda", generator=g)
    return {"lon": u() * 360.0, "lat": torch.rad2deg(torch.asin(u() * 2 - 1)), "g1": u() - 0.5, "g2": u() - 0.5, "w": u() + 0.5}


def route_new(fields, cols, page):
    cat = hx.ArrayCatalog(cols, page_size=page)
    return hx.catalog_alms(fields, {0: cat}, device="cuda")


def route_page(sht, cols, page):
    n = cols["lon"].numel()
    nlm = sht.nlm
    alm = {"POS": torch.zeros((1, nlm), dtype=torch.complex128, device="cuda"), "SHE": torch.zeros((2, nlm), dtype=torch.complex128, device="cuda"),
           "WHT": torch.zeros((1, nlm), dtype=torch.complex128, device="cuda")}
    sw = sw2 = sv2 = 0.0
    for i in range(0, n, page):
        c = {k: v[i : i + page] for k, v in cols.items()}
        loc = torch.stack([torch.deg2rad(90.0 - c["lat"]), torch.deg2rad(torch.remainder(c["lon"], 360.0))], dim=1)
        w = c["w"]
        she = torch.stack([w * c["g1"], w * c["g2"]])
        alm["POS"] += sht.adjoint_synthesis(loc, torch.ones_like(w)[None], spin=0)
        alm["SHE"] += sht.adjoint_synthesis(loc, she, spin=2)
        alm["WHT"] += sht.adjoint_synthesis(loc, w[None], spin=0)
        sw += float(w.sum())
        sw2 += float((w * w).sum())
        sv2 += float((she * she).sum())
    wbar = n / (4 * math.pi) * (sw / n)
    alm["POS"] /= n / (4 * math.pi)
    alm["SHE"] /= wbar
    alm["WHT"] /= wbar
    return alm, (sw, sw2, sv2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=1e8)
    ap.add_argument("--page", type=float, default=1e7)
    ap.add_argument("--lmax", type=int, default=6144)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--route", choices=["both", "new", "page"], default="both")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, page = int(a.rows), int(a.page)
    hx.init(0)
    cols = columns(n)
    m = hx.HipDiscreteMapper(a.lmax)
    fields = {"POS": hx.Positions(m, "lon", "lat", overdensity=False), "SHE": hx.Shears(m, "lon", "lat", "g1", "g2", "w"),
              "WHT": hx.Weights(m, "lon", "lat", "w")}
    sht = hx.get_point_sht(a.lmax)
    routes = {"new": lambda: route_new(fields, cols, page), "page": lambda: route_page(sht, cols, page)}
    names = [r for r in routes if a.route in ("both", r)]
    last = {}
    for r in names:  # warm-up: code objects, plans, the library's scratch
        last[r] = routes[r]()
        torch.cuda.synchronize()
        print(f"{r}: warmed up", file=sys.stderr, flush=True)
    times = {r: [] for r in names}
    for _ in range(a.repeats):
        for r in names:  # alternating
            torch.cuda.synchronize()
            t = time.perf_counter()
            last[r] = routes[r]()
            torch.cuda.synchronize()
            times[r].append(time.perf_counter() - t)
            print(f"{r}: {times[r][-1]:.3f} s", file=sys.stderr, flush=True)
    res = {"rows": n, "page": page, "lmax": a.lmax, "grid": sht.ngrid, "repeats": a.repeats, "components": 4}
    for r in names:
        t = sorted(times[r])
        res[r] = {"seconds": times[r], "median": t[len(t) // 2], "min": t[0], "max": t[-1], "rows_per_s": n / t[len(t) // 2]}
    if len(names) == 2:
        res["page_over_new"] = res["page"]["median"] / res["new"]["median"]
        worst = 0.0
        for k, b in last["page"][0].items():
            x = last["new"][k, 0].tensor.reshape(b.shape)
            worst = max(worst, float((x - b).abs().max() / b.abs().max()))
        res["max_difference_of_the_routes"] = worst  # relative to the largest |alm| of the field
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
