"""Time hx.mask_discs and hx.apodize_mask at production size: nside 4096, a footprint of a third of the sky (the
polar cap z > 1/3: the first third of the RING pixels), 10^6 discs of 0.5' .. 5' plus 100 discs of 0.5 .. 3 degrees at random
positions of the footprint, then the apodisation of the result with aposize 0.5 degrees, both kinds.  Everything resident in HBM,
one warm-up call each, the median of the repeats with their minimum and maximum.  Writes profiles/masktools.json and prints it.

    python tools/time_masktools.py [--nside 4096] [--small 1000000] [--large 100] [--aposize 0.5] [--repeats 5] [--out profiles/masktools.json]"""

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def main():
    import torch

    import heracles_amd as hx
    from heracles_amd import _lib

    ap = argparse.ArgumentParser()
    ap.add_argument("--nside", type=int, default=4096)
    ap.add_argument("--small", type=int, default=1000000)
    ap.add_argument("--large", type=int, default=100)
    ap.add_argument("--aposize", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "masktools.json"))
    args = ap.parse_args()
    npix = 12 * args.nside**2
    gen = torch.Generator(device="cuda").manual_seed(7)
    ndisc = args.small + args.large

    def uniform(n, lo, hi):
        return torch.rand(n, dtype=torch.float64, device="cuda", generator=gen) * (hi - lo) + lo

    lon = uniform(ndisc, 0.0, 360.0)
    lat = torch.rad2deg(torch.asin(uniform(ndisc, 1.0 / 3.0, 1.0)))
    radius = torch.cat([uniform(args.small, 0.5 / 60, 5.0 / 60), uniform(args.large, 0.5, 3.0)])
    footprint = torch.zeros(npix, dtype=torch.float64, device="cuda")
    footprint[: npix // 3] = 1.0

    def timed(call, prepare=None):
        ms, last = [], None
        for k in range(args.repeats + 1):  # (the first one warms up)
            arg = prepare() if prepare else None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last = call(arg)  # (every call ends in a stream synchronise)
            torch.cuda.synchronize()
            if k:
                ms.append((time.perf_counter() - t0) * 1e3)
        return ms, last

    def families(call, names):
        _lib.profile_enable(True)
        _lib.profile_reset()
        call()
        got = {k: _lib.profile_get(k)[1] for k in names}
        _lib.profile_enable(False)
        return got

    result = {"nside": args.nside, "pixels": npix, "footprint_pixels": npix // 3, "discs_small": args.small, "discs_large": args.large,
              "aposize_deg": args.aposize, "repeats": args.repeats}
    ms, holes = timed(lambda m: hx.mask_discs(m, lon, lat, radius), footprint.clone)
    again = hx.mask_discs(footprint.clone(), lon, lat, radius)
    cleared = int((footprint > 0).sum() - (holes > 0).sum())
    result["mask_discs"] = {"call": spread(ms), "kernel_families_ms": families(lambda: hx.mask_discs(footprint.clone(), lon, lat, radius), ("mask_discs",)),
                            "pixels_cleared": cleared, "discs_per_s": ndisc / (statistics.median(ms) * 1e-3), "repeatable": bool(torch.equal(holes, again))}
    del again
    result["apodize_mask"] = {}
    for kind in ("C1", "C2"):
        ms, apod = timed(lambda _: hx.apodize_mask(holes, args.aposize, kind))
        again = hx.apodize_mask(holes, args.aposize, kind)
        result["apodize_mask"][kind] = {
            "call": spread(ms), "kernel_families_ms": families(lambda: hx.apodize_mask(holes, args.aposize, kind), ("mask_neighbours", "mask_distance")),
            "unmasked_pixels_per_s": float((holes > 0).sum()) / (statistics.median(ms) * 1e-3), "repeatable": bool(torch.equal(apod, again)),
            "mean_of_result": float(apod.mean()), "pixels_tapered": int(((apod > 0) & (apod < holes)).sum())}
        del apod, again
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
