"""Time hx.mask_polygons at production size: nside 4096, a footprint of a third of the sky (the polar cap z > 1/3:
the first third of the RING pixels), rectangles from hx.rectangle_polygons at random positions of the footprint and random angles.
Three jobs: 10^6 diffraction spikes of 2' .. 20' by 0.3' .. 1' cut out of the footprint; 10^3 trails of 5 .. 30 degrees by 0.5'
cut out of it; 10^4 tiles of 0.7 by 0.7 degrees as a union (value = 1.0 on a map of zeros).  Everything resident in HBM, one warm-up
call each, the median of the repeats with their minimum and maximum.  Writes profiles/maskpoly.json and prints it.

    python tools/time_maskpoly.py [--nside 4096] [--spikes 1000000] [--trails 1000] [--tiles 10000] [--repeats 5] [--out profiles/maskpoly.json]"""

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
    ap.add_argument("--spikes", type=int, default=1000000)
    ap.add_argument("--trails", type=int, default=1000)
    ap.add_argument("--tiles", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "maskpoly.json"))
    args = ap.parse_args()
    npix = 12 * args.nside**2
    gen = torch.Generator(device="cuda").manual_seed(7)

    def uniform(n, lo, hi):
        return torch.rand(n, dtype=torch.float64, device="cuda", generator=gen) * (hi - lo) + lo

    def rectangles(n, length, width):
        lon, lat = uniform(n, 0.0, 360.0), torch.rad2deg(torch.asin(uniform(n, 1.0 / 3.0, 1.0)))
        return hx.rectangle_polygons(lon, lat, uniform(n, *length), uniform(n, *width), uniform(n, 0.0, 180.0))

    footprint = torch.zeros(npix, dtype=torch.float64, device="cuda")
    footprint[: npix // 3] = 1.0
    empty = torch.zeros(npix, dtype=torch.float64, device="cuda")
    jobs = {
        "spikes": (rectangles(args.spikes, (2.0 / 60, 20.0 / 60), (0.3 / 60, 1.0 / 60)), footprint, 0.0),
        "trails": (rectangles(args.trails, (5.0, 30.0), (0.5 / 60, 0.5 / 60)), footprint, 0.0),
        "tiles": (rectangles(args.tiles, (0.7, 0.7), (0.7, 0.7)), empty, 1.0),
    }

    def timed(call, prepare):
        ms, last = [], None
        for k in range(args.repeats + 1):  # (the first one warms up)
            arg = prepare()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last = call(arg)  # (every call ends in a stream synchronise)
            torch.cuda.synchronize()
            if k:
                ms.append((time.perf_counter() - t0) * 1e3)
        return ms, last

    def family(call, name):
        _lib.profile_enable(True)
        _lib.profile_reset()
        call()
        got = _lib.profile_get(name)[1]
        _lib.profile_enable(False)
        return got

    result = {"nside": args.nside, "pixels": npix, "footprint_pixels": npix // 3, "repeats": args.repeats}
    for name, ((lon, lat), start, value) in jobs.items():
        n = int(lon.shape[0])
        ms, out = timed(lambda m: hx.mask_polygons(m, lon, lat, value=value), start.clone)
        again = hx.mask_polygons(start.clone(), lon, lat, value=value)
        result[name] = {"polygons": n, "value": value, "call": spread(ms),
                        "kernels_ms": family(lambda: hx.mask_polygons(start.clone(), lon, lat, value=value), "mask_polygons"),
                        "polygons_per_s": n / (statistics.median(ms) * 1e-3), "pixels_written": int((out != start).sum()),
                        "repeatable": bool(torch.equal(out, again))}
        del out, again
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
