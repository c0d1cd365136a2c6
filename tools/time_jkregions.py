"""Time one call of hx.jackknife_regions at production size: nside 4096, njk 100, a footprint of a third of the sky
(the polar cap z > 1/3: the first third of the RING pixels) with weights uniform(0.2, 1), everything resident in HBM.  Prints one
JSON line: the whole-call times of the repeats, the kernel families of one profiled call, and the invariants of the result.

    python tools/time_jkregions.py [--nside 4096] [--njk 100] [--repeats 5]"""

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch

    import heracles_amd as hx
    from heracles_amd import _lib

    ap = argparse.ArgumentParser()
    ap.add_argument("--nside", type=int, default=4096)
    ap.add_argument("--njk", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    npix = 12 * args.nside**2
    torch.manual_seed(5)
    w = torch.zeros(npix, dtype=torch.float64, device="cuda")
    w[: npix // 3] = torch.rand(npix // 3, dtype=torch.float64, device="cuda") * 0.8 + 0.2
    labels, info = hx.jackknife_regions(w, args.njk, return_info=True)  # warm-up
    torch.cuda.synchronize()
    times = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        labels = hx.jackknife_regions(w, args.njk)  # (the call ends in a stream synchronise)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    _lib.profile_enable(True)
    _lib.profile_reset()
    again = hx.jackknife_regions(w, args.njk)
    families = {k: _lib.profile_get(k)[1] for k in ("jk_compact", "jk_moments", "jk_sort", "jk_split", "jk_labels")}
    _lib.profile_enable(False)
    counts = torch.bincount(labels.to(torch.int64), minlength=args.njk + 1)[1:]
    rw = info["weights"]
    print(json.dumps({
        "nside": args.nside, "njk": args.njk, "footprint_pixels": int((w > 0).sum()), "call_ms": times, "kernel_families_ms": families,
        "repeatable": bool(torch.equal(labels, again)), "every_label_present": bool((counts > 0).all()),
        "outside_is_zero": bool(((labels == 0) == (w <= 0)).all()),
        "weight_spread_in_pixel_weights": float((rw.max() - rw.min()) / w.max()),
        "pixels_per_region": [int(counts.min()), int(counts.max())],
    }))


if __name__ == "__main__":
    main()
