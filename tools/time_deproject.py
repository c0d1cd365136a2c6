"""Time hx_deproject_gram and hx_deproject_apply at production size: nside 4096, 32 spin-0 templates and one map, a
non-binary mask, everything resident in HBM, one warm-up call each, the median of the repeats with their minimum and maximum.  The
two calls are timed separately.  Bytes are counted from the shapes: the Gram pass reads every column and, per column tile, the mask
once; the apply pass reads the templates, the mask and the map and writes the map.  The achieved rates are those bytes (and the
matrix-unit flops the library counted) over the kernel time of the library's profile scopes.  Writes profiles/deproject.json.

    python tools/time_deproject.py [--nside 4096] [--templates 32] [--maps 1] [--repeats 5] [--out profiles/deproject.json]"""

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
    import numpy as np
    import torch

    import heracles_amd as hx
    from heracles_amd import _lib
    from heracles_amd import deprojection as dp

    ap = argparse.ArgumentParser()
    ap.add_argument("--nside", type=int, default=4096)
    ap.add_argument("--templates", type=int, default=32)
    ap.add_argument("--maps", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deproject.json"))
    args = ap.parse_args()
    npix = 12 * args.nside**2
    k, m = args.templates, args.maps
    n = k + m
    gen = torch.Generator(device="cuda").manual_seed(11)
    t = [torch.randn((1, npix), dtype=torch.float64, device="cuda", generator=gen) for _ in range(k)]
    v = torch.rand(npix, dtype=torch.float64, device="cuda", generator=gen)
    d = [torch.randn((1, npix), dtype=torch.float64, device="cuda", generator=gen) * v for _ in range(m)]
    out = [torch.empty_like(x) for x in d]
    alpha = np.random.default_rng(3).standard_normal((m, k))

    def timed(call):
        ms, last = [], None
        for r in range(args.repeats + 1):  # (the first one warms up)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last = call()  # (every call ends in a stream synchronise)
            if r:
                ms.append((time.perf_counter() - t0) * 1e3)
        return ms, last

    def scope(call, name):
        """Kernel time of the profile scope `name` over the repeats (one warm-up), each from a call of its own."""
        ms = []
        _lib.profile_enable(True)
        for r in range(args.repeats + 1):
            _lib.profile_reset()
            call()
            if r:
                ms.append(_lib.profile_get(name)[1])
        _lib.profile_enable(False)
        return ms

    result = {"nside": args.nside, "pixels": npix, "templates": k, "maps": m, "repeats": args.repeats}
    tiles = -(-n // 64)
    gram_bytes = 8.0 * npix * (n + tiles)  # every column once (one row of tiles here), the mask once per tile row
    gram_call = lambda: dp.deproject_gram(t, d, v)  # noqa: E731
    ms, g = timed(gram_call)
    again = gram_call()
    _lib.executed_flops(reset=True)
    gram_call()
    executed, _ = _lib.executed_flops(reset=True)
    kms = scope(gram_call, "deproject_gram")
    med = statistics.median(kms) * 1e-3
    result["gram"] = {"call": spread(ms), "kernels": spread(kms), "bytes_read": gram_bytes, "read_tb_per_s": gram_bytes / med / 1e12,
                      "flops_useful": 2.0 * npix * n * (n + 1) / 2, "flops_executed": executed, "executed_tflops": executed / med / 1e12,
                      "repeatable": bool(np.array_equal(g, again)), "symmetric": bool(np.array_equal(g, g.T))}
    apply_bytes = 8.0 * npix * (k + 1 + 2 * m)
    apply_call = lambda: dp.deproject_apply(t, v, d, alpha, out)  # noqa: E731
    ms, _ = timed(apply_call)
    kms = scope(apply_call, "deproject_apply")
    med = statistics.median(kms) * 1e-3
    result["apply"] = {"call": spread(ms), "kernels": spread(kms), "bytes_moved": apply_bytes, "tb_per_s": apply_bytes / med / 1e12}
    peaks = _lib.measure_peaks()
    result["device"] = {"hbm_read_gbs": peaks["hbm_read_gbs"], "fp64_mfma_tflops": peaks["fp64_mfma_tflops"]}
    result["gram"]["share_of_measured_read_bandwidth"] = result["gram"]["read_tb_per_s"] * 1e3 / peaks["hbm_read_gbs"]
    result["gram"]["share_of_measured_mfma_rate"] = result["gram"]["executed_tflops"] / peaks["fp64_mfma_tflops"]
    result["apply"]["share_of_measured_read_bandwidth"] = result["apply"]["tb_per_s"] * 1e3 / peaks["hbm_read_gbs"]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
