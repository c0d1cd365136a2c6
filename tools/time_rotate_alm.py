"""hx_rotate_alm at production size: alms resident in HBM, lmax 2048 and 6144 (env LMAXS), 1 and 8 components (env NCOMPS), generic
angles (env ANGLES: psi,theta,phi).

Per case: the whole call (host tables in long doubles, their upload, the kernel) by the library's event timer (hx_timer_*), and the
rotation kernel alone from the library's `rotate_alm` scope in calls of their own; each warmed up, median and min .. max of REPS.  The
flops the kernel counted (hx_executed_flops: 25 per step of a pair of chains, 8 per (pair, l, component) plus 4 per (pair, l)) over
its time are set against the FP64 vector rate of hx_measure_peaks.  Results as JSON in OUT (default profiles/rotate_alm.json).
DESIGN.md 4.18."""

import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

import heracles_amd as hx
from heracles_amd import _lib
from heracles_amd.rotation import TILE_COMP

LMAXS = [int(x) for x in os.environ.get("LMAXS", "2048,6144").split(",")]
NCOMPS = [int(x) for x in os.environ.get("NCOMPS", "1,8").split(",")]
REPS = int(os.environ.get("REPS", "5"))
OUT = os.environ.get("OUT", "profiles/rotate_alm.json")
ANGLES = tuple(float(x) for x in os.environ.get("ANGLES", "0.7,1.234,-2.1").split(","))  # sin(theta) < 0.1: the two-pass path


def summary(xs):
    return {"median_ms": statistics.median(xs), "min_ms": min(xs), "max_ms": max(xs)}


def main():
    hx.init(0)
    L = _lib.load()
    peaks = _lib.measure_peaks()
    print("peaks:", peaks, flush=True)
    rows = []
    for lmax in LMAXS:
        nlm = (lmax + 1) * (lmax + 2) // 2
        for n in NCOMPS:
            gen = torch.Generator(device="cuda").manual_seed(lmax + n)
            alm = torch.view_as_complex(torch.randn((n, nlm, 2), dtype=torch.float64, device="cuda", generator=gen))
            out = torch.empty_like(alm)
            pa, po = _lib.ptr(alm), _lib.ptr(out)

            def call():
                _lib.check(L.hx_rotate_alm(lmax, n, pa, po, *ANGLES))

            call()  # warm-up: code objects
            whole, kernel = [], []
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
                kernel.append(_lib.profile_get("rotate_alm")[1])
            _lib.profile_enable(False)
            k = statistics.median(kernel)
            # the pair of chains (m, |m'|) advances lmax - max(m, |m'|) steps; every block of TILE_COMP components runs them again
            d = lmax - np.arange(lmax + 1, dtype=np.float64)  # lmax - m: m + 1 pairs with |m'| <= m, then lmax - |m'| for the others
            pair_steps = float(((lmax + 1 - d) * d + d * (d - 1) / 2).sum()) * -(-n // TILE_COMP)
            row = {"lmax": lmax, "ncomp": n, "angles": ANGLES, "call": summary(whole), "kernel": summary(kernel), "pair_steps": pair_steps,
                   "executed_gflop": flops / 1e9, "gflops": flops / k / 1e6, "fp64_valu_share": flops / k / 1e9 / peaks["fp64_valu_tflops"],
                   "ns_per_pair_step": k * 1e6 / pair_steps}
            rows.append(row)
            print(json.dumps(row), flush=True)
            del alm, out
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(OUT) or ".", exist_ok=True)
    with open(OUT, "w") as f:
        json.dump({"peaks": peaks, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
