"""Throughput of the point transform at the bench's band limit, device-resident points: the adjoint (hx_pointsht_adjoint, values -> alm),
the forward direction (hx_pointsht_synthesis, alm -> values), or both on the same points in one run, alternating.
From the environment: LMAX, NPOINTS (comma-separated), SPINS (comma-separated spin weights, default 0,2; any s >= 1 is one (Q, U)
field), DIRECTION = adjoint | synthesis | both (default adjoint), REPEATS (default 5 timed calls per direction, and as many profiled).
Wall times are taken with the profile scopes off, each call ending in a synchronise; the scope times (nufft_spread, nufft_fft, ... /
nufft_fft_syn, nufft_gather, legendre_synthesis) come from calls of their own.  Every figure is the median over the repeats, with the
smallest and largest in brackets.  With DIRECTION=both a last line per case compares nufft_gather with nufft_spread."""
import os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch, heracles_amd as hx

SCOPES = {
    "adjoint": ("nufft_sort", "nufft_spread", "nufft_fft", "fourier_combine", "legendre_analysis", "alm_reduce"),
    "synthesis": ("nufft_sort", "legendre_synthesis", "nufft_fft_syn", "nufft_gather"),
}

hx.init(0)
lmax = int(os.environ.get("LMAX", 6144))
direction = os.environ.get("DIRECTION", "adjoint")
if direction not in ("adjoint", "synthesis", "both"):
    raise SystemExit("DIRECTION=adjoint|synthesis|both")
directions = ("adjoint", "synthesis") if direction == "both" else (direction,)
repeats = int(os.environ.get("REPEATS", 5))
sht = hx.PointSHT(lmax)
print("lmax", lmax, "rings on the circle", sht.nrings_circle, "grid", sht.ngrid, "kernel width", sht.kernel_width, flush=True)
g = torch.Generator(device="cuda").manual_seed(1)


def med(xs):
    return f"{statistics.median(xs):.1f} [{min(xs):.1f}, {max(xs):.1f}]"


for n in [int(float(x)) for x in os.environ.get("NPOINTS", "1e6,1e7,1e8").split(",")]:
    loc = torch.empty((n, 2), dtype=torch.float64, device="cuda")
    loc[:, 0] = torch.acos(torch.rand(n, dtype=torch.float64, device="cuda", generator=g) * 2 - 1)
    loc[:, 1] = torch.rand(n, dtype=torch.float64, device="cuda", generator=g) * 6.283185307179586
    for spin in [int(x) for x in os.environ.get("SPINS", "0,2").split(",")]:
        nc = 1 if spin == 0 else 2
        v = torch.randn((nc, n), dtype=torch.float64, device="cuda", generator=g)
        alm = sht.adjoint_synthesis(loc, v, spin=spin)  # (also the warm-up of the adjoint; a band-limited field for the forward direction)
        val = torch.empty_like(v)
        call = {
            "adjoint": lambda: sht.adjoint_synthesis(loc, v, spin=spin, out=alm_out),
            "synthesis": lambda: sht.synthesis(loc, alm, spin=spin, out=val),
        }
        alm_out = torch.empty_like(alm)
        for d in directions:
            call[d]()
        wall = {d: [] for d in directions}
        for _ in range(repeats):
            for d in directions:
                torch.cuda.synchronize(); t = time.perf_counter()
                call[d]()
                torch.cuda.synchronize(); wall[d].append((time.perf_counter() - t) * 1e3)
        parts = {d: {k: [] for k in SCOPES[d]} for d in directions}
        hx._lib.profile_enable(True)
        for _ in range(repeats):
            for d in directions:
                hx._lib.profile_reset()
                call[d]()
                torch.cuda.synchronize()
                for k in SCOPES[d]:
                    parts[d][k].append(hx._lib.profile_get(k)[1])
        hx._lib.profile_enable(False)
        for d in directions:
            ms = statistics.median(wall[d])
            print(f"n={n:.0e} spin {spin} {d}: {med(wall[d])} ms = {n/ms/1e3:.1f} Mpoints/s", {k: med(x) for k, x in parts[d].items()}, flush=True)
        if direction == "both":
            gather, spread = statistics.median(parts["synthesis"]["nufft_gather"]), statistics.median(parts["adjoint"]["nufft_spread"])
            print(f"n={n:.0e} spin {spin}: nufft_gather / nufft_spread = {gather / spread:.3f}", flush=True)
