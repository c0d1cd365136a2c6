"""HEALPix map2alm (niter = 0) and alm2map of ONE (Q, U) field resident in HBM, by spin weight: spin 2 on its own kernels (the
yardstick), spins 1 and 3 on the run-time-spin sweeps, and spin 2 through those sweeps (HX_SPIN_GENERIC=1).  Every variant is warmed
up, the variants alternate within each of REPS rounds, and the result is the median and min .. max per variant; a call is timed by
the host clock around a device synchronise.  NSIDE, LMAX, REPS and OUT (the JSON file, default profiles/healpix_spin.json) come from
the environment."""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch, heracles_amd as hx

hx.init(0)
nside, lmax, reps = int(os.environ.get("NSIDE", 4096)), int(os.environ.get("LMAX", 6144)), int(os.environ.get("REPS", 9))
out_path = os.environ.get("OUT", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "healpix_spin.json"))
plan = hx.get_plan(nside, lmax)
g = torch.Generator(device="cuda").manual_seed(1)
maps = torch.randn((2, plan.npix), dtype=torch.float64, device="cuda", generator=g)
alms = torch.empty((2, plan.nlm), dtype=torch.complex128, device="cuda")
back = torch.empty_like(maps)
variants = [("spin2", 2, False), ("spin1", 1, False), ("spin3", 3, False), ("spin2_generic", 2, True)]


def call(fn, generic):
    if generic:
        os.environ["HX_SPIN_GENERIC"] = "1"
    try:
        hx._lib.synchronize(); t = time.perf_counter()
        fn()
        hx._lib.synchronize()
        return (time.perf_counter() - t) * 1e3
    finally:
        os.environ.pop("HX_SPIN_GENERIC", None)


times = {name: {"map2alm": [], "alm2map": []} for name, _, _ in variants}
ref = {}
for rep in range(-1, reps):  # (round -1: warm-up, tables and task sets of every weight; also the results that are compared below)
    for name, s, generic in variants:
        ta = call(lambda: plan.map2alm(maps, s, out=alms), generic)
        if rep < 0 and s == 2:
            ref[name] = alms.clone()
        ts = call(lambda: plan.alm2map(alms, s, out=back), generic)
        if rep < 0 and s == 2:
            ref[name + "_map"] = back.clone()
        if rep >= 0:
            times[name]["map2alm"].append(ta)
            times[name]["alm2map"].append(ts)

rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
res = {"nside": nside, "lmax": lmax, "reps": reps, "device": torch.cuda.get_device_name(0), "unit": "ms per call, one (Q, U) field resident in HBM",
       "spin2_generic_vs_spin2": {"map2alm": rel(ref["spin2_generic"], ref["spin2"]), "alm2map": rel(ref["spin2_generic_map"], ref["spin2_map"])},
       "calls": {name: {k: {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)} for k, v in d.items()}
                 for name, d in times.items()}}
for name, d in res["calls"].items():
    print(name, {k: f"{v['median']:.2f} ({v['min']:.2f} .. {v['max']:.2f})" for k, v in d.items()}, flush=True)
print("spin 2 through the run-time-spin sweeps against its own kernels:", res["spin2_generic_vs_spin2"], flush=True)
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
