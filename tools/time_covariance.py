"""Timing of the covariance estimators at the production data vector: 10 spin-0 + 10 spin-2 maps, 210 spectra, 31 l bins
(N = 14725), n = 128 delete-1 samples; the delete-2 correction at Njk = 128 (n = 8128).  Prints one JSON line: packing + upload,
kernel time per family (HIP events of the library stream), dict assembly, and flatten(gaussian_covariance(...)) on the host.

    python tools/time_covariance.py [--njk 128] [--nell 31] [--skip-delete2]
"""

import argparse
import itertools
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--njk", type=int, default=128)
    ap.add_argument("--nell", type=int, default=31)
    ap.add_argument("--skip-delete2", action="store_true")
    args = ap.parse_args()

    import torch

    import heracles_amd as hx
    from heracles_amd import _lib
    from heracles_amd import covariance as cv

    hx.init(0)
    L, njk = args.nell, args.njk
    maps = [("POS", i) for i in range(10)] + [("SHE", i) for i in range(10)]
    keys = [(a, b, i, j) for (a, i), (b, j) in itertools.combinations_with_replacement(maps, 2)]
    spin = {"POS": 0, "SHE": 2}
    rng = np.random.default_rng(0)
    shape = {k: tuple(2 for f in k[:2] if f == "SHE") + (L,) for k in keys}
    base = {k: 1.0 + rng.random(shape[k]) for k in keys}

    def sample(scale, meta=False):
        out = {}
        for k in keys:
            arr = base[k] * (1 + scale * rng.standard_normal(shape[k]))
            if meta:
                hx.update_metadata(arr, bias=0.01 if (k[0] == k[1] and k[2] == k[3]) else 0.0)
            out[k] = hx.Result(arr, spin=(spin[k[0]], spin[k[1]]), axis=-1)
        return out

    cls0 = sample(0.0, meta=True)
    cls1 = {(r,): sample(0.05) for r in range(1, njk + 1)}
    lay = cv._Layout(cls0)
    res = {"N": lay.n, "njk": njk, "nell": L}

    def profiled(fn):
        _lib.profile_enable(True)
        _lib.profile_reset()
        out = fn()
        _lib.synchronize()
        fams = {}
        for name in ("cov_center", "cov_gram", "cov_delete2_q", "cov_shrink_sums"):
            cnt, ms = _lib.profile_get(name)
            if cnt:
                fams[name] = round(ms, 3)
        _lib.profile_enable(False)
        return out, fams

    # packing and upload
    t0 = time.perf_counter()
    X = lay.pack(list(cls1.values()))
    res["pack_s"] = round(time.perf_counter() - t0, 3)
    t0 = time.perf_counter()
    dx = torch.from_numpy(X).cuda()
    torch.cuda.synchronize()
    res["h2d_s"] = round(time.perf_counter() - t0, 4)
    del dx
    cv._gram(X[:, :64], None, 1.0)  # warm-up of the code objects
    # jackknife covariance: the Gram family, and the dict assembly on the host
    alpha = cv._nd_alpha(njk, 1)
    C, fams = profiled(lambda: cv._gram(X, None, alpha))
    res["gram_kernels_ms"] = fams
    t0 = time.perf_counter()
    first = next(iter(cls1.values()))
    cov = {}
    for k1, k2 in itertools.combinations_with_replacement(lay.keys, 2):
        key, r = cv._cov_result(first, k1, k2, lay.block(C, k1, k2))
        cov[key] = r
    res["dict_assembly_s"] = round(time.perf_counter() - t0, 3)
    t0 = time.perf_counter()
    cov = hx.jackknife_covariance(cls1, nd=1)
    res["jackknife_covariance_s"] = round(time.perf_counter() - t0, 3)
    del cov, C
    # shrinkage sums against a dense device target
    N = lay.n
    idx = torch.arange(N, device="cuda", dtype=torch.float64)
    T = torch.pow(0.9, (idx[:, None] - idx[None, :]).abs()) + 0.0
    del idx
    lam, fams = profiled(lambda: hx.shrinkage_factor(cls1, T))
    res["shrink_kernels_ms"] = fams
    res["lambda"] = lam
    del T
    torch.cuda.empty_cache()
    # the Gaussian target on the host
    t0 = time.perf_counter()
    g = hx.gaussian_covariance(cls0)
    res["gaussian_covariance_s"] = round(time.perf_counter() - t0, 3)
    t0 = time.perf_counter()
    Tg = hx.flatten(g, order=lay.keys)
    res["flatten_gaussian_s"] = round(time.perf_counter() - t0, 3)
    del g, Tg
    if not args.skip_delete2:
        pairs = np.array(list(itertools.combinations(range(njk), 2)), dtype=np.int32)
        m = len(pairs)
        c0 = lay.pack([cls0])[0]
        c1 = X
        t0 = time.perf_counter()
        c2 = c0 * (1 + 0.01 * rng.standard_normal((m, N)))
        res["delete2_samples_s"] = round(time.perf_counter() - t0, 3)
        nd = N // L
        perm = (np.arange(nd)[None, :] * L + np.arange(L)[:, None]).reshape(-1).astype(np.int32)
        bstart = (np.arange(L + 1) * nd).astype(np.int32)
        t0 = time.perf_counter()
        _, fams = profiled(lambda: cv._delete2_q(njk, c0, c1, c2, pairs, perm, bstart, cv._nd_alpha(m, 2)))
        res["delete2_call_s"] = round(time.perf_counter() - t0, 3)
        res["delete2_m"] = m
        res["delete2_kernels_ms"] = fams
    print(json.dumps(res))


if __name__ == "__main__":
    main()
