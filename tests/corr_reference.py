"""Ground truth of the Cl <-> xi transforms (numpy only, no GPU, no oracle): the un-normalised Wigner d functions P_l = d^l_00,
d^l_22, d^l_2-2, d^l_20 by the three-term recursion in l from the closed-form start at l = max(|a|, |b|), in np.longdouble, at
float64 nodes.  The kernels under test and the oracle use closed forms in P_l and P_l' instead (heracles/transforms.py:46-112), which
cancel towards x -> +-1; the recursion does not, so it can measure both.  The sums follow heracles/transforms.py:115-204: factor
(2 l + 1) / 4 pi, polarisation from l = 2, T2 +- T4, the final 2 pi.

Everything streams over l: an (lmax + 1, n) long-double table is never held (600 MB per function at lmax 6144).  Results stay long
double so that the caller subtracts before rounding."""

import numpy as np

LD = np.longdouble
EPS_LD = float(np.finfo(LD).eps)
if EPS_LD > 2e-19:
    raise RuntimeError(f"np.longdouble has eps {EPS_LD:.3g} on this platform (an 80-bit type with eps 1.08e-19 is needed): "
                       "a truth in double precision proves nothing about a double-precision kernel")

FAMILIES = ((0, 0), (2, 2), (2, -2), (2, 0))  # table order of k_corr_tables: P, d22, d2m2, d20
PI_LD = LD("3.14159265358979323846264338327950288")


def recursion_rows(lmax, x, num, sqrt, zero):
    """Generator over l = 0 .. lmax of (P_l, d22_l, d2m2_l, d20_l) at x, in whatever arithmetic `num` (number from an int), `sqrt` and
    the type of x provide: np.longdouble arrays here, mpmath numbers in tests/test_corr_reference.py.  `zero` is what l < 2 yields for
    the spin-2 families.  d^{l+1} = c1 d^l - c2 d^{l-1} with
        c1 = (2l+1) (l (l+1) x - a b) / den,  c2 = (l+1) sqrt((l^2 - a^2)(l^2 - b^2)) / den,  den = l sqrt(((l+1)^2 - a^2)((l+1)^2 - b^2))."""
    one = num(1)
    omx, opx = one - x, one + x
    start = {(0, 0): one + zero, (2, 2): opx * opx / num(4), (2, -2): omx * omx / num(4), (2, 0): sqrt(num(6)) / num(4) * omx * opx}
    prev = {f: zero for f in FAMILIES}
    cur = {f: zero for f in FAMILIES}
    for l in range(lmax + 1):
        for f in FAMILIES:
            a, b = f
            l0 = max(abs(a), abs(b))
            if l < l0:
                continue
            if l == l0:
                cur[f] = start[f]
                continue
            k = l - 1  # step k -> k + 1 = l
            if k == 0:
                nxt = x * cur[f]
            else:
                # (each integer factor is below 2^53; their product is formed in the working precision)
                den = num(k) * sqrt(num(l * l - a * a) * num(l * l - b * b))
                c1 = num(2 * k + 1) * (num(k * l) * x - num(a * b)) / den
                c2 = num(l) * sqrt(num(k * k - a * a) * num(k * k - b * b)) / den
                nxt = c1 * cur[f] - c2 * prev[f]
            prev[f], cur[f] = cur[f], nxt
        yield tuple(cur[f] for f in FAMILIES)


def wigner_rows(lmax, x):
    """Generator over l = 0 .. lmax yielding the long-double rows (P_l, d^l_22, d^l_2-2, d^l_20) at all nodes x (float64 in)."""
    x = np.asarray(x, dtype=np.float64).astype(LD)
    return recursion_rows(int(lmax), x, LD, np.sqrt, np.zeros(x.shape, dtype=LD))


def table_truth(lmax, x, ls):
    """The four rows at the multipoles `ls`: long double array (len(ls), 4, len(x))."""
    ls = [int(l) for l in ls]
    where = {}
    for i, l in enumerate(ls):
        where.setdefault(l, []).append(i)
    out = np.zeros((len(ls), 4, len(x)), dtype=LD)
    for l, rows in enumerate(wigner_rows(max(ls) if ls else -1, x)):
        for i in where.get(l, ()):
            for ix in range(4):
                out[i, ix] = rows[ix]
    return out


def cl2corr_coefficients(cls):
    """c[spec][l][ix] of xi_ix = sum_l c_ix T_ix: (2l+1)/4pi times TT, EE+BB, EE-BB, TE, zero below l = 2 for the last three."""
    cls = np.asarray(cls, dtype=np.float64).astype(LD)
    f = (2 * np.arange(cls.shape[1]).astype(LD) + 1) / (4 * PI_LD)
    c = np.stack([cls[..., 0], cls[..., 1] + cls[..., 2], cls[..., 1] - cls[..., 2], cls[..., 3]], axis=-1) * f[None, :, None]
    c[:, :2, 1:] = 0
    return c


def cl2corr_truth(cls, x):
    """xi[spec][k][ix] (T, Q+U, Q-U, cross) of cls[spec][l][ix] (TT, EE, BB, TE) at the nodes x, long double.  Spectra that vanish at a
    multipole cost nothing there, so single-l probes are cheap."""
    c = cl2corr_coefficients(cls)
    nspec, L, _ = c.shape
    out = np.zeros((nspec, len(x), 4), dtype=LD)
    live = [[np.flatnonzero(c[:, l, ix]) for ix in range(4)] for l in range(L)]
    for l, rows in enumerate(wigner_rows(L - 1, x)):
        for ix in range(4):
            s = live[l][ix]
            if s.size:
                out[s, :, ix] += c[s, l, ix][:, None] * rows[ix][None, :]
    return out


def corr2cl_truth(corrs, x, w, lmax=None):
    """cls[spec][l][ix] (TT, EE, BB, TE), l = 0 .. lmax, of corrs[spec][k][ix] given at the nodes x with weights w, long double.  lmax
    defaults to len(x) - 1; with an input that vanishes outside a few nodes, pass those nodes only and lmax explicitly."""
    if lmax is None:
        lmax = len(x) - 1
    corrs = np.asarray(corrs, dtype=np.float64).astype(LD)
    wl = np.asarray(w, dtype=np.float64).astype(LD)
    nspec = corrs.shape[0]
    a0 = corrs[..., 0] * wl
    a1 = corrs[..., 1] * wl / 2
    a2 = corrs[..., 2] * wl / 2
    a3 = corrs[..., 3] * wl
    out = np.zeros((nspec, lmax + 1, 4), dtype=LD)
    for l, (P, d22, d2m2, d20) in enumerate(wigner_rows(lmax, x)):
        out[:, l, 0] = a0 @ P
        if l >= 2:
            t2, t4 = a1 @ d22, a2 @ d2m2
            out[:, l, 1] = t2 + t4
            out[:, l, 2] = t2 - t4
            out[:, l, 3] = a3 @ d20
    return 2 * PI_LD * out


# ---- inputs and error measures shared by the CPU and the GPU tests ---------------------------------------------------------------
def red_spectra(rng, lmax, nspec=1):
    return rng.standard_normal((nspec, lmax + 1, 4)) / (1.0 + np.arange(lmax + 1))[None, :, None] ** 2


def white_spectra(rng, lmax, nspec=1):
    return rng.choice([-1.0, 1.0], (nspec, lmax + 1, 4)) * rng.uniform(0.5, 1.5, (nspec, lmax + 1, 4))


def probe_spectra(lmax, ls):
    """TT = EE = TE = 4 pi / (2 l + 1) at one l, BB = 0: xi is then the table row (P, d22, d2m2, d20) at that l."""
    out = np.zeros((len(ls), lmax + 1, 4))
    for i, l in enumerate(ls):
        out[i, l, [0, 1, 3]] = 4.0 * np.pi / (2.0 * l + 1.0)
    return out


def indser_of(x):
    """Number of multipoles from l = 2 that take the small-angle series at node x (transforms.py:88-96), before clipping to lmax."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(divide="ignore"):
        v = np.sqrt((400.0 + 3.0 / (1.0 - x * x)) / 150.0).astype(np.int64) - 1
    return np.where(x > 0.998, np.maximum(v, 0), 0)


def probe_multipoles(rng, lmax, x):
    """All l < 8, 16 random l, the multipoles around the largest series switch-over, lmax - 1, lmax."""
    ls = set(range(min(8, lmax + 1))) | {lmax - 1, lmax}
    ls |= set(rng.integers(0, lmax + 1, 16).tolist())
    sw = int(indser_of(x).max()) + 2
    ls |= {sw - 2, sw - 1, sw, sw + 1}
    return sorted(l for l in ls if 0 <= l <= lmax)


def node_bands(x):
    """The 8 nodes nearest x = -1, the 8 nearest x = +1, the remaining nodes with x > 0.998, the rest (x ascending)."""
    n = len(x)
    idx = np.arange(n)
    lo = idx < min(8, n)
    hi = (idx >= n - 8) & ~lo
    ser = (np.asarray(x) > 0.998) & ~lo & ~hi
    return {"x->-1": lo, "x->+1": hi, "series": ser, "rest": ~(lo | hi | ser)}


def ell_bands(lmax):
    """l < 2, 2 <= l < 64, then the rest in quarters."""
    l = np.arange(lmax + 1)
    bands = {"l<2": l < 2, "2<=l<64": (l >= 2) & (l < 64)}
    if lmax >= 64:
        edges = np.linspace(64, lmax + 1, 5).astype(int)
        for q in range(4):
            bands[f"q{q + 1}"] = (l >= edges[q]) & (l < edges[q + 1])
    return bands


def cl2corr_floor(cls):
    """16 eps sum_l |c_ix[l]| per (spec, column): the rounding floor of the sum itself (|T| <= 1)."""
    return 16 * np.finfo(np.float64).eps * np.abs(cl2corr_coefficients(cls)).sum(axis=1).astype(np.float64)


def corr2cl_floor(corrs, w):
    """16 eps 2 pi sum_k w_k |xi_k| per (spec, column); the two polarisation columns each take half of both polarisation terms."""
    a = 2 * np.pi * (np.abs(np.asarray(corrs)) * np.asarray(w)[None, :, None]).sum(axis=1)
    pol = 0.5 * (a[:, 1] + a[:, 2])
    return 16 * np.finfo(np.float64).eps * np.stack([a[:, 0], pol, pol, a[:, 3]], axis=-1)


def yardstick(got, ref, truth, floor, bands, axis_specs=None):
    """Per (column, band): E_got = max |got - truth|, E_ref = max |ref - truth| over the specs in `axis_specs` (all by default) and the
    band, and the bound 8 E_ref + max floor.  got / ref / truth: [spec][k or l][4]; floor: [spec][4].  Returns a list of
    (column, band, E_got, E_ref, bound); asserts nothing."""
    specs = np.arange(got.shape[0]) if axis_specs is None else np.asarray(axis_specs)
    dg = np.abs(got[specs].astype(LD) - truth[specs]).astype(np.float64)
    dr = np.abs(ref[specs].astype(LD) - truth[specs]).astype(np.float64)
    rows = []
    for ix in range(4):
        for name, m in bands.items():
            if not m.any():
                continue
            eg, er = dg[:, m, ix].max(), dr[:, m, ix].max()
            rows.append((ix, name, eg, er, 8.0 * er + floor[specs, ix].max()))
    return rows


def format_rows(tag, rows):
    cols = ("T", "Q+U", "Q-U", "X")
    return "\n".join(f"{tag} {cols[ix]:>3} {name:>8}: E_got {eg:.2e} E_ref {er:.2e} ratio {eg / er if er else float('inf'):.2f} bound {b:.2e}"
                     for ix, name, eg, er, b in rows)


# ---- norms in which the reference vectors of tests/golden/reference_transforms.npz are compared at size --------------------------
def dev_xi(got, ref):
    """max |d| / max |ref| per column of a correlation function [k][4] (element-wise rtol fails at its zero crossings)."""
    return np.abs(np.asarray(got) - ref).max(axis=0) / np.abs(ref).max(axis=0)


def dev_cl(got, ref):
    """max |d| (1 + l)^2 per column of a red spectrum [l][4] coming back."""
    return (np.abs(np.asarray(got) - ref) * (1.0 + np.arange(ref.shape[0]))[:, None] ** 2).max(axis=0)


def dev_rel(got, ref):
    """max |d| / max |ref| over a whole array."""
    return float(np.abs(np.asarray(got) - ref).max() / np.abs(ref).max())


def dev_back(got, ref):
    """max |d| (1 + l)^2 over an array whose last axis is l."""
    return float((np.abs(np.asarray(got) - ref) * (1.0 + np.arange(ref.shape[-1])) ** 2).max())
