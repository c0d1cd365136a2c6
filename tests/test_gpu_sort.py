"""The stable LSD radix sort of heracles_amd/csrc/hx_sort.h against an independent stable sort, called exactly as production calls it
through the probe tests/csrc/libhxsortprobe.so (built by __graft_entry__.build(); no sort logic of its own): radix_sort_pairs<unsigned>
(tile order of the point transform), radix_sort_pairs<long long> (pixel and view keys beyond 32 bits) and radix_sort_pairs_narrow (pixel
and view keys that fit 32 bits).

``end_bit = b``: the pairs come out stably ordered by ``key & (2^b - 1)``; bits at and above b do not influence the order, the two
full-width routines carry them through, the narrow one returns ``(unsigned)key``.  The values are the input indices, so their equality
with the reference's permutation IS the stability check.  Reference: numpy's stable argsort on the host, torch's stable sort on the
device for the 33 554 433-key case.  Every assertion is exact equality.

Sizes follow the constants of hx_sort.h: waves of 64, wave segments of 1024, tiles of 4096, scan tiles of 2048 counts (n = 32768 is
exactly one), 1024 threads in k_scan_top (more than one block sum per thread from 8193 tiles: n = 8192 * 4096 + 1).

Left unpinned: n near 2^32, where gdelta in k_sort_scatter wraps modulo 2^32 (its comment) -- tens of GB of pairs, not a test of seconds."""

import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROUTINES = ("u32", "narrow", "i64")
END_BITS = {"u32": (1, 7, 8, 9, 16, 17, 18, 24, 26, 28, 30, 32), "narrow": (1, 7, 8, 9, 16, 17, 18, 24, 26, 28, 30, 32), "i64": (30, 33, 36, 40)}
EDGES = (1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097)
SIZES = EDGES + (32768, 32769, 100_003)
N_MID = 100_003
N_TOP = 8192 * 4096 + 1  # 8193 tiles, 1025 block sums: k_scan_top takes two per thread
U64 = np.uint64


@pytest.fixture(scope="module")
def probe():
    from heracles_amd import _lib

    _lib.load()  # first: torch's HIP runtime has to be the resident one
    _lib.ensure_init()
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libhxsortprobe.so")
    if not os.path.exists(path):
        pytest.fail(f"{path} not found: __graft_entry__.build() builds it (make -C tests/csrc)")
    lib = ctypes.CDLL(path)
    for name in ("hxprobe_sort_u32", "hxprobe_sort_i64", "hxprobe_sort_narrow"):
        f = getattr(lib, name)
        f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_ulonglong, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        f.restype = ctypes.c_int
    return lib


def _sort_device(probe, routine, dkeys, dvals, end_bit):
    """dkeys: int32 (bit patterns of the unsigned keys) for u32, int64 otherwise; dvals: int32.  Device tensors in and out."""
    import torch

    from heracles_amd import _lib

    n = dkeys.numel()
    wide_out = routine == "i64"
    out_k = torch.full((n,), -1, dtype=torch.int64 if wide_out else torch.int32, device="cuda")
    out_v = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    f = {"u32": probe.hxprobe_sort_u32, "i64": probe.hxprobe_sort_i64, "narrow": probe.hxprobe_sort_narrow}[routine]
    _lib.check(f(_lib.ptr(dkeys), _lib.ptr(dvals), n, int(end_bit), _lib.ptr(out_k), _lib.ptr(out_v)))
    return out_k, out_v


def _check_host(probe, routine, keys, end_bit, twice=False):
    """keys: uint64 on the host (below 2^32 for u32).  Compares with numpy's stable argsort of key & mask."""
    import torch

    n = keys.size
    assert keys.dtype == U64 and (routine != "u32" or int(keys.max()) < 2**32)
    mask = U64((1 << end_bit) - 1)
    order = np.argsort(keys & mask, kind="stable")
    want_k = keys[order] if routine == "i64" else keys[order] & U64(0xFFFFFFFF)
    hk = keys.astype(np.uint32).view(np.int32) if routine == "u32" else keys.view(np.int64)
    dkeys = torch.as_tensor(np.ascontiguousarray(hk), device="cuda")
    dvals = torch.arange(n, dtype=torch.int32, device="cuda")
    keep_k, keep_v = dkeys.clone(), dvals.clone()
    out_k, out_v = _sort_device(probe, routine, dkeys, dvals, end_bit)
    got_k = out_k.cpu().numpy().view(U64 if routine == "i64" else np.uint32).astype(U64)
    got_v = out_v.cpu().numpy().astype(np.int64)
    where = f"{routine} n={n} end_bit={end_bit}"
    np.testing.assert_array_equal(got_v, order, err_msg=where + " (values: the stable permutation)")
    np.testing.assert_array_equal(got_k, want_k, err_msg=where + " (keys)")
    assert torch.equal(dkeys, keep_k) and torch.equal(dvals, keep_v), where + ": the probe's inputs were written"
    if twice:
        again_k, again_v = _sort_device(probe, routine, dkeys, dvals, end_bit)
        assert torch.equal(again_k, out_k) and torch.equal(again_v, out_v), where + ": second run differs"


def _uniform(rng, n, b):
    return rng.integers(0, 1 << b, n, dtype=U64)


def _width(routine):
    return 32 if routine == "u32" else 64


# ---- key patterns: (rng, n, end_bit, routine) -> uint64 keys ------------------------------------------------------------------------------
def _p_uniform(rng, n, b, routine):
    return _uniform(rng, n, b)


def _p_all_equal(rng, n, b, routine):
    return np.full(n, int(rng.integers(0, 1 << b)), dtype=U64)


def _p_two_values(rng, n, b, routine):
    base = int(rng.integers(0, 1 << b)) & ~(1 << (b - 1))
    return U64(base) | (rng.integers(0, 2, n, dtype=U64) << U64(b - 1))


def _p_ascending(rng, n, b, routine):
    # non-decreasing over the whole range of b bits (strictly increasing where 2^b >= n); Python integers: no overflow at b = 40
    return np.array([(i << b) // n for i in range(n)], dtype=U64) if n < 5000 else ((np.arange(n, dtype=np.float64) * (2.0**b / n)).astype(U64))


def _p_descending(rng, n, b, routine):
    return np.ascontiguousarray(_p_ascending(rng, n, b, routine)[::-1])


def _p_multiples_of_256(rng, n, b, routine):
    return (_uniform(rng, n, b) >> U64(8)) << U64(8)  # the first digit is constant


def _p_crowded(rng, n, b, routine):
    k = _uniform(rng, n, b)
    k[rng.random(n) < 1.0 / 3.0] = U64(int(rng.integers(0, 1 << b)))  # the crowded pixel
    return k


def _p_high_bits(rng, n, b, routine):
    # random bits above end_bit: ignored for the order, preserved in the output (nothing above bit 31 for the 32-bit keys)
    w = _width(routine)
    if b >= w:
        return _uniform(rng, n, b)
    high = rng.integers(0, 1 << (w - b), n, dtype=U64) if w - b < 64 else rng.integers(0, 2**64, n, dtype=U64, endpoint=False)
    return _uniform(rng, n, b) | (high << U64(b))


PATTERNS = {"uniform": _p_uniform, "all_equal": _p_all_equal, "two_values": _p_two_values, "ascending": _p_ascending,
            "descending": _p_descending, "multiples_of_256": _p_multiples_of_256, "crowded": _p_crowded, "high_bits": _p_high_bits}


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("routine", ROUTINES)
def test_sizes_against_stable_argsort(probe, routine, n):
    """Uniform keys over all b bits at every size edge and every end_bit of the routine."""
    rng = np.random.default_rng(1000 + n)
    for b in END_BITS[routine]:
        _check_host(probe, routine, _uniform(rng, n, b), b)


@pytest.mark.parametrize("pattern", list(PATTERNS))
@pytest.mark.parametrize("routine", ROUTINES)
def test_key_patterns_against_stable_argsort(probe, routine, pattern):
    """Every key pattern at n = 100 003 with every end_bit, and at the partial-wave, -segment and -tile edges with a subset."""
    rng = np.random.default_rng(sorted(PATTERNS).index(pattern) + 17)
    make = PATTERNS[pattern]
    for b in END_BITS[routine]:
        _check_host(probe, routine, make(rng, N_MID, b, routine), b)
    for n in (63, 65, 1025, 4097):
        for b in END_BITS[routine][::3]:
            _check_host(probe, routine, make(rng, n, b, routine), b)


def test_invalid_point_key_among_small_ones(probe):
    """k_nufft_keys gives invalid points the key 0xffffffff: with end_bit 32 they sort behind every tile, in input order."""
    rng = np.random.default_rng(5)
    for n in EDGES + (N_MID,):
        keys = rng.integers(0, 561, n, dtype=U64)
        keys[rng.random(n) < 0.01] = U64(0xFFFFFFFF)
        keys[n // 2] = U64(0xFFFFFFFF)
        _check_host(probe, "u32", keys, 32)


@pytest.mark.parametrize("end_bit", END_BITS["narrow"])
def test_npix_sentinel_among_pixel_keys(probe, end_bit):
    """hx_catmap_page gives dropped rows the key npix, the largest key of a page.  Here: the sentinel 2^(end_bit - 1) among keys below it
    (in these keys it alone has the top bit set): the sentinels sort behind every other key, in input order."""
    rng = np.random.default_rng(end_bit)
    top = 1 << (end_bit - 1)
    for n in (65, 4097, N_MID):
        keys = rng.integers(0, top, n, dtype=U64)
        keys[rng.random(n) < 0.1] = U64(top)
        keys[n // 2] = U64(top)
        _check_host(probe, "narrow", keys, end_bit)


@pytest.mark.parametrize("routine", ROUTINES)
def test_repeatable(probe, routine):
    rng = np.random.default_rng(9)
    for b in END_BITS[routine][-3:]:
        _check_host(probe, routine, _p_crowded(rng, N_MID, b, routine), b, twice=True)
        _check_host(probe, routine, _p_crowded(rng, 4097, b, routine), b, twice=True)


@pytest.mark.parametrize("routine,end_bit", [("u32", 26), ("narrow", 28), ("i64", 33)])
def test_two_block_sums_per_scan_thread(probe, routine, end_bit):
    """n = 8192 * 4096 + 1: 8193 tiles, 1025 block sums, so every thread of k_scan_top takes two (the branch production reaches above
    33.5 M rows per page).  Keys with random bits above end_bit, generated on the device; reference: torch's stable sort there."""
    import torch

    g = torch.Generator(device="cuda").manual_seed(end_bit)
    width = 32 if routine == "u32" else 62
    keys = torch.randint(0, 2**width, (N_TOP,), dtype=torch.int64, device="cuda", generator=g)
    if routine != "u32":
        keys[::2] |= -(2**63)  # the sign bit too
    vals = torch.arange(N_TOP, dtype=torch.int32, device="cuda")
    _, order = torch.sort(keys & ((1 << end_bit) - 1), stable=True)
    want_k = keys[order] if routine == "i64" else keys[order] & 0xFFFFFFFF
    dkeys = keys.view(torch.int32)[::2].contiguous() if routine == "u32" else keys  # the low words (little endian)
    out_k, out_v = _sort_device(probe, routine, dkeys, vals, end_bit)
    assert torch.equal(out_v.to(torch.int64), order), "values: the stable permutation"
    del order
    got_k = out_k if routine == "i64" else out_k.to(torch.int64) & 0xFFFFFFFF
    assert torch.equal(got_k, want_k), "keys"
    del got_k, want_k
    again_k, again_v = _sort_device(probe, routine, dkeys, vals, end_bit)
    assert torch.equal(again_k, out_k) and torch.equal(again_v, out_v), "second run differs"
