"""FitsCatalog on the MI355X: hx_fits_unpack_columns against the numpy decoder bit for bit (both kernels, host and device tables, odd
widths and odd starts, the edge values of every type), the pages against the decoder with the reader thread running, and map_catalogs
from a file against map_catalogs from an ArrayCatalog of the decoder's columns, bit for bit -- plain, and as thirteen views in one pass
over the file."""

import ctypes as C
import warnings

import numpy as np
import pytest

import heracles_amd as hx
from fits_table_cases import (CATALOG_COLUMNS, CATALOG_SCALING, NBINS, SCALAR_NAMES, catalog_rows, decode, dtype_of, write_catalog_file)
from heracles_amd import _lib

pytestmark = pytest.mark.gpu

WIDTH = dtype_of(CATALOG_COLUMNS).itemsize
NROWS = 3001
NSIDE = 32


def _descr(names, columns=CATALOG_COLUMNS, scaling=CATALOG_SCALING):
    dt = dtype_of(columns)
    tform = {name: t for name, t, _ in columns}
    return [(tform[n], dt.fields[n][1], *map(float, scaling.get(n, (1, 0)))) for n in names]


def _tile_rows(width):
    """Records of one LDS tile, by the rule include/hxsht.h states; 0: read from global memory."""
    if width > 48 * 1024:
        return 0
    r = min(1024, 48 * 1024 // width)
    return r - r % 64 if r >= 64 else r


def _unpack(table, nrows, width, descr, direct=False):
    """hx_fits_unpack_columns of ``table`` (numpy bytes or a device tensor) -> [numpy column]."""
    import torch

    _lib.ensure_init()
    outs = [torch.full((nrows,), -7.0, dtype=torch.float64, device="cuda") for _ in descr]
    ptrs = (C.c_void_p * len(descr))(*[_lib.ptr(o).value for o in outs])
    offsets = np.array([d[1] for d in descr], dtype=np.int64)
    tscal = np.array([d[2] for d in descr])
    tzero = np.array([d[3] for d in descr])
    rc = _lib.load().hx_fits_unpack_columns(nrows, width, len(descr), offsets.ctypes.data, "".join(d[0] for d in descr).encode(),
                                            tscal.ctypes.data, tzero.ctypes.data, _lib.ptr(table), ptrs, 1 if direct else 0)
    _lib.check(rc)
    return [o.cpu().numpy() for o in outs]


def _misplaced(payload, shift, device):
    """The bytes of ``payload`` starting ``shift`` bytes into a larger buffer, on the host or in HBM."""
    import torch

    buf = np.zeros(len(payload) + 64, dtype=np.uint8)
    buf[shift : shift + len(payload)] = np.frombuffer(payload, dtype=np.uint8)
    if device:
        whole = torch.as_tensor(buf).cuda()
        view = whole[shift : shift + len(payload)]
        assert not len(payload) or view.data_ptr() % 16 == (whole.data_ptr() + shift) % 16
        return view
    view = buf[shift : shift + len(payload)]
    return view


@pytest.fixture(scope="module")
def rows():
    return catalog_rows(NROWS)


@pytest.mark.parametrize("variant", ["tile", "direct"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_unpack_columns_equals_numpy(rows, variant, device):
    tile = _tile_rows(WIDTH)
    assert 64 <= tile and 2 * tile + 1 < NROWS and tile * WIDTH <= 48 * 1024
    descr = _descr(SCALAR_NAMES)
    for n, first, shift in [(0, 0, 1), (1, 0, 1), (1, 5, 3), (7, 2, 5), (tile - 1, 1, 7), (tile, 3, 9), (tile + 1, 0, 15), (2 * tile + 1, 11, 13),
                            (NROWS, 0, 1), (NROWS, 0, 0), (NROWS - 1, 1, 0)]:
        page = rows[first : first + n]
        assert len(page) == n
        table = _misplaced(page.tobytes(), shift, device)
        got = _unpack(table, n, WIDTH, descr, variant == "direct")
        want = decode(page, SCALAR_NAMES)
        for name, g in zip(SCALAR_NAMES, got):
            np.testing.assert_array_equal(g, want[name], err_msg=f"{name}: {n} rows from row {first}, shift {shift}")


def test_unpack_edge_values(rows):
    """What the first rows hold, spelled out (the decoder is numpy's; these are the numbers themselves)."""
    got = dict(zip(SCALAR_NAMES, _unpack(_misplaced(rows[:8].tobytes(), 1, True), 8, WIDTH, _descr(SCALAR_NAMES))))
    assert got["ID"].tolist() == [2.0**53, -(2.0**53), 2.0**53, -(2.0**53), 2.0**63, -(2.0**63), 0.0, -1.0]  # a C cast: to nearest even
    z = got["Z"]
    assert z[0] == 2.0**-149 and z[1] == -(2.0**-149) and z[2] == 2.0**-126 and np.isnan(z[3]) and z[4] == np.inf and z[5] == -np.inf
    assert z[6] == 0 and np.signbit(z[6]) and z[7] == float(np.float32(3.4028235e38))
    assert got["FLAG_B"][:2].tolist() == [0.0, 255.0] and got["S8"][:2].tolist() == [-128.0, 127.0]
    assert got["U16"][:2].tolist() == [0.0, 65535.0] and got["FLAG_I"][:2].tolist() == [-32768.0, 32767.0]
    assert got["SCALED"][:2].tolist() == [-2147483648 * 0.01 + -3.0, 2147483647 * 0.01 + -3.0]
    j_unsigned = _unpack(_misplaced(rows[:2].tobytes(), 0, False), 2, WIDTH,
                         [("J", dtype_of(CATALOG_COLUMNS).fields["SCALED"][1], 1.0, 2147483648.0)])[0]
    assert j_unsigned.tolist() == [0.0, 4294967295.0]


@pytest.mark.parametrize("variant", ["tile", "direct"])
def test_unpack_other_widths(variant):
    """Record widths around the sizes of a tile: one byte, a multiple of 16, one that leaves a single row per tile, and one too wide
    for LDS (read from global memory whatever the variant)."""
    rng = np.random.default_rng(5)
    assert [_tile_rows(w) for w in (1, 64, 30_000, 48 * 1024 + 1)] == [1024, 768, 1, 0]
    for width, n in [(1, 2500), (64, 1601), (30_000, 5), (48 * 1024 + 1, 3)]:
        raw = rng.integers(0, 256, (n, width), dtype=np.uint8)
        if width == 1:
            descr, want = [("B", 0, 1.0, 0.0), ("L", 0, 1.0, 0.0)], [raw[:, 0].astype("f8"), (raw[:, 0] == ord("T")).astype("f8")]
        else:
            offs = [0, 3, width - 8, width - 4 - 1]
            descr = [("K", offs[0], 1.0, 0.0), ("I", offs[1], 1.0, 32768.0), ("K", offs[2], 1.0, 0.0), ("J", offs[3], 0.01, -3.0)]
            field = lambda o, dt: np.ascontiguousarray(raw[:, o : o + np.dtype(dt).itemsize]).view(dt)[:, 0].astype("f8")
            want = [field(offs[0], ">i8"), field(offs[1], ">i2") * 1.0 + 32768.0, field(offs[2], ">i8"), field(offs[3], ">i4") * 0.01 + -3.0]
        for device in (False, True):
            got = _unpack(_misplaced(raw.tobytes(), 3, device), n, width, descr, variant == "direct")
            for g, w in zip(got, want):
                np.testing.assert_array_equal(g, w, err_msg=f"width {width}")


def test_unpack_rejects_bad_arguments(rows):
    import torch

    table = _misplaced(rows[:4].tobytes(), 0, True)
    for descr in ([("A", 0, 1.0, 0.0)], [("D", WIDTH - 7, 1.0, 0.0)], [("B", -1, 1.0, 0.0)], [("B", 0, 1.0, 0.0)] * 65):
        with pytest.raises(hx.HxError):
            _unpack(table, 4, WIDTH, descr)
    host_out = np.zeros(4)
    ptrs = (C.c_void_p * 1)(host_out.ctypes.data)
    off = np.zeros(1, dtype=np.int64)
    assert _lib.load().hx_fits_unpack_columns(4, WIDTH, 1, off.ctypes.data, b"B", None, None, _lib.ptr(table), ptrs, 0) != 0
    torch.cuda.synchronize()


# ---- pages ---------------------------------------------------------------------------------------------------------------------------


def _cat_columns(pages, names):
    import torch

    pages = list(pages)
    return {n: torch.cat([p[n] for p in pages]).cpu().numpy() for n in names}, pages


@pytest.fixture(scope="module")
def catfile(tmp_path_factory):
    path = tmp_path_factory.mktemp("fitscat") / "cat.fits"
    return path, write_catalog_file(path, NROWS)


@pytest.mark.parametrize("page_size", [1, 1000, NROWS - 1, NROWS, 10 * NROWS])
def test_pages_equal_decoder(catfile, page_size):
    import torch

    path, rows = catfile
    cat = hx.FitsCatalog(path, page_size=page_size)
    got, pages = _cat_columns(cat, SCALAR_NAMES)
    want = decode(rows, SCALAR_NAMES)
    assert [p.size for p in pages] == [min(page_size, NROWS - i) for i in range(0, NROWS, page_size)]
    for p in pages[:3]:
        assert p.names == SCALAR_NAMES
        for n in SCALAR_NAMES:
            assert p[n].is_cuda and p[n].dtype == torch.float64 and p[n].is_contiguous() and p[n].ndim == 1
    for n in SCALAR_NAMES:
        np.testing.assert_array_equal(got[n], want[n], err_msg=n)
    assert cat.bytes_read == NROWS * WIDTH  # one pass, and the reader thread never went past the end


def test_requested_columns_and_cache(catfile):
    path, rows = catfile
    names = ["Z", "RA", "SCALED", "GOOD"]
    cat = hx.FitsCatalog(path, columns=names, ext="CATALOG", page_size=1200)  # three pages: all of them stay in the cache
    want = decode(rows, names)
    for _ in range(2):
        got, pages = _cat_columns(cat, names)
        assert all(p.names == names for p in pages)
        for n in names:
            np.testing.assert_array_equal(got[n], want[n], err_msg=n)
        assert cat.bytes_read == NROWS * WIDTH
    # views iterated one after the other share what was read
    for k in range(3):
        view = cat.where(f"GOOD == {k % 2}")
        got, _ = _cat_columns(view, names)
        np.testing.assert_array_equal(got["RA"], want["RA"][want["GOOD"] == k % 2])
        assert view.size == int((want["GOOD"] == k % 2).sum())
    assert cat.bytes_read == NROWS * WIDTH
    cat.release()  # the cached pages go: the next iteration reads the file again
    assert not cat._cache and cat._stage == [None, None]
    got, _ = _cat_columns(cat, names)
    np.testing.assert_array_equal(got["SCALED"], want["SCALED"])
    assert cat.bytes_read == 2 * NROWS * WIDTH
    cat.bytes_read = 0
    cat.page_size = 500  # seven pages through a cache of three: each iteration reads the file once more
    list(cat)
    list(cat)
    assert cat.bytes_read == 2 * NROWS * WIDTH


def test_selected_and_filtered_pages(catfile, tmp_path):
    """Pages are cut every page_size rows of the file, then selected and filtered."""
    nanpath = tmp_path / "nan.fits"

    def edit(r):
        r["G1"][::7] = np.nan
        r["W"][::14] = 0

    rows = write_catalog_file(nanpath, NROWS, edit=edit)
    want = decode(rows, SCALAR_NAMES)
    cat = hx.FitsCatalog(nanpath, page_size=700)
    cat.add_filter(hx.InvalidValueFilter("G1", weight="W", warn=False))
    mask = np.arange(NROWS) % 3 != 0
    view = cat.where("TOM_BIN_ID < 6")[mask]
    keep = (want["TOM_BIN_ID"] < 6) & mask & ~(np.isnan(want["G1"]) & (want["W"] != 0))
    got, pages = _cat_columns(view, SCALAR_NAMES)
    assert [p.size for p in pages] == [int(keep[i : i + 700].sum()) for i in range(0, NROWS, 700)]
    for n in SCALAR_NAMES:
        np.testing.assert_array_equal(got[n], want[n][keep], err_msg=n)
    assert view.size == int(((want["TOM_BIN_ID"] < 6) & mask).sum())  # (before the filters, as for ArrayCatalog)
    import torch

    dview = cat.where(torch.as_tensor(mask).cuda())
    np.testing.assert_array_equal(_cat_columns(dview, ["ID"])[0]["ID"], want["ID"][mask & ~(np.isnan(want["G1"]) & (want["W"] != 0))])


def test_two_million_rows(tmp_path):
    n = 2_000_003
    path = tmp_path / "large.fits"
    rows = write_catalog_file(path, n, seed=12)
    cat = hx.FitsCatalog(path, page_size=300_007)
    got, pages = _cat_columns(cat, SCALAR_NAMES)
    assert len(pages) == 7 and cat.bytes_read == n * WIDTH
    want = decode(rows, SCALAR_NAMES)
    for name in SCALAR_NAMES:
        np.testing.assert_array_equal(got[name], want[name], err_msg=name)  # (ID is random per row: the pages came in file order)


# ---- mapping -------------------------------------------------------------------------------------------------------------------------

MAPCOLS = ["RA", "DEC", "W", "G1", "G2", "TOM_BIN_ID"]


def _fields():
    m = hx.HipHealpixMapper(NSIDE, 2 * NSIDE, deconvolve=False)
    return {"POS": hx.Positions(m, "RA", "DEC", overdensity=True), "SHE": hx.Shears(m, "RA", "DEC", "G1", "-G2", "W"),
            "WHT": hx.Weights(m, "RA", "DEC", "W")}


def _visibility(seed=2):
    vis = np.random.default_rng(seed).uniform(0.5, 1.0, 12 * NSIDE**2)
    vis[:100] = 0.0
    return vis


def _same(got, want, device):
    assert list(got) == list(want) and len(got) > 0
    for key, w in want.items():
        g = got[key]
        if device:
            assert isinstance(g, hx.DeviceArray) and isinstance(w, hx.DeviceArray)
            gm, wm = dict(g.dtype.metadata), dict(w.dtype.metadata)
            g, w = g.tensor.cpu().numpy(), w.tensor.cpu().numpy()
        else:
            gm, wm = dict(g.dtype.metadata), dict(w.dtype.metadata)
            g, w = np.asarray(g), np.asarray(w)
        np.testing.assert_array_equal(g, w, err_msg=str(key))
        assert np.abs(w).max() > 0, key
        assert gm == wm and len(wm) >= 4, key


@pytest.mark.parametrize("device", [None, "cuda"])
def test_map_catalogs_from_file_equals_array_catalog(catfile, device):
    path, rows = catfile
    vis = _visibility()
    fits = hx.FitsCatalog(path, columns=MAPCOLS, page_size=700, visibility=vis, metadata={"catalog": "from-file"})
    array = hx.ArrayCatalog(decode(rows, MAPCOLS), page_size=700, visibility=vis, metadata={"catalog": "from-file"})
    got = hx.map_catalogs(_fields(), {1: fits}, device=device)
    want = hx.map_catalogs(_fields(), {1: array}, device=device)
    _same(got, want, device)
    assert fits.bytes_read == NROWS * WIDTH


@pytest.mark.parametrize("device", [None, "cuda"])
def test_thirteen_views_in_one_pass(tmp_path, device):
    path = tmp_path / "bins.fits"

    def edit(r):
        r["G1"][::11] = np.nan
        r["W"][::33] = 0

    n = 20_011
    rows = write_catalog_file(path, n, seed=13, edit=edit)
    vis = {k: _visibility(k) for k in range(NBINS)}
    bases = [hx.FitsCatalog(path, page_size=3_000), hx.ArrayCatalog(decode(rows, SCALAR_NAMES), page_size=3_000)]
    out = []
    for base in bases:
        base.add_filter(hx.InvalidValueFilter("G1", "G2", weight="W"))
        bins = {k: base.where(f"TOM_BIN_ID=={k}", visibility=vis[k]) for k in range(NBINS)}
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            out.append(hx.map_catalogs(_fields(), bins, device=device))
        assert "WARNING: catalog contains invalid values" in {str(r.message) for r in rec}
    assert len(out[0]) == 3 * NBINS
    _same(out[0], out[1], device)
    assert bases[0].bytes_read == n * WIDTH  # one context holds the three fields: one pass over the file, not one per view
