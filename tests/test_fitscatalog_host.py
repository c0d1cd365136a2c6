"""FitsCatalog without a GPU: what it learns from the headers (columns, offsets, types, scaling, size), the choice of the HDU, the
errors for what it does not read, and that nothing touches the file before the first use."""

import copy
import gzip

import numpy as np
import pytest

import heracles_amd as hx
from fits_table_cases import (CATALOG_COLUMNS, CATALOG_SCALING, SCALAR_NAMES, dtype_of, table_header, write_catalog_file,
                              write_primary, write_table)
from heracles_amd.fits import _card

NROWS = 1237


@pytest.fixture(scope="module")
def catfile(tmp_path_factory):
    path = tmp_path_factory.mktemp("fitscat") / "cat.fits"
    rows = write_catalog_file(path, NROWS)
    return path, rows


def test_layout(catfile):
    path, rows = catfile
    cat = hx.FitsCatalog(path)
    assert cat.names == SCALAR_NAMES
    assert cat.size == NROWS
    off, width, size, columns = cat._layout()
    dt = dtype_of(CATALOG_COLUMNS)
    assert width == dt.itemsize == 83 and width % 2 == 1 and size == NROWS
    tform = {name: t for name, t, _ in CATALOG_COLUMNS}
    for name, letter, offset, tscal, tzero in columns:
        assert letter == tform[name]
        assert offset == dt.fields[name][1]
        assert (tscal, tzero) == tuple(map(float, CATALOG_SCALING.get(name, (1, 0))))
    # the payload really starts there
    with open(path, "rb") as f:
        f.seek(off)
        first = np.frombuffer(f.read(width), dtype=dt)
    assert first.tobytes() == rows[:1].tobytes()


def test_requested_columns_keep_their_order(catfile):
    path, _ = catfile
    cat = hx.FitsCatalog(path, columns=["Z", "RA", "tom_bin_id"])
    assert cat.names == ["Z", "RA", "tom_bin_id"]
    assert [c[1] for c in cat._layout()[3]] == ["E", "D", "J"]
    with pytest.raises(ValueError, match="no column 'NOPE'"):
        hx.FitsCatalog(path, columns=["NOPE"]).size


def test_ext(catfile):
    path, _ = catfile
    for ext in (None, 3, "CATALOG", "catalog"):
        cat = hx.FitsCatalog(path, ext=ext)
        assert (cat.size, cat.names) == (NROWS, SCALAR_NAMES), ext
    other = hx.FitsCatalog(path, ext="OTHER")
    assert (other.size, other.names) == (5, ["X", "Y"])
    assert hx.FitsCatalog(path, ext=4).names == ["X", "Y"]
    assert hx.FitsCatalog(path, ext=2).size == 0  # the empty table, when asked for
    with pytest.raises(TypeError, match="not a binary table"):
        hx.FitsCatalog(path, ext=1).size
    with pytest.raises(TypeError, match="not a binary table"):
        hx.FitsCatalog(path, ext="IMG").size
    with pytest.raises(KeyError):
        hx.FitsCatalog(path, ext="MISSING").size
    with pytest.raises(IndexError):
        hx.FitsCatalog(path, ext=7).size


def test_no_table_data(tmp_path):
    path = tmp_path / "empty.fits"
    cols = [("X", "D", ">f8")]
    with open(path, "wb") as f:
        write_primary(f)
        write_table(f, cols, np.zeros(0, dtype_of(cols)), "EMPTY")
    with pytest.raises(TypeError, match="^no table data in FITS$"):
        hx.FitsCatalog(path).size


def test_lazy_open(tmp_path):
    path = tmp_path / "missing.fits"
    cat = hx.FitsCatalog(path, columns=["RA"], ext="CATALOG", page_size=10, metadata={"catalog": "c"})
    assert cat.path == path and cat.page_size == 10 and cat.label == "c" and cat.names == ["RA"]
    assert cat.base is None and cat.selection is None and cat.filters == []
    view = cat.where("RA > 1")["RA < 2"]
    assert view.base is cat and view.selection == ("RA > 1", "RA < 2")
    copy.copy(cat)
    for use in (lambda: cat.size, lambda: hx.FitsCatalog(path).names, lambda: next(iter(cat)), lambda: view.size,
                lambda: cat.where(np.ones(3, bool))):
        with pytest.raises(FileNotFoundError):
            use()


def test_repr(tmp_path):
    assert repr(hx.FitsCatalog("cat.fits")) == "cat.fits"
    assert repr(hx.FitsCatalog("cat.fits", ext="CATALOG")) == "cat.fits['CATALOG']"
    assert repr(hx.FitsCatalog(tmp_path / "c.fits", ext=2)) == f"{tmp_path / 'c.fits'}[2]"
    assert repr(hx.FitsCatalog("cat.fits")["RA > 1"]) == "cat.fits['RA > 1']"


def test_copy(catfile):
    path, _ = catfile
    vis = np.ones(12)
    cat = hx.FitsCatalog(path, columns=["RA", "DEC"], ext=3, page_size=100, visibility=vis, metadata={"catalog": "x"})
    filt = hx.InvalidValueFilter("RA")
    cat.add_filter(filt)
    other = copy.copy(cat)
    assert type(other) is hx.FitsCatalog and other is not cat
    assert (other.path, other.names, repr(other), other.page_size, other.label) == (path, ["RA", "DEC"], repr(cat), 100, "x")
    assert other.visibility is vis and other.fsky == 1.0 and other.size == NROWS
    assert other.filters == [filt] and other.filters is not cat.filters
    other.add_filter(hx.InvalidValueFilter("DEC"))
    other.page_size = 7
    assert len(cat.filters) == 1 and cat.page_size == 100


def test_masks_are_checked_against_the_table(catfile):
    path, _ = catfile
    cat = hx.FitsCatalog(path)
    assert cat.where(np.ones(NROWS, bool)).base is cat
    with pytest.raises(ValueError, match=f"catalogue of {NROWS} rows"):
        cat.where(np.ones(NROWS - 1, bool))
    with pytest.raises(TypeError, match="cannot select rows"):
        cat.where(np.arange(3))


UNREADABLE = [("S", "8A"), ("V", "3E"), ("BITS", "12X"), ("C", "C"), ("M", "M"), ("P", "1PE(7)"), ("Q", "1QD(9)"), ("D0", "0D")]


def _odd_table(path):
    """One scalar column either side of every kind of column that is not read."""
    widths = {"8A": "S8", "3E": (">f4", (3,)), "12X": "S2", "C": "S8", "M": "S16", "1PE(7)": "S8", "1QD(9)": "S16", "0D": "S0"}
    cols = [("A", "J", ">i4"), *[(name, tform, widths[tform]) for name, tform in UNREADABLE], ("B", "I", ">i2")]
    dt = np.dtype({"names": [c[0] for c in cols], "formats": [c[2] for c in cols]})
    rows = np.zeros(4, dt)
    rows["A"], rows["B"] = np.arange(4), -np.arange(4)
    with open(path, "wb") as f:
        write_primary(f)
        f.write(table_header(cols, 4, "ODD"))
        f.write(rows.tobytes())
        f.write(b"\0" * (-rows.nbytes % 2880))
    return dt


def test_unreadable_columns(tmp_path, catfile):
    path = tmp_path / "odd.fits"
    dt = _odd_table(path)
    cat = hx.FitsCatalog(path)
    assert cat.names == ["A", "B"] and cat.size == 4  # skipped when nobody asked for them
    (_, _, offa, _, _), (_, _, offb, _, _) = cat._layout()[3]
    assert (offa, offb) == (0, dt.itemsize - 2) and cat._layout()[1] == dt.itemsize
    for name, tform in UNREADABLE:
        with pytest.raises(TypeError, match=name) as e:
            hx.FitsCatalog(path, columns=["A", name]).size
        assert repr(tform) in str(e.value)
    for name, tform in (("NAME", "8A"), ("VEC", "3E")):
        with pytest.raises(TypeError) as e:
            hx.FitsCatalog(catfile[0], columns=["RA", name]).size
        assert repr(name) in str(e.value) and repr(tform) in str(e.value)


def test_compressed_files(tmp_path, catfile):
    gz = tmp_path / "cat.fits.gz"
    with open(catfile[0], "rb") as f, gzip.open(gz, "wb") as g:
        g.write(f.read())
    with pytest.raises(ValueError, match="gzip-compressed"):
        hx.FitsCatalog(gz).size
    cols = [("COMPRESSED_DATA", "1PB(10)", "S8")]
    for key in ("ZIMAGE", "ZTABLE"):
        path = tmp_path / f"{key}.fits"
        with open(path, "wb") as f:
            write_primary(f)
            write_table(f, cols, np.zeros(3, dtype_of(cols)), "COMPRESSED", extra=[_card(key, True)])
        for ext in (None, 1, "COMPRESSED"):
            with pytest.raises(ValueError, match=f"tile-compressed \\({key}\\)"):
                hx.FitsCatalog(path, ext=ext).size
    junk = tmp_path / "junk.fits"
    junk.write_bytes(b"not a FITS file at all")
    with pytest.raises(ValueError, match="not a FITS file"):
        hx.FitsCatalog(junk).size


def test_page_source_of_array_catalog():
    cols = {"a": np.arange(10, dtype=np.int64), "b": np.linspace(0, 1, 10)}
    cat = hx.ArrayCatalog(cols, page_size=4)
    assert cat._column_dtypes() == {"a": np.dtype(np.int64), "b": np.dtype(np.float64)}
    page = cat._page_columns(4, 8)
    assert list(page) == ["a", "b"] and page["a"].tolist() == [4, 5, 6, 7] and np.shares_memory(page["b"], cols["b"])
