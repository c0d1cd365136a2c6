"""FITS binary tables for the FitsCatalog tests and timings, written with numpy and the card helpers of ``heracles_amd.fits`` only, and
the numpy decoder that is the expected value everywhere.

A table is a big-endian structured array: its bytes are the payload.  ``write_catalog_file`` puts the catalogue table behind a primary
HDU, an image extension and an empty table, and a second named table after it.  The catalogue table holds every scalar type, the two
scaled columns, the unsigned and signed-byte conventions, a string and a vector column, and is 83 bytes wide: odd, with every field
behind the leading byte column misaligned."""

import numpy as np

from heracles_amd.fits import BLOCK, _card, _header_bytes

# (name, TFORM, numpy dtype of the field)
CATALOG_COLUMNS = [
    ("FLAG_B", "B", "u1"), ("RA", "D", ">f8"), ("DEC", "D", ">f8"), ("W", "E", ">f4"), ("G1", "D", ">f8"), ("G2", "D", ">f8"),
    ("TOM_BIN_ID", "J", ">i4"), ("ID", "K", ">i8"), ("FLAG_I", "I", ">i2"), ("GOOD", "L", "u1"), ("U16", "I", ">i2"),
    ("SCALED", "J", ">i4"), ("NAME", "8A", "S8"), ("VEC", "3E", (">f4", (3,))), ("Z", "E", ">f4"), ("S8", "B", "u1"),
]
CATALOG_SCALING = {"U16": (1, 32768), "SCALED": (0.01, -3), "S8": (1, -128)}  # name -> (TSCAL, TZERO)
SCALAR_NAMES = [name for name, tform, _ in CATALOG_COLUMNS if tform in tuple("LBIJKED")]
NBINS = 13

# the eight columns of the README's example (positions, shears, weight, redshift, tomographic bin, a flag): 47 bytes a row
EXAMPLE_COLUMNS = [("ra", "D", ">f8"), ("dec", "D", ">f8"), ("g1", "D", ">f8"), ("g2", "D", ">f8"), ("w", "D", ">f8"), ("z", "E", ">f4"),
                   ("TOM_BIN_ID", "I", ">i2"), ("flag", "B", "u1")]


def dtype_of(columns):
    return np.dtype([(name, dt) for name, _, dt in columns])


def catalog_rows(nrows, seed=11, extremes=True):
    """``nrows`` rows of the catalogue table; ``extremes`` puts the edge values of every type into the first rows."""
    rng = np.random.default_rng(seed)
    a = np.zeros(nrows, dtype=dtype_of(CATALOG_COLUMNS))
    a["FLAG_B"] = rng.integers(0, 256, nrows)
    a["RA"] = rng.uniform(0, 360, nrows)
    a["DEC"] = np.degrees(np.arcsin(rng.uniform(-1, 1, nrows)))
    a["W"] = rng.choice([0.0, 0.5, 1.0, 2.0], nrows, p=[0.1, 0.2, 0.5, 0.2])
    a["G1"] = rng.normal(0, 0.3, nrows)
    a["G2"] = rng.normal(0, 0.3, nrows)
    a["TOM_BIN_ID"] = rng.integers(0, NBINS, nrows)
    a["ID"] = rng.integers(-2**62, 2**62, nrows)
    a["FLAG_I"] = rng.integers(-2**15, 2**15, nrows)
    a["GOOD"] = rng.choice(np.frombuffer(b"TF\0t", dtype="u1"), nrows)
    a["U16"] = rng.integers(-2**15, 2**15, nrows)
    a["SCALED"] = rng.integers(-2**31, 2**31, nrows)
    a["NAME"] = b"abcdefgh"
    a["VEC"] = rng.normal(size=(nrows, 3))
    a["Z"] = rng.uniform(0, 2, nrows)
    a["S8"] = rng.integers(0, 256, nrows)
    if extremes and nrows >= 8:
        a["ID"][:8] = [2**53, -(2**53), 2**53 + 1, -(2**53) - 1, 2**63 - 1, -(2**63), 0, -1]
        z = np.array([1e-45, -1e-45, np.finfo(np.float32).tiny, np.nan, np.inf, -np.inf, -0.0, 3.4028235e38], dtype=np.float32)
        a["Z"][:8] = z
        a["FLAG_B"][:2] = [0, 255]
        a["S8"][:2] = [0, 255]
        a["FLAG_I"][:2] = [-(2**15), 2**15 - 1]
        a["U16"][:2] = [-(2**15), 2**15 - 1]
        a["SCALED"][:2] = [-(2**31), 2**31 - 1]
        a["TOM_BIN_ID"][:2] = [0, NBINS - 1]
    return a


def decode(rows, names, scaling=None, columns=CATALOG_COLUMNS):
    """{name: float64 column} as numpy decodes the table: ``astype('f8')`` (``'T'`` -> 1 for a logical column), then
    ``stored * TSCAL + TZERO`` in two steps where the column is scaled."""
    scaling = CATALOG_SCALING if scaling is None and columns is CATALOG_COLUMNS else (scaling or {})
    tform = {name: t for name, t, _ in columns}
    out = {}
    for name in names:
        v = (rows[name] == ord("T")).astype("f8") if tform[name] == "L" else rows[name].astype("f8")
        if name in scaling:
            tscal, tzero = scaling[name]
            v = v * np.float64(tscal)
            v = v + np.float64(tzero)
        out[name] = v
    return out


def table_header(columns, nrows, extname, scaling=None, extra=()):
    width = dtype_of(columns).itemsize
    cards = [_card("XTENSION", "BINTABLE", "binary table extension"), _card("BITPIX", 8), _card("NAXIS", 2), _card("NAXIS1", width),
             _card("NAXIS2", nrows), _card("PCOUNT", 0), _card("GCOUNT", 1), _card("TFIELDS", len(columns))]
    for i, (name, tform, _) in enumerate(columns, start=1):
        cards += [_card(f"TTYPE{i}", name), _card(f"TFORM{i}", tform)]
        if scaling and name in scaling:
            cards += [_card(f"TSCAL{i}", scaling[name][0]), _card(f"TZERO{i}", scaling[name][1])]
    cards.append(_card("EXTNAME", extname))
    return _header_bytes(cards + list(extra))


def _padded(f, nbytes):
    f.write(b"\0" * (-nbytes % BLOCK))


def write_primary(f):
    f.write(_header_bytes([_card("SIMPLE", True), _card("BITPIX", 16), _card("NAXIS", 0), _card("EXTEND", True)]))


def write_table(f, columns, rows, extname, scaling=None, extra=(), repeat=1):
    """One BINTABLE HDU whose payload is ``rows.tobytes()``, ``repeat`` times over."""
    assert rows.dtype == dtype_of(columns)
    f.write(table_header(columns, len(rows) * repeat, extname, scaling, extra))
    payload = rows.tobytes()
    for _ in range(repeat):
        f.write(payload)
    _padded(f, len(payload) * repeat)


def write_catalog_file(path, nrows, seed=11, extremes=True, edit=None):
    """The test file: primary HDU, a 3 x 5 int16 image, an empty table, the catalogue table ``CATALOG``, and a table ``OTHER`` of two
    float64 columns.  ``edit(rows)`` changes the catalogue rows before they are written.  Returns the catalogue rows."""
    rows = catalog_rows(nrows, seed, extremes)
    if edit is not None:
        edit(rows)
    other = [("X", "D", ">f8"), ("Y", "D", ">f8")]
    with open(path, "wb") as f:
        write_primary(f)
        f.write(_header_bytes([_card("XTENSION", "IMAGE"), _card("BITPIX", 16), _card("NAXIS", 2), _card("NAXIS1", 5), _card("NAXIS2", 3),
                               _card("PCOUNT", 0), _card("GCOUNT", 1), _card("EXTNAME", "IMG")]))
        f.write(np.arange(15, dtype=">i2").tobytes())
        _padded(f, 30)
        write_table(f, other, np.zeros(0, dtype_of(other)), "EMPTY")
        write_table(f, CATALOG_COLUMNS, rows, "CATALOG", CATALOG_SCALING)
        xy = np.zeros(5, dtype_of(other))
        xy["X"], xy["Y"] = np.arange(5), -np.arange(5)
        write_table(f, other, xy, "OTHER")
    return rows


def example_rows(nrows, seed=3, bins=NBINS):
    rng = np.random.default_rng(seed)
    a = np.zeros(nrows, dtype=dtype_of(EXAMPLE_COLUMNS))
    a["ra"] = rng.uniform(0.0, 360.0, nrows)
    a["dec"] = np.degrees(np.arcsin(rng.uniform(-1.0, 1.0, nrows)))
    a["g1"] = rng.uniform(-0.5, 0.5, nrows)
    a["g2"] = rng.uniform(-0.5, 0.5, nrows)
    a["w"] = rng.uniform(0.5, 1.5, nrows)
    a["z"] = rng.uniform(0.0, 2.0, nrows)
    a["TOM_BIN_ID"] = rng.integers(0, bins, nrows)
    a["flag"] = rng.integers(0, 4, nrows)
    return a


def write_example_file(path, nrows, block=10_000_000, seed=3):
    """A catalogue of the README's eight columns: ``block`` random rows, repeated to ``nrows`` (a multiple of ``block`` if larger)."""
    block = min(block, nrows)
    assert nrows % block == 0
    rows = example_rows(block, seed)
    with open(path, "wb") as f:
        write_primary(f)
        write_table(f, EXAMPLE_COLUMNS, rows, "CATALOG", repeat=nrows // block)
    return rows
