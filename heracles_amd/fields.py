"""The field types of heracles/fields.py, mapped on the GPU by ``heracles_amd.map_catalogs``.

A field names the catalogue columns it reads and the mapper that pixelises them; what it computes is the reference's
(heracles/fields.py:197-559), and so are its column rules, its properties and the texts of its errors.  The maps themselves are made by
``map_catalogs``, which reads each catalogue page once for all the fields mapped from that catalogue; calling a field on a catalogue is a
shorthand for mapping that one field.
"""

from __future__ import annotations

from itertools import combinations_with_replacement, product

from .core import toc_match

__all__ = ["Field", "Positions", "ScalarField", "ComplexField", "Spin2Field", "Shears", "Ellipticities", "Visibility", "Weights",
           "get_masks"]


def _uses_tuple(uses):
    if uses is None:
        return ()
    if isinstance(uses, str):
        return (uses,)
    return tuple(uses)


class Field:
    """Base class of the field types.  ``uses`` lists the columns; trailing ``"[name]"`` entries are optional and become ``None``
    when not given.  Subclasses set their spin weight with ``class X(Field, spin=...)``."""

    uses = None
    _spin_weight = None
    _ncols = (0, 0)

    def __init_subclass__(cls, *, spin=None, **kwargs):
        super().__init_subclass__(**kwargs)
        if spin is not None:
            cls._spin_weight = spin
        uses = _uses_tuple(cls.uses)
        optional = 0
        while optional < len(uses) and uses[len(uses) - 1 - optional][:1] == "[" and uses[len(uses) - 1 - optional][-1:] == "]":
            optional += 1
        cls._ncols = (len(uses) - optional, len(uses))

    def __init__(self, mapper, *columns, mask=None):
        self._mapper = mapper
        self._columns = self._init_columns(*columns) if columns else None
        self._mask = mask

    @classmethod
    def _init_columns(cls, *columns):
        lo, hi = cls._ncols
        if len(columns) < lo or len(columns) > hi:
            uses = _uses_tuple(cls.uses)
            count = f"{lo}" if lo == hi else f"{lo} to {hi}"
            listed = f" ({', '.join(uses)})" if uses else ""
            raise ValueError(f"field of type '{cls.__name__}' accepts {count} columns{listed}, received {len(columns)}")
        return tuple(columns) + (None,) * (hi - len(columns))

    @property
    def mapper(self):
        return self._mapper

    @property
    def mapper_or_error(self):
        if self._mapper is None:
            raise ValueError("no mapper for field")
        return self._mapper

    @property
    def columns(self):
        return self._columns

    @property
    def columns_or_error(self):
        if self._columns is None:
            raise ValueError("no columns for field")
        return self._columns

    @property
    def spin(self):
        if self._spin_weight is None:
            raise ValueError(f"field of type '{type(self).__name__}' has undefined spin weight")
        return self._spin_weight

    @property
    def mask(self):
        return self._mask

    def __call__(self, catalog, *, progress=None, device=None):
        """The map of this field for one catalogue (``map_catalogs`` of one field and one catalogue)."""
        from .mapping import map_catalogs

        return map_catalogs({None: self}, {None: catalog}, device=device)[None, None]


class Positions(Field, spin=0):
    """Number counts, or the density contrast when ``overdensity`` is true (the default)."""

    uses = "longitude", "latitude", "[weight]"

    def __init__(self, mapper, *columns, overdensity=True, nbar=None, mask=None):
        super().__init__(mapper, *columns, mask=mask)
        self._overdensity = overdensity
        self._nbar = nbar

    @property
    def overdensity(self):
        return self._overdensity

    @property
    def nbar(self):
        return self._nbar

    @nbar.setter
    def nbar(self, nbar):
        self._nbar = nbar


class ScalarField(Field, spin=0):
    """Weighted real values."""

    uses = "longitude", "latitude", "value", "[weight]"


class ComplexField(Field, spin=0):
    """Weighted complex values (real and imaginary column); subclasses carry a spin weight."""

    uses = "longitude", "latitude", "real", "imag", "[weight]"


class Visibility(Field, spin=0):
    """The catalogue's visibility map at the mapper's resolution."""


class Weights(Field, spin=0):
    """The catalogue's weights."""

    uses = "longitude", "latitude", "[weight]"


class Spin2Field(ComplexField, spin=2):
    """Spin-2 complex field."""


Shears = Spin2Field
Ellipticities = Spin2Field


def get_masks(fields, *, comb=None, include=None, exclude=None, append_eb=False):
    """Masks of ``fields`` (heracles/fields.py:519-559): one per field that has a mask and passes the ``include`` / ``exclude``
    filter, or, with ``comb``, one tuple per combination (with replacement) of ``comb`` fields that all have masks.  With
    ``append_eb`` the filter sees ``name_E`` / ``name_B`` for fields of non-zero spin."""

    def names(key):
        return (f"{key}_E", f"{key}_B") if append_eb and fields[key].spin != 0 else (key,)

    def passes(key):
        return any(toc_match(k, include=include, exclude=exclude) for k in key)

    if comb is None:
        return [f.mask for k, f in fields.items() if f.mask is not None and passes(names(k))]
    out = []
    for keys in combinations_with_replacement(fields, comb):
        masks = tuple(fields[k].mask for k in keys)
        if None in masks:
            continue
        if passes(product(*map(names, keys))):
            out.append(masks)
    return out
