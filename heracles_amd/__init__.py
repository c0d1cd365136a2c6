"""heracles_amd -- MI355X-native backend for the harmonic-space two-point hot path of
Heracles (map2alm/alm2map, all-pairs alm x alm -> Cl, Wigner-3j mixing matrices).

Everything numerical runs in libhxsht.so (hand-written HIP for gfx950, C ABI in
include/hxsht.h).  There is no CPU fallback.
"""

from . import _lib
from ._lib import HxError, device_count, init, pinned_empty, release_caches, synchronize
from .binning import BinPlan, binned
from .covariance import (
    bias,
    debias_covariance,
    delete2_correction,
    flatten,
    gaussian_covariance,
    get_cl,
    impose_correlation,
    jackknife_bias,
    jackknife_covariance,
    sample_covariance,
    shrink,
    shrinkage_factor,
)
from .core import DeviceArray, Result, TocDict, toc_match, update_metadata
from .discrete import HipDiscreteMapper, PointField, PointSHT, alm_resample, get_point_sht
from .jackknife import RegionAlms, correct_footprint_naturalspice_batch, jackknife_cls, region_alms
from .mapper import HipHealpixMapper
from .catalog import ArrayCatalog, CatalogView, FootprintFilter, InvalidValueFilter
from .fitscatalog import FitsCatalog
from .fields import (
    ComplexField,
    Ellipticities,
    Field,
    Positions,
    ScalarField,
    Shears,
    Spin2Field,
    Visibility,
    Weights,
    get_masks,
)
from .masks import apodize_mask, mask_discs, mask_distance, mask_polygons, rectangle_polygons
from .deprojection import DeprojectionInfo, deproject_maps, deproject_templates, deprojection_bias
from .mapping import catalog_alms, map_catalogs, transform
from .mocks import gaussian_maps, mock_catalogs, poisson_catalog, synalm, synalm_components
from .lognormal import lognormal_gaussian_cls, lognormal_maps, lognormal_realised_cls, nearest_psd_cls
from .regions import jackknife_regions
from .rotation import coord_matrix, euler_from_matrix, matrix_from_euler, rotate_alm, rotate_alms
from .sht import Plan, get_plan
from .transforms import cl2corr, cl2corr_columns, corr2cl, corr2cl_columns, gauss_legendre, wigner_d_table
from .fits import read_vmap
from .gausscov import covariance_requests, gaussian_covariance_coupled, mask_product_cls, table_key
from .twopoint import (
    alm2cl,
    alm2cl_pairs,
    alm2lmax,
    angular_power_spectra,
    apply_mixing_matrix,
    debias_cls,
    MixmatContext,
    invert_mixing_matrix,
    mixing_matrices,
    mixmat,
    mixmat_eb,
    mixmat_release,
    split_requests,
)
from .unmixing import naturalspice, naturalspice_batch
from .weights import compute_pixel_weights
from .pixwin import compute_pixel_window, find_window_file, read_pixel_window, write_pixel_window

__all__ = [
    "HipHealpixMapper", "HipDiscreteMapper", "PointSHT", "PointField", "get_point_sht", "alm_resample", "Plan", "get_plan", "HxError", "init", "device_count", "synchronize",
    "alm2cl", "alm2cl_pairs", "alm2lmax", "angular_power_spectra", "debias_cls",
    "mixing_matrices", "mixmat", "mixmat_eb", "cl2corr", "corr2cl", "gauss_legendre",
    "wigner_d_table", "naturalspice", "naturalspice_batch", "cl2corr_columns", "corr2cl_columns", "correct_footprint_naturalspice_batch", "Result", "TocDict", "toc_match", "update_metadata", "DeviceArray",
    "pinned_empty", "release_caches", "mixmat_release", "split_requests", "binned", "BinPlan", "MixmatContext", "jackknife_cls", "region_alms", "RegionAlms", "transform", "read_vmap", "apply_mixing_matrix", "invert_mixing_matrix",
    "sample_covariance", "jackknife_covariance", "delete2_correction", "debias_covariance", "gaussian_covariance",
    "shrinkage_factor", "shrink", "flatten", "impose_correlation", "get_cl", "bias", "jackknife_bias",
    "map_catalogs", "catalog_alms", "ArrayCatalog", "FitsCatalog", "CatalogView", "FootprintFilter", "InvalidValueFilter", "Field", "Positions", "ScalarField", "ComplexField", "Spin2Field", "Shears", "Ellipticities",
    "Visibility", "Weights", "get_masks", "compute_pixel_weights", "compute_pixel_window", "write_pixel_window", "read_pixel_window", "find_window_file", "synalm", "synalm_components", "gaussian_maps", "poisson_catalog", "mock_catalogs",
    "jackknife_regions", "rotate_alm", "rotate_alms", "euler_from_matrix", "matrix_from_euler", "coord_matrix",
    "mask_product_cls", "covariance_requests", "gaussian_covariance_coupled", "table_key",
    "mask_discs", "mask_polygons", "rectangle_polygons", "mask_distance", "apodize_mask",
    "deproject_templates", "deproject_maps", "deprojection_bias", "DeprojectionInfo",
    "lognormal_gaussian_cls", "lognormal_realised_cls", "nearest_psd_cls", "lognormal_maps",
]
