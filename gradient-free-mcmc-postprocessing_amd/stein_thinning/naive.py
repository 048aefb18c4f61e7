"""Naive thinning and its evaluation curves -- the baseline every method of the reference is compared
against (``Gaussian_mixture.ipynb``: ``naive_thin``, ``ksd_naive``, ``naive_st``;
``lotka_volterra/Comparison.ipynb``: ``rw_ksd_naive`` / ``rw_energy_distance_naive`` over
``thinned_sizes``).  Naive index sets are not nested -- ``np.linspace(0, n - 1, m).astype(int)`` is a
different set for every m -- so the reference evaluates one full KSD, or one full energy distance, per
thinned size.  Here all sizes go to the device as one batch over index sets
(``stein.ksd_sets`` / ``energy.energy_distance_sets``): one standardisation, one upload, a fixed number
of launches.
"""
from __future__ import annotations

import numpy as np

from . import energy, stein
from .thinning import _make_stein_integrand


def naive_idx(n: int, m: int) -> np.ndarray:
    """The notebooks' naive thinning: m indices evenly spread over [0, n - 1], truncated to int."""
    return np.linspace(0, n - 1, m).astype(int)


def calculate_ksd_sets(sample, gradient, index_sets) -> np.ndarray:
    """``calculate_ksd(sample, gradient, idx)[-1]`` of the reference harness (code/src/utils/ksd.py:19-27:
    standardised sample, 'id' preconditioner) for every idx in ``index_sets``, with one
    standardisation and one upload for all of them."""
    return stein.ksd_sets(_make_stein_integrand(sample, gradient), index_sets)


def naive_ksd_curve(sample, gradient, sizes) -> np.ndarray:
    """KSD of the naive-thinned subsample of every size in ``sizes`` (ksd_naive / rw_ksd_naive)."""
    n = np.asarray(sample).shape[0]
    return calculate_ksd_sets(sample, gradient, [naive_idx(n, int(m)) for m in np.asarray(sizes).reshape(-1)])


def naive_energy_curve(reference_points, sample, sizes) -> np.ndarray:
    """fit_quality -- sqrt(energy_distance(reference_points, subsample)) -- of the naive-thinned
    subsample of every size in ``sizes`` (naive_st / rw_energy_distance_naive)."""
    n = np.asarray(sample).shape[0]
    return energy.energy_distance_sets(reference_points, sample,
                                       [naive_idx(n, int(m)) for m in np.asarray(sizes).reshape(-1)])
