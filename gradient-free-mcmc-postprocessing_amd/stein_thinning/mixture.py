"""Gaussian-mixture log density and score on the GPU, as a target and as a proxy.

The reference's Gaussian-mixture study builds its target with ``make_mvn_mixture(weights, means,
covs)`` (``code/src/utils/mvn.py``) and feeds ``logpdf(sample)`` / ``score(sample)`` to ``thin`` /
``thin_gf`` throughout ``Gaussian_mixture.ipynb``.  There both are sums of component *densities*
(``log(sum_c w_c pdf_c(x))``, ``-num / den``; the score a four-operand NumPy einsum of O(n k d^2)
work on the host): once every component density underflows the row is ``-inf`` / ``NaN``.

Here the per-component constants are computed on the host (``mixture_factors``: scipy's
log-pseudo-determinant and ``np.linalg.inv``, as ``gaussian_proxy``) and the per-row work runs in one
HIP kernel (``st_mixture_logpdf_score``, csrc/mixture.hpp) in log space::

    dev_c = x - mu_c,  y_c = P_c dev_c,  l_c = a_c - dev_c . y_c / 2
    log_p = logsumexp_c l_c,  score = - sum_c exp(l_c - log_p) y_c

so far tails stay finite, zero-weight components contribute nothing, and the values agree with the
reference's to fp64 rounding where the reference is finite (weights are used as given, without
normalisation, as the reference does).  The same function is a mixture *proxy* for ``thin_gf``
(``proxy.mixture_proxy`` / ``proxy.mixture_thin``).  Importing this module touches no GPU.
"""
from __future__ import annotations

from typing import Callable, Tuple

import numpy as np

from . import _native as nat

MAX_DIM = 64   # st_mixture_logpdf_score: d <= 64 (csrc/stein_internal.hpp kMixtureMaxDim)
_LOG_2PI = float(np.log(2 * np.pi))


def mixture_factors(weights, means, covs) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Host-side constants of the mixture: ``(log_coef, means, precision)`` with ``log_coef[c] =
    log w_c - (d log 2 pi + log det Sigma_c) / 2`` (-inf for a zero weight; the log determinant is
    scipy's ``_PSD`` log-pseudo-determinant), ``means`` (k, d) and ``precision = np.linalg.inv(covs)``
    (k, d, d), all float64 and contiguous.  ValueError for misshapen inputs, negative or non-finite
    weights, a zero weight sum or a covariance that is not symmetric; a singular covariance raises
    as ``gaussian_proxy`` does (LinAlgError); NotImplementedError for d > 64."""
    from .proxy import _psd
    w = np.asarray(weights, dtype=np.float64)
    mu = np.asarray(means, dtype=np.float64)
    cv = np.asarray(covs, dtype=np.float64)
    if w.ndim != 1 or w.shape[0] < 1:
        raise ValueError(f'weights must be a vector (k,), got shape {w.shape}')
    k = w.shape[0]
    if mu.ndim != 2 or mu.shape[0] != k or mu.shape[1] < 1:
        raise ValueError(f'means must be ({k}, d), got shape {mu.shape}')
    d = mu.shape[1]
    if cv.shape != (k, d, d):
        raise ValueError(f'covs must be ({k}, {d}, {d}), got shape {cv.shape}')
    if not np.all(np.isfinite(w)) or np.any(w < 0):
        raise ValueError('weights must be finite and non-negative')
    if not np.sum(w) > 0:
        raise ValueError('weights must not sum to zero')
    if not np.all(np.isfinite(mu)):
        raise ValueError('means must be finite')
    if d > MAX_DIM:
        raise NotImplementedError(f'mixture: d = {d} exceeds the supported maximum {MAX_DIM}')
    log_det = np.empty(k)
    for c in range(k):
        if not np.array_equal(cv[c], cv[c].T):
            raise ValueError(f'covariance {c} is not symmetric')
        log_det[c] = _psd(cv[c], allow_singular=False).log_pdet
    precision = np.linalg.inv(cv)
    with np.errstate(divide='ignore'):
        log_w = np.log(w)
    log_coef = log_w - 0.5 * (d * _LOG_2PI + log_det)
    return (np.ascontiguousarray(log_coef), np.ascontiguousarray(mu), np.ascontiguousarray(precision))


def _launch(xd, factors, dev):
    """Enqueue the kernel on device tensor ``xd`` (n, d), n >= 1; returns device tensors."""
    import torch
    log_coef, mu, precision = factors
    n, d = xd.shape
    log_p = torch.empty(n, dtype=torch.float64, device=dev)
    score = torch.empty((n, d), dtype=torch.float64, device=dev)
    cd = torch.from_numpy(log_coef).to(dev)
    md = torch.from_numpy(mu).to(dev)
    pd = torch.from_numpy(precision).to(dev)
    nat.check(nat.lib().st_mixture_logpdf_score(nat.ptr(xd), n, d, log_coef.shape[0], nat.ptr(cd), nat.ptr(md),
                                                nat.ptr(pd), nat.ptr(log_p), nat.ptr(score), nat.stream_handle()),
              'st_mixture_logpdf_score')
    return log_p, score


def _eval(sample, factors):
    d = factors[1].shape[1]
    if bool(getattr(sample, 'is_cuda', False)):   # a ROCm tensor: evaluated in place on its device
        import torch
        if sample.dtype != torch.float64:
            raise ValueError(f'a device sample must be float64, got {sample.dtype}')
        x = sample[:, None] if sample.dim() == 1 else sample
        if x.dim() != 2 or x.shape[1] != d:
            raise ValueError(f'sample must be (n, {d}), got shape {tuple(sample.shape)}')
        x = x.contiguous()
        if x.shape[0] == 0:
            return x.new_empty(0), x.new_empty((0, d))
        with torch.cuda.device(x.device):
            return _launch(x, factors, x.device)
    x = np.asarray(sample, dtype=np.float64)
    if x.ndim == 1:
        x = x[:, None]
    if x.ndim != 2 or x.shape[1] != d:
        raise ValueError(f'sample must be (n, {d}), got shape {np.shape(sample)}')
    if x.shape[0] == 0:
        return np.empty(0), np.empty((0, d))
    import warnings
    import torch
    dev = nat.require_device()
    with warnings.catch_warnings():   # a read-only array is only read (torch warns that it could be written)
        warnings.filterwarnings('ignore', message='The given NumPy array is not writable')
        xd = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    log_p, score = _launch(xd, factors, dev)
    return log_p.cpu().numpy(), score.cpu().numpy()


def mixture_logpdf_score(sample, weights, means, covs):
    """(log_p, score) of the Gaussian mixture ``sum_c w_c N(mu_c, Sigma_c)`` at every row of
    ``sample`` (n, d): shapes (n,) and (n, d).  A NumPy sample returns NumPy arrays; a float64 ROCm
    tensor returns tensors on its device, nothing copied to the host.  A 1-d sample means d = 1."""
    return _eval(sample, mixture_factors(weights, means, covs))


def make_mvn_mixture(weights, means, covs) -> Tuple[Callable, Callable]:
    """``(logpdf, score)`` with the call shapes of the reference's ``utils.mvn.make_mvn_mixture``:
    ``logpdf(x, axes=slice(None))`` -- ``axes`` a slice or an int: the marginal mixture on those
    coordinates (the means and covariances subset on the host, the same kernel at the smaller d) --
    and ``score(x)``.  Sampling (``rvs``) and the JAX variant are not provided."""
    w = np.asarray(weights, dtype=np.float64)
    mu = np.asarray(means, dtype=np.float64)
    cv = np.asarray(covs, dtype=np.float64)
    full = mixture_factors(w, mu, cv)
    d = mu.shape[1]

    def logpdf(x, axes=slice(None)):
        if isinstance(axes, slice) and axes == slice(None):
            return _eval(x, full)[0]
        idx = np.atleast_1d(np.arange(d)[axes])
        sub = mixture_factors(w, mu[:, idx], cv[:, idx[:, None], idx[None, :]])
        return _eval(x, sub)[0]

    def score(x):
        return _eval(x, full)[1]

    return logpdf, score
