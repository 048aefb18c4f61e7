"""Proxy producers for gradient-free Stein thinning: log q and grad log q on the GPU.

The reference builds the proxy q of ``thin_gf`` on the host before every gradient-free thin:

* ``gaussian_thin(sample, log_p, mean, cov, thinned_size, range_cap=200)``
  (``code/src/thinning.py:14-17``): ``log_q = scipy.stats.multivariate_normal.logpdf(sample, mean,
  cov)``, ``gradient_q = -np.einsum('ij,kj->ki', np.linalg.inv(cov), sample - mean)``;
* ``thin_gf_t(sample, log_p, t_mu, t_scale, t_df, thinned_size)``
  (``code/notebooks/lotka_volterra/Gradient_free_Student_t.ipynb`` cells 29, 31, 40):
  ``log_q = scipy.stats.multivariate_t.logpdf(sample, loc, shape, df)``, ``gradient_q =
  t_grad_log_pdf(sample, loc, shape, df)``; both with ``range_cap=200``.

* the KDE proxy of ``Gaussian_mixture.ipynb`` cells 42-48 (and the weighted KDE of cell 51):
  ``kde = jax.scipy.stats.gaussian_kde(sample.T, bw_method='silverman'[, weights=w])``,
  ``log_q = kde.logpdf(sample.T)``, ``gradient_q`` = jax.grad of it at every row
  (``kde_proxy``; O(n^2 d): csrc/kde.hip, ``st_kde_logpdf_grad``).

* beyond the reference (its report's "Further Work": KDE kernels other than Gaussian): the Student-t
  kernel density ``kde_t_proxy`` / ``kde_t_thin`` (``st_kde_t_logpdf_grad``).

* the fit of the Student-t proxy in the same notebook: ``fit_mvt`` / ``fit_mvt2`` (maximum likelihood under
  ``scipy.optimize.minimize``, the objective ``-np.sum(stats.multivariate_t.logpdf(Y, loc, shape, df))``
  differentiated by finite differences: 16 passes over the rows per gradient at d = 4) and
  ``extract_t_params``.  Here (``StudentTLikelihood``, ``fit_mvt``, ``fit_mvt2``) one pass over the
  device-resident rows gives the objective and its full analytic gradient (st_mvt_moments,
  csrc/mvt_moments.hpp: the sums S0, S1, Sz, Szz; d <= 16).

* beyond the reference (which fits no mixture; its report asks for "bespoke treatment" of the auxiliary
  distribution): the fit of the Gaussian-mixture proxy by EM, ``fit_mixture`` / ``mixture_fit_thin``, one pass
  over the device-resident rows per iteration (st_mixture_em_stats, csrc/mixture_fit.hpp; d <= 16, k <= 32).

The parametric proxies are O(n d^2) per proxy (C5: n = 5e5, d = 50).  Here the d x d factors are computed on the host
exactly as scipy does (``_PSD``: eigh, pseudo-inverse square root; ``np.linalg.inv``; the scalar
constants in scipy's operation order) and the per-row work runs in one HIP kernel
(``st_proxy_logpdf_grad``, csrc/proxy.hip).  The per-row dot products are summed in a different
order than NumPy/BLAS: log q and grad log q agree with scipy to fp64 rounding (tests: relative
1e-12), not bit for bit.  For 16 < d <= 64 the Mahalanobis term of log q is ``dev . inv(cov) dev`` where
scipy's is ``|dev U|^2``: equal up to the gap between those two float64 factors, which is rounding-sized
for well-scaled covariances and grows with cond(cov) (about 7e-9 of the term at cond 2e8; DESIGN.md
section 1).
"""
from __future__ import annotations

import ctypes
import dataclasses
import math
from typing import Optional, Tuple

import numpy as np

from . import _native as nat

_LOG_2PI = float(np.log(2 * np.pi))   # scipy.stats._multivariate._LOG_2PI


class PsdFactor:
    """The factorisation scipy's multivariate_normal / multivariate_t logpdf use
    (scipy.stats._multivariate._PSD, restated on its public pieces so the same doubles come out):
    eigh of the lower triangle, eigenvalues below 1e6 * eps * max|eigenvalue| treated as zero,
    U = eigenvectors * sqrt(pseudo-inverse eigenvalues) (so U U^T = pinv(M)), log pseudo-determinant
    and rank."""

    def __init__(self, m: np.ndarray, allow_singular: bool = True):
        import scipy.linalg
        m = np.asarray(m)
        s, u = scipy.linalg.eigh(m, lower=True, check_finite=True)
        eps = 1e6 * np.finfo(s.dtype.char.lower()).eps * np.max(abs(s))
        if np.min(s) < -eps:
            raise ValueError('The input matrix must be symmetric positive semidefinite.')
        d = s[s > eps]
        if len(d) < len(s) and not allow_singular:
            raise np.linalg.LinAlgError('When `allow_singular is False`, the input matrix must be '
                                        'symmetric positive definite.')
        s_pinv = np.array([0 if abs(x) <= eps else 1 / x for x in s], dtype=float)
        self.U = np.multiply(u, np.sqrt(s_pinv))
        self.rank = len(d)
        self.log_pdet = np.sum(np.log(d))


def _psd(m: np.ndarray, allow_singular: bool) -> PsdFactor:
    return PsdFactor(m, allow_singular=allow_singular)


def _params(sample, loc, cov):
    x = np.ascontiguousarray(sample, dtype=np.float64)
    if x.ndim != 2:
        raise ValueError(f'sample must be 2-d (n, d), got shape {x.shape}')
    d = x.shape[1]
    loc = np.zeros(d) if loc is None else np.asarray(loc, dtype=np.float64).reshape(-1)
    if loc.shape != (d,):
        raise ValueError(f"location must be a vector of length {d}, got shape {loc.shape}")
    cov = np.asarray(cov, dtype=np.float64)
    if cov.ndim == 0:
        cov = cov * np.eye(d)
    elif cov.ndim == 1:
        cov = np.diag(cov)
    if cov.shape != (d, d):
        raise ValueError(f'covariance / shape matrix must be ({d}, {d}), got {cov.shape}')
    return x, loc, cov


def _device_eval(x, loc, whiten, precision, df: float, c_log: float):
    import torch
    dev = nat.require_device()
    n, d = x.shape
    log_q = torch.empty(max(n, 1), dtype=torch.float64, device=dev)
    grad = torch.empty((max(n, 1), d), dtype=torch.float64, device=dev)
    if n:
        xd = torch.from_numpy(x).to(dev)
        ld = torch.from_numpy(np.ascontiguousarray(loc)).to(dev)
        ud = torch.from_numpy(np.ascontiguousarray(whiten, dtype=np.float64)).to(dev)
        pd = torch.from_numpy(np.ascontiguousarray(precision, dtype=np.float64)).to(dev)
        nat.check(nat.lib().st_proxy_logpdf_grad(nat.ptr(xd), n, d, nat.ptr(ld), nat.ptr(ud), nat.ptr(pd),
                                                 float(df), float(c_log), nat.ptr(log_q), nat.ptr(grad),
                                                 nat.stream_handle()), 'st_proxy_logpdf_grad')
    return log_q[:n].cpu().numpy(), grad[:n].cpu().numpy()


def gaussian_proxy(sample, mean, cov) -> Tuple[np.ndarray, np.ndarray]:
    """(log_q, gradient_q) of the Gaussian proxy N(mean, cov) at every row of ``sample``:
    ``multivariate_normal.logpdf(sample, mean, cov)`` and ``-inv(cov) @ (x - mean)`` per row
    (code/src/thinning.py:15-16).  Raises like scipy / NumPy on a singular covariance."""
    x, mean, cov = _params(sample, mean, cov)
    psd = _psd(cov, allow_singular=False)
    precision = np.linalg.inv(cov)
    return _device_eval(x, mean, psd.U, precision, 0.0, psd.rank * _LOG_2PI + psd.log_pdet)


def student_t_proxy(sample, loc, shape, df: float) -> Tuple[np.ndarray, np.ndarray]:
    """(log_q, gradient_q) of the multivariate t proxy: ``multivariate_t.logpdf(sample, loc, shape,
    df)`` and the notebook's ``t_grad_log_pdf(sample, loc, shape, df)``
    (Gradient_free_Student_t.ipynb cells 29, 31)."""
    from scipy.special import gammaln
    x, loc, shape = _params(sample, loc, shape)
    df = float(df)
    if not df > 0 or not math.isfinite(df):
        raise ValueError("'df' must be a finite number greater than zero")
    d = x.shape[1]
    psd = _psd(shape, allow_singular=True)        # scipy.stats.multivariate_t's default
    precision = np.linalg.inv(shape)               # t_grad_log_pdf: np.linalg.inv(sigma)
    if psd.rank < d:
        raise ValueError('singular shape matrix')
    # scipy multivariate_t._logpdf: A - B - C - D + E, constants in its order
    t = 0.5 * (df + d)
    c_log = gammaln(t) - gammaln(0.5 * df) - d / 2. * np.log(df * np.pi) - 0.5 * psd.log_pdet
    return _device_eval(x, loc, psd.U, precision, df, float(c_log))


def kde_factors(dataset, bw_method='silverman', weights=None):
    """The constructor arithmetic of jax.scipy.stats.gaussian_kde (= scipy.stats.gaussian_kde) on an
    (n, d) dataset: normalised weights, n_eff, the bandwidth factor ('scott', 'silverman' or a
    scalar), the weighted data covariance, the precision inv(cov) / factor^2 and its lower
    Cholesky factor L (the kernel evaluation whitens with it: points @ L), log_norm =
    sum(log diag L) - d/2 log(2 pi).  Returns (weights, L, log_norm)."""
    x = np.asarray(dataset, dtype=np.float64)
    if x.ndim == 1:
        x = x[:, None]
    n, d = x.shape
    if n < 2:
        raise ValueError('a KDE needs at least two data points')
    w = np.full(n, 1.0 / n) if weights is None else np.asarray(weights, dtype=np.float64).reshape(-1)
    if w.shape != (n,):
        raise ValueError(f'weights must have length {n}')
    w = w / np.sum(w)
    neff = 1.0 / np.sum(w ** 2)
    if bw_method is None or bw_method == 'scott':
        factor = np.power(neff, -1.0 / (d + 4))
    elif bw_method == 'silverman':
        factor = np.power(neff * (d + 2) / 4.0, -1.0 / (d + 4))
    elif np.isscalar(bw_method) and not isinstance(bw_method, str):
        factor = float(bw_method)
    else:
        raise ValueError("bw_method must be 'scott', 'silverman' or a scalar")
    cov = np.atleast_2d(np.cov(x.T, rowvar=1, bias=False, aweights=w))
    inv_cov = np.linalg.inv(cov) / factor ** 2
    L = np.linalg.cholesky(inv_cov)
    log_norm = float(np.sum(np.log(np.diag(L))) - 0.5 * d * np.log(2 * np.pi))
    return w, L, log_norm


def kde_t_factors(dataset, df, bw_method='silverman', weights=None):
    """``kde_factors`` for the Student-t kernel density: the same normalised weights and whitening factor L
    (the Gaussian KDE's bandwidth rule, unchanged) and the kernel's log normaliser

        log_norm_t = sum(log diag L) + gammaln((df + d) / 2) - gammaln(df / 2) - d / 2 log(df pi),

    so that the density is sum_i w_i multivariate_t(y; loc = x_i, shape = cov * factor^2, df).  Returns
    (weights, L, log_norm_t).  For df >> 1e7 the two gammaln terms cancel to a few digits in float64 (their
    difference is ~ d / 2 log(df / 2) against values ~ df log df): the Gaussian limit is better served by
    ``kde_proxy`` itself."""
    from scipy.special import gammaln
    df = float(df)
    if not df > 0 or not math.isfinite(df):
        raise ValueError("'df' must be a finite number greater than zero")
    w, L, _ = kde_factors(dataset, bw_method, weights)
    d = L.shape[0]
    log_norm_t = float(np.sum(np.log(np.diag(L))) + gammaln(0.5 * (df + d)) - gammaln(0.5 * df)
                       - 0.5 * d * np.log(df * np.pi))
    return w, L, log_norm_t


def collapse_rows(rows, weights=None):
    """Repeated rows collapsed (an RW chain repeats its row at every rejection): ``(unique, summed, inverse)``
    with ``unique`` the distinct rows (np.unique's order), ``summed`` the sum of ``weights`` over each one's
    copies (None when ``weights`` is None) and ``inverse`` the index of every input row in ``unique``."""
    rows = np.asarray(rows, dtype=np.float64)
    unique, inverse = np.unique(rows, axis=0, return_inverse=True)
    inverse = np.asarray(inverse).reshape(-1)
    summed = None if weights is None else np.bincount(inverse, weights=weights, minlength=unique.shape[0])
    return unique, summed, inverse


def _kde_eval(data, pts, w, weighted, L, log_norm, df, collapse_repeats):
    """The GPU part of kde_proxy (df None: st_kde_logpdf_grad) and kde_t_proxy (st_kde_t_logpdf_grad): data
    and queries whitened with L and uploaded, log q and its gradient at every row of ``pts`` back on the
    host.  ``w`` are the normalised weights of the full data set (used when ``weighted`` or when rows are
    collapsed: a unique row then carries the log of its copies' summed weight)."""
    import torch
    from .device import padded_ld
    n, d = data.shape
    m = pts.shape[0]
    dev = nat.require_device()
    if m == 0:
        return np.empty(0), np.empty((0, d))
    inverse = None
    if collapse_repeats:
        same = pts is data
        data, w, inv_d = collapse_rows(data, w)
        weighted = True
        if same:
            pts, inverse = data, inv_d
        else:
            pts, _, inverse = collapse_rows(pts)
        n, m = data.shape[0], pts.shape[0]
    log_q = torch.empty(m, dtype=torch.float64, device=dev)
    grad = torch.empty((m, d), dtype=torch.float64, device=dev)

    def soa(a):
        ld = padded_ld(a.shape[0])
        t = torch.zeros((d, ld), dtype=torch.float64, device=dev)
        t[:, :a.shape[0]] = torch.from_numpy(np.ascontiguousarray((a @ L).T)).to(dev)   # whitened: a @ L
        return t, ld
    p_t, ldp = soa(data)
    q_t, ldq = soa(pts)
    logw = torch.from_numpy(np.log(w)).to(dev) if weighted else None   # a zero weight: -inf (NumPy warns)
    lt = torch.from_numpy(np.ascontiguousarray(L)).to(dev)
    lib = nat.lib()
    if df is None:
        wsb = int(lib.st_kde_workspace_bytes(m, d))
        ws = torch.empty(max(wsb // 8, 2), dtype=torch.float64, device=dev)
        nat.check(lib.st_kde_logpdf_grad(nat.ptr(p_t), ldp, n, nat.ptr(logw), float(np.log(1.0 / n)),
                                         nat.ptr(q_t), ldq, m, d, log_norm, nat.ptr(lt), nat.ptr(log_q),
                                         nat.ptr(grad), nat.ptr(ws), ws.numel() * 8, nat.stream_handle()),
                  'st_kde_logpdf_grad')
    else:
        wsb = int(lib.st_kde_t_workspace_bytes(m, d))
        ws = torch.empty(max(wsb // 8, 2), dtype=torch.float64, device=dev)
        nat.check(lib.st_kde_t_logpdf_grad(nat.ptr(p_t), ldp, n, nat.ptr(logw), float(np.log(1.0 / n)),
                                           nat.ptr(q_t), ldq, m, d, float(df), log_norm, nat.ptr(lt),
                                           nat.ptr(log_q), nat.ptr(grad), nat.ptr(ws), ws.numel() * 8,
                                           nat.stream_handle()),
                  'st_kde_t_logpdf_grad')
    log_q, grad = log_q.cpu().numpy(), grad.cpu().numpy()
    if inverse is not None:
        log_q, grad = log_q[inverse], grad[inverse]
    return log_q, grad


def _kde_inputs(sample, points):
    data = np.asarray(sample, dtype=np.float64)
    data = data[:, None] if data.ndim == 1 else data
    if points is None:
        return data, data
    pts = np.asarray(points, dtype=np.float64)
    pts = pts[:, None] if pts.ndim == 1 else pts
    if pts.ndim != 2 or pts.shape[1] != data.shape[1]:
        raise ValueError(f'points must be (m, {data.shape[1]})')
    return data, pts


def kde_proxy(sample, points=None, bw_method='silverman', weights=None,
              collapse_repeats=False) -> Tuple[np.ndarray, np.ndarray]:
    """(log_q, gradient_q) of the Gaussian KDE of ``sample`` at ``points`` (default: the sample
    itself) -- ``gaussian_kde(sample.T, bw_method, weights).logpdf(points.T)`` and its gradient, as
    Gaussian_mixture.ipynb cells 46-48 / 51 compute them for thin_gf.  The O(n m d) pair sums run
    on the GPU (st_kde_logpdf_grad); agrees with the restatement to fp64 rounding (the
    logsumexp and the softmax-weighted sums are sequential here, pairwise in NumPy).

    ``collapse_repeats=True``: repeated rows (an RW chain's rejections) are sent to the kernel once -- a
    unique data row carries the log of its copies' summed weight, a unique query row is evaluated once and
    scattered back.  The bandwidth factors still come from the full data set; the result differs from the
    uncollapsed one by the rounding of the reordered sums."""
    data, pts = _kde_inputs(sample, points)
    w, L, log_norm = kde_factors(data, bw_method, weights)
    return _kde_eval(data, pts, w, weights is not None, L, log_norm, None, collapse_repeats)


def kde_t_proxy(sample, points=None, df=4.0, bw_method='silverman', weights=None,
                collapse_repeats=False) -> Tuple[np.ndarray, np.ndarray]:
    """(log_q, gradient_q) of the Student-t kernel density of ``sample`` at ``points`` (default: the sample
    itself): q = sum_i w_i multivariate_t(y; loc = x_i, shape = cov * factor^2, df) with the polynomial
    tails the Gaussian KDE lacks (far from the data log q falls like -(df + d) log r, not -r^2 / 2) and a
    closed-form score.  Conventions as ``kde_proxy`` (1-D input is a column; ``collapse_repeats``).  The
    bandwidth is the Gaussian KDE's rule (``bw_method``: 'scott', 'silverman' or a scalar factor on the
    weighted data covariance) applied unchanged to the t kernel's shape matrix: a choice made here, not
    something the reference pins (it evaluates no KDE kernel other than the Gaussian).  The pair sums run
    on the GPU (st_kde_t_logpdf_grad, csrc/kde.hip)."""
    data, pts = _kde_inputs(sample, points)
    w, L, log_norm_t = kde_t_factors(data, df, bw_method, weights)
    return _kde_eval(data, pts, w, weights is not None, L, log_norm_t, float(df), collapse_repeats)


def kde_t_thin(sample, log_p, thinned_size: int, df=4.0, bw_method='silverman',
               range_cap: Optional[float] = 200, collapse_repeats=True) -> np.ndarray:
    """``gaussian_thin`` with the Student-t kernel density of the sample itself as the proxy
    (``kde_t_proxy``), then ``thin_gf(..., preconditioner='med')``."""
    from .thinning import thin_gf
    log_q, gradient_q = kde_t_proxy(sample, None, df, bw_method, collapse_repeats=collapse_repeats)
    return thin_gf(sample, log_p, log_q, gradient_q, thinned_size, range_cap=range_cap, preconditioner='med')


def gaussian_thin(sample, log_p, mean, cov, thinned_size: int, range_cap: Optional[float] = 200) -> np.ndarray:
    """code/src/thinning.py:14-17 with the proxy evaluated on the GPU."""
    from .thinning import thin_gf
    log_q, gradient_q = gaussian_proxy(sample, mean, cov)
    return thin_gf(sample, log_p, log_q, gradient_q, thinned_size, range_cap=range_cap, preconditioner='med')


def mixture_thin(sample, log_p, weights, means, covs, thinned_size: int,
                 range_cap: Optional[float] = 200) -> np.ndarray:
    """``gaussian_thin`` with a Gaussian-mixture proxy q = sum_c w_c N(mu_c, Sigma_c) (``mixture_proxy``:
    st_mixture_logpdf_score) -- the natural proxy of a multimodal target."""
    from .thinning import thin_gf
    log_q, gradient_q = mixture_proxy(sample, weights, means, covs)
    return thin_gf(sample, log_p, log_q, gradient_q, thinned_size, range_cap=range_cap, preconditioner='med')


def thin_gf_t(sample, log_p, t_mu, t_scale, t_df, thinned_size: int, range_cap: Optional[float] = 200) -> np.ndarray:
    """Gradient_free_Student_t.ipynb cell 40 with the proxy evaluated on the GPU (that cell keeps
    thin_gf's default preconditioner 'id')."""
    from .thinning import thin_gf
    log_q, gradient_q = student_t_proxy(sample, t_mu, t_scale, t_df)
    return thin_gf(sample, log_p, log_q, gradient_q, thinned_size, range_cap=range_cap)


MVT_MAX_DIM = 16   # st_mvt_moments: the moment kernels' widest instantiation


def _mvt_moments(lik: 'StudentTLikelihood', loc: np.ndarray, whiten: np.ndarray, df: float, want_grad: bool) -> np.ndarray:
    """All the GPU work of a StudentTLikelihood: on first use the rows go to the device (a ROCm tensor is
    used in place) with the workspace and the output; every call uploads loc and whiten (one small
    copy), enqueues st_mvt_moments (two launches) and brings the 2 + d + d (d + 1) / 2 doubles back
    (want_grad false: only S0 is computed; the rest of the record is stale)."""
    import torch
    n, d = lik.n, lik.d
    st = lik._device
    if st is None:
        dev = nat.require_device()
        x = lik.sample
        if torch.is_tensor(x):
            xd = x if x.is_contiguous() else x.contiguous()
            if not bool(torch.isfinite(xd).all()):
                raise ValueError('sample holds non-finite values')
        else:
            xd = torch.from_numpy(x if x.flags.writeable else x.copy()).to(dev)
        wsb = int(nat.lib().st_mvt_moments_workspace_bytes(n, d))
        if wsb < 0:
            raise NotImplementedError(f'st_mvt_moments: d = {d} exceeds {MVT_MAX_DIM}')
        st = lik._device = {
            'x': xd,
            'ws': torch.empty(wsb // 8, dtype=torch.float64, device=xd.device),
            'out': torch.zeros(2 + d + d * (d + 1) // 2, dtype=torch.float64, device=xd.device),
            'par': torch.empty(d + d * d, dtype=torch.float64, device=xd.device),
            'host': np.empty(d + d * d),
        }
    host = st['host']
    host[:d] = loc
    host[d:] = np.asarray(whiten, dtype=np.float64).reshape(-1)
    par = st['par']
    par.copy_(torch.from_numpy(host))
    with torch.cuda.device(par.device):
        nat.check(nat.lib().st_mvt_moments(nat.ptr(st['x']), n, d, ctypes.c_void_p(par.data_ptr()),
                                           ctypes.c_void_p(par.data_ptr() + 8 * d), float(df), 1 if want_grad else 0,
                                           nat.ptr(st['out']), nat.ptr(st['ws']), st['ws'].numel() * 8,
                                           nat.stream_handle()), 'st_mvt_moments')
        return st['out'].cpu().numpy()


class StudentTLikelihood:
    """The multivariate-t likelihood of a sample with the rows resident on the GPU: the objective of
    ``fit_mvt`` / ``fit_mvt2`` (Gradient_free_Student_t.ipynb: ``-np.sum(stats.multivariate_t.logpdf(Y,
    loc, shape, df))``) and its analytic gradient from one pass over the rows (st_mvt_moments).

    ``sample``: an (n, d) NumPy array or a float64 ROCm tensor (used in place), d <= 16, finite.  The
    rows, the workspace and the output stay on the device for the object's lifetime; an evaluation is
    two launches and one small copy each way."""

    def __init__(self, sample):
        tensor = hasattr(sample, 'data_ptr') and hasattr(sample, 'is_cuda')
        if tensor:
            import torch
            if sample.dtype != torch.float64 or not sample.is_cuda:
                raise ValueError('a tensor sample must be a float64 tensor on the ROCm device')
            x = sample[:, None] if sample.ndim == 1 else sample
        else:
            x = np.ascontiguousarray(sample, dtype=np.float64)
            x = x[:, None] if x.ndim == 1 else x
        if x.ndim != 2:
            raise ValueError(f'sample must be 2-d (n, d), got shape {tuple(x.shape)}')
        self.n, self.d = int(x.shape[0]), int(x.shape[1])
        if self.n < 1 or self.d < 1:
            raise ValueError(f'sample must hold at least one row and one column, got shape {tuple(x.shape)}')
        if self.d > MVT_MAX_DIM:
            raise ValueError(f'd = {self.d} exceeds the moment kernels\' maximum {MVT_MAX_DIM}')
        if not tensor and not np.all(np.isfinite(x)):
            raise ValueError('sample holds non-finite values')
        self.sample = x
        self._device = None

    def moments(self, loc, whiten, df: float, grad: bool = True):
        """(S0, S1, Sz, Szz) as host doubles for z = (x - loc) @ whiten, delta = |z|^2, w = (df + d) /
        (df + delta): S0 = sum log(1 + delta / df), S1 = sum w, Sz = sum w z (d), Szz = sum w z z^T
        ((d, d), symmetric).  ``grad=False``: S0 alone (the same bits), the others None."""
        d = self.d
        loc = np.asarray(loc, dtype=np.float64).reshape(-1)
        whiten = np.asarray(whiten, dtype=np.float64)
        if loc.shape != (d,) or whiten.shape != (d, d):
            raise ValueError(f'loc must have length {d} and whiten shape ({d}, {d})')
        df = float(df)
        if not df > 0 or not math.isfinite(df):
            raise ValueError("'df' must be a finite number greater than zero")
        if not (np.all(np.isfinite(loc)) and np.all(np.isfinite(whiten))):
            raise ValueError('loc and whiten must be finite')
        out = _mvt_moments(self, loc, whiten, df, bool(grad))
        if not grad:
            return float(out[0]), None, None, None
        szz = np.zeros((d, d))
        szz[np.triu_indices(d)] = out[2 + d:]
        szz = szz + np.triu(szz, 1).T
        return float(out[0]), float(out[1]), out[2:2 + d].copy(), szz

    def _value_and_grads(self, loc, whiten, log_det: float, df: float, grad: bool):
        """NLL for the shape with whitening ``whiten`` and log determinant ``log_det``; with ``grad``
        also the moments and d NLL / d df."""
        from scipy.special import gammaln, psi
        n, d = self.n, self.d
        s0, s1, sz, szz = self.moments(loc, whiten, df, grad)
        c = gammaln(0.5 * (df + d)) - gammaln(0.5 * df) - d / 2. * np.log(df * np.pi) - 0.5 * log_det
        value = -n * c + 0.5 * (df + d) * s0
        if not grad:
            return float(value), None
        dc = 0.5 * psi(0.5 * (df + d)) - 0.5 * psi(0.5 * df) - d / (2. * df)
        g_df = -n * dc + 0.5 * s0 - (df + d) / (2. * df) * (n - df * s1 / (df + d))
        return float(value), (sz, szz, float(g_df))

    def _split(self, par):
        """fit_mvt's parameter vector -> (mu, A, inv(A), df); ValueError on a singular A."""
        d = self.d
        par = np.asarray(par, dtype=np.float64).reshape(-1)
        if par.shape != (d + d * (d + 1) // 2 + 1,):
            raise ValueError(f'par must have length {d + d * (d + 1) // 2 + 1}, got {par.shape[0]}')
        a = np.zeros((d, d))
        a[np.triu_indices(d)] = par[d:-1]
        diag = np.diag(a)
        if not np.all(np.isfinite(a)) or np.any(diag == 0.0):
            raise ValueError('singular shape matrix: A has a zero on its diagonal')
        from scipy.linalg import solve_triangular
        u = np.triu(solve_triangular(a, np.eye(d), lower=False))
        if not np.all(np.isfinite(u)):
            raise ValueError('singular shape matrix: A cannot be inverted')
        return par[:d], a, u, float(par[-1])

    def nll(self, par) -> float:
        """-sum multivariate_t.logpdf(sample, mu, A^T A, df) for par = [mu, triu(A), df]."""
        mu, a, u, df = self._split(par)
        log_det = 2.0 * np.sum(np.log(np.abs(np.diag(a))))
        return self._value_and_grads(mu, u, log_det, df, False)[0]

    def nll_and_grad(self, par):
        """(value, gradient) of ``nll`` in the same parametrisation, from one pass over the rows."""
        mu, a, u, df = self._split(par)
        n, d = self.n, self.d
        log_det = 2.0 * np.sum(np.log(np.abs(np.diag(a))))
        value, (sz, szz, g_df) = self._value_and_grads(mu, u, log_det, df, True)
        g_mu = -u @ sz
        g_a = np.triu((n * np.eye(d) - szz) @ u.T)
        return value, np.concatenate([g_mu, g_a[np.triu_indices(d)], [g_df]])

    def nll_scaled(self, mu, whiten_c, log_det_c: float, s: float, df: float, grad: bool = True):
        """fit_mvt2's objective: shape = exp(s) C with the fixed whitening ``whiten_c`` of C and its log
        determinant; returns the value, or (value, [d / ds, d / d df])."""
        n, d = self.n, self.d
        value, g = self._value_and_grads(mu, math.exp(-0.5 * s) * np.asarray(whiten_c), d * s + log_det_c, df, grad)
        if not grad:
            return value
        _, szz, g_df = g
        return value, np.array([0.5 * (n * d - np.trace(szz)), g_df])


def extract_t_params(par, d: int):
    """(mu, scale, df) of fit_mvt's parameter vector [mu (d), triu(A) (np.triu_indices order), df]:
    scale = A^T A (Gradient_free_Student_t.ipynb, extract_t_params)."""
    par = np.asarray(par)
    n_cov = d * (d + 1) // 2
    a = np.zeros((d, d))
    a[np.triu_indices(d)] = par[d:d + n_cov]
    return par[:d], a.T @ a, par[d + n_cov]


def _host_rows(sample) -> np.ndarray:
    return sample.detach().cpu().numpy() if hasattr(sample, 'detach') else np.asarray(sample)


def _check_jac(jac):
    if jac not in ('analytic', None):
        raise ValueError("jac must be 'analytic' or None")


def fit_mvt(Y, mu_bounds, a_bounds, df_bounds, mu_init=None, df_init=4., method='L-BFGS-B', options=None,
            jac='analytic'):
    """Maximum-likelihood multivariate t of the rows of ``Y`` -- the notebook's ``fit_mvt`` (same start
    vector: np.mean, the upper Cholesky factor of np.cov(Y, ddof=d), df_init; same bounds; the same
    scipy.optimize.minimize call; returns its OptimizeResult) with the objective on the GPU.
    ``jac='analytic'``: value and full gradient from one pass over the rows per evaluation (minimize's
    jac=True); ``jac=None``: the value only, scipy differentiating by finite differences as the
    reference does.  The rows are uploaded once per fit."""
    from scipy.optimize import minimize
    _check_jac(jac)
    lik = Y if isinstance(Y, StudentTLikelihood) else StudentTLikelihood(Y)
    rows = _host_rows(lik.sample)
    d = lik.d
    n_cov = d * (d + 1) // 2
    if mu_init is None:
        mu_init = np.mean(rows, axis=0)
    sample_cov = np.atleast_2d(np.cov(rows, rowvar=False, ddof=d))
    a = np.linalg.cholesky(sample_cov).T
    start = np.concatenate([mu_init, a[np.triu_indices(d)], [df_init]])
    lower = np.array([mu_bounds[0]] * d + [a_bounds[0]] * n_cov + [df_bounds[0]])
    upper = np.array([mu_bounds[1]] * d + [a_bounds[1]] * n_cov + [df_bounds[1]])
    bounds = list(zip(lower, upper))
    if jac == 'analytic':
        return minimize(lik.nll_and_grad, start, method=method, jac=True, bounds=bounds, options=options)
    return minimize(lik.nll, start, method=method, bounds=bounds, options=options)


def fit_mvt2(Y, scale_bounds, df_bounds, mu, scale_init=0.0, df_init=4., method='L-BFGS-B', options=None,
             jac='analytic'):
    """The notebook's ``fit_mvt2``: location ``mu`` fixed, shape = exp(scale) * np.cov(Y, ddof=d), the
    parameters (scale, df); same start, bounds and minimize call, the objective on the GPU (``jac`` as
    in ``fit_mvt``)."""
    from scipy.linalg import solve_triangular
    from scipy.optimize import minimize
    _check_jac(jac)
    lik = Y if isinstance(Y, StudentTLikelihood) else StudentTLikelihood(Y)
    rows = _host_rows(lik.sample)
    d = lik.d
    mu = np.asarray(mu, dtype=np.float64).reshape(-1)
    sample_cov = np.atleast_2d(np.cov(rows, rowvar=False, ddof=d))
    a = np.linalg.cholesky(sample_cov).T                      # C = a^T a
    whiten_c = np.triu(solve_triangular(a, np.eye(d), lower=False))
    log_det_c = 2.0 * np.sum(np.log(np.diag(a)))
    bounds = [scale_bounds, df_bounds]
    start = np.array([scale_init, df_init])
    if jac == 'analytic':
        return minimize(lambda beta: lik.nll_scaled(mu, whiten_c, log_det_c, beta[0], beta[1], True), start,
                        method=method, jac=True, bounds=bounds, options=options)
    return minimize(lambda beta: lik.nll_scaled(mu, whiten_c, log_det_c, beta[0], beta[1], False), start,
                    method=method, bounds=bounds, options=options)


MIXTURE_FIT_MAX_DIM = 16           # st_mixture_em_stats: the EM kernel's widest instantiation
MIXTURE_FIT_MAX_COMPONENTS = 32
KMEANSPP_MAX_ROWS = 16384          # the seeding looks at an evenly strided subsample of at most this many rows


def kmeanspp_seeds(rows, k: int, seed=0) -> np.ndarray:
    """k-means++ seeding on the host: the indices of ``k`` rows of ``rows`` (n, d), the first uniform, every
    further one drawn with probability proportional to its squared distance to the nearest row chosen so
    far (D^2 sampling), all from ``np.random.default_rng(seed)``.  A row at distance 0 from a chosen one is
    never drawn while any row is farther; only when every row coincides with a chosen one is the draw
    uniform.  Pure NumPy: no GPU."""
    x = np.asarray(rows, dtype=np.float64)
    if x.ndim != 2 or x.shape[0] < 1:
        raise ValueError(f'rows must be (n, d) with n >= 1, got shape {x.shape}')
    n = x.shape[0]
    if not 1 <= k <= n:
        raise ValueError(f'k must be in [1, {n}], got {k}')
    rng = np.random.default_rng(seed)
    chosen = np.empty(k, dtype=np.int64)
    chosen[0] = rng.integers(n)
    d2 = np.sum((x - x[chosen[0]]) ** 2, axis=1)
    for j in range(1, k):
        total = float(np.sum(d2))
        chosen[j] = rng.choice(n, p=d2 / total) if total > 0 else rng.integers(n)
        d2 = np.minimum(d2, np.sum((x - x[chosen[j]]) ** 2, axis=1))
    return chosen


def mixture_m_step(weight_sum: float, means, n_c, s_c, q_c, reg_covar: float):
    """The M-step from the statistics centred on the current means: ``(weights, means, covs)`` with N_c + 10 eps
    first, w_c = N_c / W, mu_c + S_c / N_c and Q_c / N_c - (S_c / N_c)(S_c / N_c)^T + reg_covar I (the update of
    scikit-learn's GaussianMixture(covariance_type='full'), written around the current mean)."""
    n_c = np.asarray(n_c, dtype=np.float64) + 10 * np.finfo(np.float64).eps
    sn = np.asarray(s_c, dtype=np.float64) / n_c[:, None]
    d = sn.shape[1]
    covs = np.asarray(q_c, dtype=np.float64) / n_c[:, None, None] - sn[:, :, None] * sn[:, None, :] + reg_covar * np.eye(d)
    return n_c / weight_sum, np.asarray(means, dtype=np.float64) + sn, covs


def _is_tensor(a) -> bool:
    return hasattr(a, 'data_ptr') and hasattr(a, 'is_cuda')


class MixtureEStep:
    """One EM pass of a Gaussian mixture over rows resident on the GPU (st_mixture_em_stats, csrc/mixture_fit.hpp).

    ``sample``: an (n, d) NumPy array (finite) or a float64 ROCm tensor (used in place, never copied to the
    host), d <= 16; ``row_weights``: None or n non-negative finite weights with a positive sum (array or
    tensor).  Everything is validated here, before any launch.  The rows, the weights, the workspace and the
    output stay on the device for the object's lifetime; ``stats`` uploads the parameters, enqueues two
    launches and brings the 1 + k (1 + d + d (d + 1) / 2) doubles back."""

    def __init__(self, sample, row_weights=None):
        tensor = _is_tensor(sample)
        if tensor:
            import torch
            if sample.dtype != torch.float64 or not sample.is_cuda:
                raise ValueError('a tensor sample must be a float64 tensor on the ROCm device')
            x = sample[:, None] if sample.ndim == 1 else sample
        else:
            x = np.ascontiguousarray(sample, dtype=np.float64)
            x = x[:, None] if x.ndim == 1 else x
        if x.ndim != 2:
            raise ValueError(f'sample must be 2-d (n, d), got shape {tuple(x.shape)}')
        self.n, self.d = int(x.shape[0]), int(x.shape[1])
        if self.n < 1 or self.d < 1:
            raise ValueError(f'sample must hold at least one row and one column, got shape {tuple(x.shape)}')
        if self.d > MIXTURE_FIT_MAX_DIM:
            raise NotImplementedError(f'd = {self.d} exceeds the EM kernel\'s maximum {MIXTURE_FIT_MAX_DIM}')
        if not tensor and not np.all(np.isfinite(x)):
            raise ValueError('sample holds non-finite values')
        self.sample = x
        self.row_weights = None
        self.weight_sum = float(self.n)
        if row_weights is not None:
            if _is_tensor(row_weights):
                import torch
                if row_weights.dtype != torch.float64 or not row_weights.is_cuda or tuple(row_weights.shape) != (self.n,):
                    raise ValueError(f'tensor row_weights must be a float64 ROCm tensor of shape ({self.n},)')
                ok = bool((torch.isfinite(row_weights) & (row_weights >= 0)).all())
                total = float(row_weights.sum()) if ok else 0.0
                w = row_weights.contiguous()
            else:
                w = np.ascontiguousarray(row_weights, dtype=np.float64)
                if w.shape != (self.n,):
                    raise ValueError(f'row_weights must have shape ({self.n},), got {w.shape}')
                ok = bool(np.all(np.isfinite(w)) and np.all(w >= 0))
                total = float(np.sum(w)) if ok else 0.0
            if not ok:
                raise ValueError('row_weights must be finite and non-negative')
            if not total > 0:
                raise ValueError('row_weights must have a positive sum')
            self.row_weights, self.weight_sum = w, total
        self._device = None

    def _state(self, k: int):
        import torch
        n, d = self.n, self.d
        st = self._device
        if st is None:
            x = self.sample
            if _is_tensor(x):
                xd = x if x.is_contiguous() else x.contiguous()
            else:
                xd = torch.from_numpy(x if x.flags.writeable else x.copy()).to(nat.require_device())
            w = self.row_weights
            if w is not None and not _is_tensor(w):
                w = torch.from_numpy(w if w.flags.writeable else w.copy()).to(xd.device)
            elif w is not None:
                w = w.to(xd.device)
            st = self._device = {'x': xd, 'w': w, 'log_p': None, 'k': {}}
        if k not in st['k']:
            wsb = int(nat.lib().st_mixture_em_workspace_bytes(n, d, k))
            if wsb < 0:
                raise NotImplementedError(f'st_mixture_em_stats: d = {d}, k = {k} is not supported')
            npar = k + k * d + k * d * d
            dev = st['x'].device
            st['k'][k] = {
                'ws': torch.empty(wsb // 8, dtype=torch.float64, device=dev),
                'out': torch.zeros(1 + k * (1 + d + d * (d + 1) // 2), dtype=torch.float64, device=dev),
                'par': torch.empty(npar, dtype=torch.float64, device=dev),
                'host': np.empty(npar),
            }
        return st, st['k'][k]

    def record(self, factors, log_p: bool = False) -> np.ndarray:
        """The raw output record for ``factors = mixture.mixture_factors(weights, means, covs)``: LL, then per
        component N_c, S_c[d] and the upper triangle of Q_c.  ``log_p=True`` also fills ``self.log_p`` (a
        device tensor (n,): the rows' log density, st_mixture_logpdf_score's bits)."""
        import torch
        log_coef, mu, precision = factors
        k, d = mu.shape
        if d != self.d:
            raise ValueError(f'the parameters have d = {d}, the sample d = {self.d}')
        if k > MIXTURE_FIT_MAX_COMPONENTS:
            raise NotImplementedError(f'k = {k} exceeds the EM kernel\'s maximum {MIXTURE_FIT_MAX_COMPONENTS}')
        st, sk = self._state(k)
        host, par = sk['host'], sk['par']
        host[:k] = log_coef
        host[k:k + k * d] = mu.reshape(-1)
        host[k + k * d:] = precision.reshape(-1)
        par.copy_(torch.from_numpy(host))
        if log_p and st['log_p'] is None:
            st['log_p'] = torch.empty(self.n, dtype=torch.float64, device=par.device)
        base = par.data_ptr()
        with torch.cuda.device(par.device):
            nat.check(nat.lib().st_mixture_em_stats(
                nat.ptr(st['x']), self.n, d, k, ctypes.c_void_p(base), ctypes.c_void_p(base + 8 * k),
                ctypes.c_void_p(base + 8 * (k + k * d)), nat.ptr(st['w']), nat.ptr(sk['out']),
                nat.ptr(st['log_p'] if log_p else None), nat.ptr(sk['ws']), sk['ws'].numel() * 8,
                nat.stream_handle()), 'st_mixture_em_stats')
            return sk['out'].cpu().numpy()

    @property
    def log_p(self):
        return None if self._device is None else self._device['log_p']

    def stats(self, weights, means, covs, log_p: bool = False):
        """(LL, N, S, Q) at the mixture ``(weights, means, covs)``: LL = sum w_i log_p_i, N (k,), S (k, d) and
        Q (k, d, d) symmetric, centred on ``means``."""
        from .mixture import mixture_factors
        rec = self.record(mixture_factors(weights, means, covs), log_p)
        return unpack_em_record(rec, np.shape(means)[0], self.d)


def unpack_em_record(rec, k: int, d: int):
    """(LL, N, S, Q) of st_mixture_em_stats' output record."""
    body = np.asarray(rec[1:]).reshape(k, 1 + d + d * (d + 1) // 2)
    q = np.zeros((k, d, d))
    iu = np.triu_indices(d)
    q[:, iu[0], iu[1]] = body[:, 1 + d:]
    q = q + np.triu(q, 1).transpose(0, 2, 1)
    return float(rec[0]), body[:, 0].copy(), body[:, 1:1 + d].copy(), q


@dataclasses.dataclass(frozen=True)
class MixtureFit:
    """The result of ``fit_mixture``: the parameters, the mean log likelihood per unit row weight AT those
    parameters, the number of evaluations, whether |ll_t - ll_{t-1}| < tol was reached, every ll_t."""
    weights: np.ndarray
    means: np.ndarray
    covs: np.ndarray
    log_likelihood: float
    n_iter: int
    converged: bool
    history: Tuple[float, ...]
    weight_sum: float
    sample: object = dataclasses.field(default=None, repr=False, compare=False)

    @property
    def n_parameters(self) -> int:
        k, d = self.means.shape
        return k - 1 + k * d + k * d * (d + 1) // 2

    @property
    def bic(self) -> float:
        """scikit-learn's GaussianMixture.bic with n = the sum of the row weights."""
        return -2.0 * self.log_likelihood * self.weight_sum + self.n_parameters * math.log(self.weight_sum)

    @property
    def aic(self) -> float:
        return -2.0 * self.log_likelihood * self.weight_sum + 2.0 * self.n_parameters

    def proxy(self, points=None):
        """(log_q, grad_log_q) of the fitted mixture at ``points`` (default: the fitted sample) through
        ``mixture_proxy``."""
        pts = self.sample if points is None else points
        if pts is None:
            raise ValueError('this fit holds no sample: pass points')
        return mixture_proxy(pts, self.weights, self.means, self.covs)


def _mixture_start(est: MixtureEStep, k, weights_init, means_init, covs_init, seed, reg_covar):
    """Start values of fit_mixture: what is given is used as it is; the means default to k-means++ seeds over
    an evenly strided subsample of at most KMEANSPP_MAX_ROWS rows (of positive weight), every covariance to
    the (weighted, biased) sample covariance + reg_covar I, the weights to 1 / k.  Of a tensor sample only that
    subsample comes to the host; its start covariance is summed on the device, so the default start of a tensor
    fit equals the host one to rounding, not bit for bit (all three ``*_init`` given: bit for bit).  Rows of
    weight 0 are left out of the seeding unless fewer than k rows of the subsample have positive weight."""
    n, d = est.n, est.d
    x, rw = est.sample, est.row_weights
    tensor = _is_tensor(x)
    if means_init is None:
        stride = -(-n // KMEANSPP_MAX_ROWS)
        sub = x[::stride]
        sub = sub.detach().cpu().numpy() if tensor else sub
        if rw is not None:
            sw = rw[::stride]
            sw = sw.detach().cpu().numpy() if _is_tensor(sw) else sw
            keep = sw > 0
            if int(np.count_nonzero(keep)) >= k:
                sub = sub[keep]
        if not np.all(np.isfinite(sub)):
            raise ValueError('sample holds non-finite values')
        means = sub[kmeanspp_seeds(sub, k, seed)].copy()
    else:
        means = np.array(means_init, dtype=np.float64)
        if means.shape != (k, d):
            raise ValueError(f'means_init must be ({k}, {d}), got {means.shape}')
    if covs_init is None:
        if tensor:
            import torch
            w = torch.ones(n, dtype=torch.float64, device=x.device) if rw is None else \
                (rw if _is_tensor(rw) else torch.from_numpy(np.array(rw)).to(x.device))
            m = (w[:, None] * x).sum(0) / est.weight_sum
            c = x - m
            cov = ((w[:, None] * c).T @ c / est.weight_sum).cpu().numpy()
        else:
            w = None if rw is None else (rw.detach().cpu().numpy() if _is_tensor(rw) else rw)
            m = np.average(x, axis=0, weights=w)
            c = x - m
            cov = (c.T * (1.0 if w is None else w)) @ c / est.weight_sum
        cov = 0.5 * (cov + cov.T) + reg_covar * np.eye(d)
        covs = np.repeat(cov[None], k, axis=0)
    else:
        covs = np.array(covs_init, dtype=np.float64)
        if covs.shape != (k, d, d):
            raise ValueError(f'covs_init must be ({k}, {d}, {d}), got {covs.shape}')
    if weights_init is None:
        weights = np.full(k, 1.0 / k)
    else:
        weights = np.array(weights_init, dtype=np.float64)
        if weights.shape != (k,):
            raise ValueError(f'weights_init must be ({k},), got {weights.shape}')
    return weights, means, covs


def fit_mixture(sample, k: int, *, row_weights=None, weights_init=None, means_init=None, covs_init=None, seed=0,
                tol: float = 1e-3, max_iter: int = 100, reg_covar: float = 1e-6,
                collapse_repeats: bool = False) -> MixtureFit:
    """Fit a k-component Gaussian mixture (full covariances) to the rows of ``sample`` by EM, one pass over the
    device-resident rows per iteration (st_mixture_em_stats) -- the proxy of a multimodal or curved target
    for ``mixture_proxy`` / ``mixture_thin``.  The reference fits no mixture; the constants and the M-step are
    those of scikit-learn's ``GaussianMixture(covariance_type='full')``.

    With W = sum of the row weights (n without), evaluation t = 1, 2, ...: the statistics at the current
    parameters give ll_t = LL / W; stop (``converged``) when |ll_t - ll_{t-1}| < tol; otherwise the M-step
    (``mixture_m_step``) gives the next parameters.  The returned parameters are the ones ``log_likelihood`` was
    evaluated at; after ``max_iter`` evaluations ``converged`` is False and a RuntimeWarning is raised.  The
    M-step and ``mixture.mixture_factors`` run on the host: per iteration only the statistics come down and the
    parameters go up.  A float64 ROCm tensor is used in place: only the seeding's strided subsample (at most
    16 384 rows, and only when ``means_init`` is not given) comes to the host, and the default start covariance is
    summed on the device, so a tensor fit from the default start equals the NumPy-input fit to rounding; from
    given ``*_init`` it is the same bits.  Start values: ``_mixture_start``.
    ``collapse_repeats=True`` (host samples): repeated rows are sent once with their summed weights
    (``collapse_rows``); the seeding still looks at the rows as given.  ValueError / NotImplementedError
    (d > 16, k > 32) before any launch; a covariance that stops being positive definite raises as
    ``mixture_factors`` does."""
    import operator
    from .mixture import mixture_factors
    try:
        k = operator.index(k)
    except TypeError:
        raise ValueError(f'k must be an integer, got {k!r}') from None
    if k < 1:
        raise ValueError(f'k must be >= 1, got {k}')
    if k > MIXTURE_FIT_MAX_COMPONENTS:
        raise NotImplementedError(f'k = {k} exceeds the EM kernel\'s maximum {MIXTURE_FIT_MAX_COMPONENTS}')
    if not tol > 0 or not math.isfinite(tol):
        raise ValueError('tol must be finite and > 0')
    if int(max_iter) < 1:
        raise ValueError('max_iter must be >= 1')
    if not reg_covar >= 0 or not math.isfinite(reg_covar):
        raise ValueError('reg_covar must be finite and >= 0')
    if collapse_repeats and _is_tensor(sample):
        raise ValueError('collapse_repeats needs a host sample')
    est = MixtureEStep(sample, row_weights)
    if k > est.n:
        raise ValueError(f'k = {k} exceeds the number of rows {est.n}')
    weights, means, covs = _mixture_start(est, k, weights_init, means_init, covs_init, seed, float(reg_covar))
    factors = mixture_factors(weights, means, covs)          # every check of the start values, before any launch
    kept = est.sample
    if collapse_repeats:
        base = np.ones(est.n) if est.row_weights is None else np.asarray(est.row_weights)
        unique, summed, _ = collapse_rows(est.sample, base)
        est = MixtureEStep(unique, summed)
    total = est.weight_sum
    history = []
    converged = False
    for t in range(1, int(max_iter) + 1):
        if t > 1:
            factors = mixture_factors(weights, means, covs)
        ll_sum, n_c, s_c, q_c = unpack_em_record(est.record(factors), k, est.d)
        if not math.isfinite(ll_sum):
            raise ValueError('the log likelihood is not finite: the sample holds non-finite rows of positive weight, '
                             'or every component has weight 0')
        history.append(ll_sum / total)
        if t > 1 and abs(history[-1] - history[-2]) < tol:
            converged = True
            break
        if t == int(max_iter):
            break
        weights, means, covs = mixture_m_step(total, means, n_c, s_c, q_c, float(reg_covar))
    if not converged:
        import warnings
        warnings.warn(f'fit_mixture: no convergence to tol = {tol} in {max_iter} evaluations', RuntimeWarning)
    return MixtureFit(weights, means, covs, history[-1], len(history), converged, tuple(history), total, kept)


def mixture_fit_thin(sample, log_p, k: int, thinned_size: int, range_cap: Optional[float] = 200, **fit_kwargs) -> np.ndarray:
    """``fit_mixture(sample, k, **fit_kwargs)`` followed by ``mixture_thin`` with the fitted parameters."""
    fit = fit_mixture(sample, k, **fit_kwargs)
    rows = _host_rows(sample)
    return mixture_thin(rows, log_p, fit.weights, fit.means, fit.covs, thinned_size, range_cap=range_cap)


from .mixture import mixture_logpdf_score as mixture_proxy  # noqa: E402  (mixture.py imports _psd from here)
