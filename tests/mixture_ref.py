"""Shared helper of the Gaussian-mixture tests (tests/test_mixture_cpu.py, tests/test_gpu_mixture.py):
the seeded recipe and a numerically stable restatement of the mixture's log density and score.

Recipe (``case(n, d, k)``): ``rng = default_rng(100 d + k)``; means = 2 N(0, 1); cov_c = A A^T / d +
0.3 I (A standard normal: condition numbers stay <= 18); w ~ Dirichlet(2, ..., 2); every row is drawn
from a component chosen with probabilities w, spread x 1.5.  Draw order: A, means, w, then the rows'
standard normals, then their components.

``stable(x, w, means, covs, dtype)`` restates the definition in log space (logsumexp over the
components, softmax-weighted score) in float64 or ``np.longdouble``, from the same float64 precision
matrices ``np.linalg.inv(covs)`` and ``np.linalg.slogdet(covs)``: finite where the oracle's sum of
densities (``oracle.models.make_mvn_mixture``) underflows.

On the recipe (n = 2000, d in DIMS, k in COMPONENTS) the oracle is finite everywhere and within 1e-14
of the long-double restatement relative to max(|want|.max(), 1) (tests/test_mixture_cpu.py checks it),
so the project's proxy tolerance RTOL = 1e-12 (``close``, as tests/test_gpu_proxy.py::_close) has
about 100x headroom.
"""
import functools

import numpy as np

RTOL = 1e-12
DIMS = [1, 2, 3, 4, 8, 9, 16, 17, 33, 50, 64]
COMPONENTS = [1, 2, 3, 7]


def close(got, want):
    scale = max(float(np.abs(want).max()), 1.0) if want.size else 1.0
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=RTOL * scale)


def parameters(d, k):
    """(rng, weights, means, covs) of the recipe; the rng is positioned after the parameter draws."""
    rng = np.random.default_rng(100 * d + k)
    a = rng.normal(size=(k, d, d))
    covs = a @ a.transpose(0, 2, 1) / d + 0.3 * np.eye(d)
    means = 2.0 * rng.normal(size=(k, d))
    weights = rng.dirichlet(np.full(k, 2.0))
    return rng, weights, means, covs


def rows(rng, n, weights, means, covs, spread=1.5):
    k, d = means.shape
    z = rng.normal(size=(n, d))
    comp = rng.choice(k, size=n, p=weights)
    chol = np.linalg.cholesky(covs)
    return means[comp] + spread * np.einsum('nij,nj->ni', chol[comp], z)


@functools.lru_cache(maxsize=None)
def case(n, d, k):
    """(x, weights, means, covs), read-only: computed once per shape and shared."""
    rng, weights, means, covs = parameters(d, k)
    x = rows(rng, n, weights, means, covs)
    for arr in (x, weights, means, covs):
        arr.setflags(write=False)
    return x, weights, means, covs


@functools.lru_cache(maxsize=None)
def oracle(n, d, k):
    """The oracle's (logpdf, score) on case(n, d, k), computed once."""
    from oracle import models
    x, weights, means, covs = case(n, d, k)
    _, logpdf, score = models.make_mvn_mixture(weights, means, covs)
    out = np.atleast_1d(logpdf(x)), score(x)
    for arr in out:
        arr.setflags(write=False)
    return out


def stable(x, weights, means, covs, dtype=np.float64):
    """(log_p, score) by logsumexp over the components, in ``dtype``."""
    x = np.asarray(x, dtype=np.float64)
    means = np.asarray(means, dtype=np.float64)
    covs = np.asarray(covs, dtype=np.float64)
    k, d = means.shape
    prec = np.linalg.inv(covs).astype(dtype)
    _, logdet = np.linalg.slogdet(covs)
    with np.errstate(divide='ignore'):
        log_w = np.log(np.asarray(weights, dtype=dtype))
    a = log_w - (d * np.log(2 * np.pi * np.ones((), dtype=dtype)) + logdet.astype(dtype)) / 2
    dev = x.astype(dtype)[None, :, :] - means.astype(dtype)[:, None, :]          # (k, n, d)
    y = np.einsum('cjk,cnk->cnj', prec, dev)
    q = np.sum(dev * y, axis=-1)
    l = a[:, None] - q / 2                                                           # (k, n)
    m = np.max(l, axis=0)
    e = np.exp(l - m)
    s = np.sum(e, axis=0)
    log_p = m + np.log(s)
    score = -np.einsum('cn,cnj->nj', e, y) / s[:, None]
    return log_p, score
