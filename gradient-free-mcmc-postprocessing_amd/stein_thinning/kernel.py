"""``stein_thinning.kernel`` -- IMQ Stein kernel and preconditioners.

Mirrors the reference dependency's module (imported at
``code/notebooks/Kernel_Stein_discrepancy.ipynb`` cell 2 and ``JAX_Stein_Thinning.ipynb`` cells 15,
26): ``vfk0_imq(a, b, sa, sb, linv)``, ``make_imq(sample, preconditioner)``,
``make_precon(sample, preconditioner)``.  ``vfk0_imq`` evaluates on the GPU (HIP pair kernel);
the preconditioner is O(1000^2) host preprocessing exactly as the reference computes it ('smpcov':
the sample covariance of all n rows and a d x d inverse).
"""
from __future__ import annotations

from typing import Callable

import numpy as np
from numpy.linalg import inv
from scipy.spatial.distance import pdist

MED_SUBSAMPLE = 1000


def make_precon(sample: np.ndarray, preconditioner='id', on_device: bool = False) -> np.ndarray:
    """Gamma^-1 for the IMQ kernel (reference usage: ``make_precon(s, 'id')``,
    ``JAX_Stein_Thinning.ipynb`` cell 28; median heuristic ``report.tex:432``).

    'id' -> I; 'med' -> inv(med^2 I), med = median pairwise distance of the (standardised) sample,
    sub-sampled at ``linspace(0, n-1, 1000)`` rows when n > 1000 (sub-sampling rule: parity
    unpinned); 'sclmed' -> inv(med^2 / log(min(1000, n)) I); a number s -> inv(s I);
    'smpcov' -> the inverse sample covariance, a dense matrix: c = atleast_2d(np.cov(sample,
    rowvar=False)), (inv(c) + inv(c).T) / 2 (exactly symmetric), ValueError('Too few unique samples
    in smp.') when c has no Cholesky factor or no inverse (upstream's exact rule is recalled, not held
    by the reference: parity unpinned).  It reads every row of the sample on the host.
    ``on_device``: the median's distances computed and sorted on the GPU (device.pdist_median, the
    same bits; the drop-in thin's path, which holds the GPU anyway) instead of scipy + np.median.
    """
    sample = np.asarray(sample, dtype=np.float64)
    n, d = sample.shape
    return make_precon_rows(n, d, lambda rows: sample[rows], preconditioner, on_device)


def make_precon_rows(n: int, d: int, rows_of, preconditioner='id', on_device: bool = False,
                     med_squared=None) -> np.ndarray:
    """make_precon for an (n, d) sample given only ``rows_of(index array) -> those rows`` of it (the
    median heuristic reads its subsample rows, nothing else).  ``med_squared``: the squared median
    distance when the caller already holds it (thinning.thin_many takes every chain's on the device)."""
    def med2():
        if med_squared is not None:
            return med_squared
        idx = np.linspace(0, n - 1, MED_SUBSAMPLE, dtype=int) if n > MED_SUBSAMPLE else np.arange(n)
        sub = rows_of(idx)
        if on_device and 2 <= sub.shape[0] <= 65535:
            from .device import pdist_median
            return pdist_median(sub) ** 2
        return np.median(pdist(sub)) ** 2

    if isinstance(preconditioner, str):
        if preconditioner == 'id':
            return np.identity(d)
        if preconditioner == 'med':
            m2 = med2()
            if m2 == 0:
                raise ValueError('Too few unique samples in smp.')
            return inv(m2 * np.identity(d))
        if preconditioner == 'sclmed':
            m2 = med2()
            if m2 == 0:
                raise ValueError('Too few unique samples in smp.')
            return inv(m2 / np.log(np.minimum(MED_SUBSAMPLE, n)) * np.identity(d))
        if preconditioner == 'smpcov':
            if n < 2:
                raise ValueError('Too few unique samples in smp.')
            c = np.atleast_2d(np.cov(rows_of(np.arange(n)), rowvar=False))   # d = 1: np.cov returns a 0-d array
            try:
                np.linalg.cholesky(c)
                ci = inv(c)
            except np.linalg.LinAlgError:
                raise ValueError('Too few unique samples in smp.') from None
            return (ci + ci.T) / 2
    try:
        scale = float(preconditioner)
    except (TypeError, ValueError):
        raise ValueError('Incorrect preconditioner type.') from None
    return inv(scale * np.identity(d))


class _ResidentRows:
    """Device copy of one large (rows, scores) operand of vfk0_imq plus one spare row for the
    single-row side of a call.

    The reference's plug-in loop (``JAX_Stein_Thinning.ipynb:201-244``) calls
    ``vfk0(s[:], s[[j]], g[:], g[[j]])`` once per greedy step: the same n x d sample every time
    and one new row.  The large operand is uploaded once and re-used while the caller's arrays
    still hold exactly the same values (compared on every call, so an array changed in place is
    uploaded again); a step then copies only the new row into the spare row and launches the pair
    kernel on index vectors that stay on the device."""

    def __init__(self, x: np.ndarray, g: np.ndarray, l: float, tr: float, linv=None):
        import torch
        from .device import DeviceProblem
        self.hx, self.hg = x.copy(), g.copy()
        self.n, d = x.shape
        self.l, self.tr = l, tr
        self.linv = None if linv is None else linv.copy()   # dense preconditioner (l unused)
        pad = np.zeros((1, d))
        self.prob = DeviceProblem(np.vstack([x, pad]), np.vstack([g, pad]), None, l, tr, linv=linv)
        dev = self.prob.device
        self.rows = torch.arange(self.n, dtype=torch.int64, device=dev)
        self.spare = torch.full((self.n,), self.n, dtype=torch.int64, device=dev)

    def holds(self, x: np.ndarray, g: np.ndarray, l: float, tr: float, linv=None) -> bool:
        same_l = (linv is None) == (self.linv is None) and (linv is None or np.array_equal(linv, self.linv))
        return (x.shape == self.hx.shape and l == self.l and tr == self.tr and same_l
                and np.array_equal(x, self.hx) and np.array_equal(g, self.hg))

    def put(self, x: np.ndarray, g: np.ndarray) -> None:
        """Copy the (1, d) row into the spare row (row n of the SoA arrays)."""
        import torch
        row = torch.from_numpy(np.concatenate([x[0], g[0]])).to(self.prob.device)
        d = x.shape[1]
        self.prob.x[:, self.n] = row[:d]
        self.prob.g[:, self.n] = row[d:]


_RESIDENT: list = []      # most recently used first; at most _RESIDENT_MAX entries
_RESIDENT_MAX = 2
_RESIDENT_MIN_ROWS = 4096  # smaller operands are uploaded per call (cheaper than the comparisons)


def _resident_for(x: np.ndarray, g: np.ndarray, l: float, tr: float, linv=None) -> '_ResidentRows':
    for k, e in enumerate(_RESIDENT):
        if e.holds(x, g, l, tr, linv):
            if k:
                _RESIDENT.insert(0, _RESIDENT.pop(k))
            return e
    e = _ResidentRows(x, g, l, tr, linv)
    _RESIDENT.insert(0, e)
    del _RESIDENT[_RESIDENT_MAX:]
    return e


def vfk0_imq(a: np.ndarray, b: np.ndarray, sa: np.ndarray, sb: np.ndarray, linv: np.ndarray) -> np.ndarray:
    """IMQ Langevin Stein kernel k_P(a_i, b_i) (c = 1, beta = -1/2), evaluated by the HIP pair kernel.

    Same broadcasting as the reference (row-wise pairs; either side may have a single row).
    linv = l I ('id', 'med', 'sclmed', scalar) runs the isotropic kernel; any other symmetric
    positive-definite linv with d <= 16 ('smpcov', or a matrix of the caller's) the dense one
    (device.dense_preconditioner validates it: ValueError / NotImplementedError otherwise).
    A large operand seen in consecutive calls (the plug-in greedy loop: all rows against one) stays
    resident on the device (``_ResidentRows``); anything else is uploaded for the call.
    """
    from .device import DeviceProblem, dense_preconditioner, isotropic_scale
    a = np.atleast_2d(np.asarray(a, dtype=np.float64))
    b = np.atleast_2d(np.asarray(b, dtype=np.float64))
    sa = np.atleast_2d(np.asarray(sa, dtype=np.float64))
    sb = np.atleast_2d(np.asarray(sb, dtype=np.float64))
    if a.shape != sa.shape or b.shape != sb.shape or a.shape[1] != b.shape[1]:
        raise ValueError('inconsistent shapes for vfk0_imq')
    iso = isotropic_scale(linv)
    dense = None
    if iso is None:
        dense, tr = dense_preconditioner(linv, a.shape[1])
        iso = (0.0, tr)
    na, nb = a.shape[0], b.shape[0]
    ia, ib = np.broadcast_arrays(np.arange(na), np.arange(nb))
    big, small = max(na, nb), min(na, nb)
    if big >= _RESIDENT_MIN_ROWS:
        if small == big and np.array_equal(a, b) and np.array_equal(sa, sb):   # the diagonal
            e = _resident_for(a, sa, iso[0], iso[1], dense)
            return e.prob.pairs_device(e.rows, e.rows)
        if small == 1:                                                          # all rows vs one
            a_big = na == big
            e = _resident_for(*((a, sa) if a_big else (b, sb)), iso[0], iso[1], dense)
            e.put(*((b, sb) if a_big else (a, sa)))
            return e.prob.pairs_device(e.rows, e.spare) if a_big else e.prob.pairs_device(e.spare, e.rows)
    prob = DeviceProblem(np.vstack([a, b]), np.vstack([sa, sb]), None, iso[0], iso[1], linv=dense)
    return prob.pairs(ia.astype(np.int64), ib.astype(np.int64) + na)


def make_imq(sample: np.ndarray, preconditioner='id') -> Callable:
    linv = make_precon(sample, preconditioner)

    def vfk0(a, b, sa, sb):
        return vfk0_imq(a, b, sa, sb, linv)
    vfk0.linv = linv
    return vfk0
