"""Convergence diagnostics on the GPU: rank-normalised split R-hat, effective sample sizes and Monte-Carlo
standard errors of ``(C, n, d)`` chains (Vehtari, Gelman, Simpson, Carpenter, Buerkner 2021), the columns the
reference's ``Sampling.ipynb`` reads from ``az.summary``.  This is the project's own statement of the paper's
definitions (tests/convergence_ref.py); it does not claim arviz's bits.

Every pass over the draws that the definitions need -- tie runs, ranks and the inverse normal cdf
(``st_rank_normalize``), the means, lag-0 values and autocovariances of every split chain (``st_autocov``) --
is a HIP kernel; ``torch`` sorts (as it does for the 'med' preconditioner), splits the chains and forms the
elementwise series one quantity at a time.  The host sees per-series means and chain-averaged
autocovariances only, asked for in growing lag blocks until Geyer's initial positive sequence has ended.
"""
from __future__ import annotations

import contextlib
import dataclasses
import math
import time
from typing import Optional, Sequence

import numpy as np

from . import _native as nat

# lags of the first st_autocov call; every later call doubles the lags held (a chain
# with tau up to ~30 ends inside the first block)
FIRST_LAGS = 64
# no call's workspace exceeds this many bytes (the lag block is halved until it fits)
MAX_WORKSPACE_BYTES = 1 << 30
COLUMNS = ('mean', 'sd', 'mcse_mean', 'mcse_sd', 'ess_bulk', 'ess_tail', 'r_hat')


def geyer_ess(ac: np.ndarray, n_series: int, h: int, var_of_means: float, full: bool = True):
    """(ess, max_t) from the chain-averaged autocovariances ``ac[0:K]`` of ``n_series`` series of length ``h``
    (``var_of_means``: np.var of the series means, ddof = 1; unused for one series), in the operation order
    of DESIGN.md section 20.  ``full=False``: None when the positive-sequence loop needs a lag >= K."""
    S = int(n_series)
    K = ac.shape[0]
    mean_var = ac[0] * h / (h - 1)
    var_plus = mean_var * (h - 1) / h
    if S > 1:
        var_plus = var_plus + var_of_means
    # The definition's loops, vectorised without changing a rounding.  The positive-sequence loop visits the
    # pairs (rho[2k], rho[2k + 1]) at t = 2k + 1 and stops at the first whose sum is not > 0 or whose t >= h - 3.
    raw = 1 - (mean_var - ac) / var_plus
    raw[0] = 1.0
    pairs = K // 2
    sums = raw[0:2 * pairs:2] + raw[1:2 * pairs:2]
    stop = ~(sums > 0) | (2 * np.arange(pairs) + 1 >= h - 3)
    if not stop.any():
        if full:
            raise ValueError(f'geyer_ess: lag {2 * pairs + 1} needed, {K} given')
        return None
    ks = int(np.argmax(stop))
    rho = np.zeros(h, dtype=ac.dtype)
    rho[:2 * ks] = raw[:2 * ks]
    if ks == 0:
        rho[:2] = raw[:2]
    elif sums[ks] >= 0:
        rho[2 * ks:2 * ks + 2] = raw[2 * ks:2 * ks + 2]
    max_t = 2 * ks - 1
    if raw[2 * ks] > 0:
        rho[max_t + 1] = raw[2 * ks]
    # The monotone pass replaces a pair whose sum exceeds the previous (already replaced) pair's by twice that
    # pair's mean; halving and doubling are exact, so the replaced sums are the running minimum of the sums.
    if ks >= 2:
        q = sums[:ks]
        low = np.minimum.accumulate(q)
        k = np.nonzero(q[1:] > low[:-1])[0] + 1
        rho[2 * k] = low[k - 1] / 2
        rho[2 * k + 1] = rho[2 * k]
    tau = -1 + 2 * np.sum(rho[:max_t + 1]) + rho[max_t + 1]
    tau = max(tau, 1 / np.log10(ac.dtype.type(S * h)))
    return S * h / tau, max_t


def _lerp_quantile(lo: float, hi: float, g: float) -> float:
    """NumPy's linear interpolation between two neighbouring order statistics (np.quantile, method 'linear')."""
    lo, hi, g = np.float64(lo), np.float64(hi), np.float64(g)
    d = hi - lo
    out = lo + d * g
    if g >= 0.5:
        out = hi - d * (1 - g)
    if g == 1:
        out = hi
    return float(out)


class _Stages:
    """Per-stage wall times (tools/convergence_bench.py): each stage is closed by a device synchronisation."""

    def __init__(self, enabled: bool):
        self.enabled = enabled
        self.seconds = {}

    @contextlib.contextmanager
    def __call__(self, name: str):
        if not self.enabled:
            yield
            return
        import torch
        torch.cuda.synchronize()
        t = time.perf_counter()
        yield
        torch.cuda.synchronize()
        self.seconds[name] = self.seconds.get(name, 0.0) + time.perf_counter() - t


def _as_chains(x):
    """The (d, C, n) contiguous float64 device tensor of an input ``(C, n, d)`` or ``(n, d)``."""
    import torch
    if isinstance(x, torch.Tensor):
        if x.dtype != torch.float64:
            raise ValueError(f'convergence: tensors must be float64 (got {x.dtype})')
        if x.ndim not in (2, 3):
            raise ValueError(f'convergence: expected (C, n, d) or (n, d) chains, got {x.ndim} dimensions')
        t = x
    else:
        h = np.asarray(x)
        if h.ndim not in (2, 3):
            raise ValueError(f'convergence: expected (C, n, d) or (n, d) chains, got {h.ndim} dimensions')
        t = None
    shape = tuple(t.shape) if t is not None else h.shape
    if len(shape) == 2:
        shape = (1,) + shape
    if shape[1] < 8:
        raise ValueError(f'convergence: need n >= 8 draws per chain (got {shape[1]})')
    if shape[0] < 1 or shape[2] < 1:
        raise ValueError(f'convergence: empty input {shape}')
    dev = nat.require_device()
    if t is None:
        t = torch.from_numpy(np.ascontiguousarray(h, dtype=np.float64)).to(dev)
    elif not t.is_cuda:
        t = t.to(dev)
    return t.reshape(shape).permute(2, 0, 1).contiguous()


def _split(a):
    """split of (d, C, n): (d, 2C, h), the first and the last h = n // 2 draws of every chain."""
    import torch
    n = a.shape[2]
    h = n // 2
    return torch.cat([a[:, :, :h], a[:, :, n - h:]], dim=1).contiguous()


def autocov(series, lag0: int, lag1: int, plan: int = 0, per_series: bool = False):
    """st_autocov on a (G, S, h) float64 device tensor: (acov_mean (G, lag1 - lag0), series_mean (G, S),
    series_var0 (G, S)[, acov_series (G, S, lag1 - lag0)]) as device tensors."""
    import torch
    G, S, h = series.shape
    L = nat.lib()
    nb = int(L.st_autocov_workspace_bytes(G, S, h, lag0, lag1, plan))
    if nb < 0:   # the shape is rejected before anything is read or written: the call only fetches the reason
        q = nat.ptr(series)
        nat.check(L.st_autocov(q, G, S, h, lag0, lag1, plan, q, q, q, None, q, 0, None), 'st_autocov')
    dev = series.device
    ws = torch.empty(max(1, nb // 8), dtype=torch.float64, device=dev)
    ac = torch.empty((G, lag1 - lag0), dtype=torch.float64, device=dev)
    mu = torch.empty((G, S), dtype=torch.float64, device=dev)
    v0 = torch.empty((G, S), dtype=torch.float64, device=dev)
    ser = torch.empty((G, S, lag1 - lag0), dtype=torch.float64, device=dev) if per_series else None
    nat.check(L.st_autocov(nat.ptr(series), G, S, h, lag0, lag1, plan, nat.ptr(ac), nat.ptr(mu), nat.ptr(v0),
                           nat.ptr(ser), nat.ptr(ws), ws.numel() * 8, nat.stream_handle()), 'st_autocov')
    return (ac, mu, v0, ser) if per_series else (ac, mu, v0)


def rank_normalize(values, want_p: bool = False):
    """z (and p) of a (vars, N) float64 device tensor, each row ranked on its own (st_rank_normalize)."""
    import torch
    vals, perm = torch.sort(values, dim=1, stable=True)
    return _rank_sorted(vals, perm, want_p)


def _rank_sorted(vals, perm, want_p: bool = False):
    import torch
    vals, perm = vals.contiguous(), perm.contiguous()
    z = torch.empty_like(vals)
    p = torch.empty_like(vals) if want_p else None
    nat.check(nat.lib().st_rank_normalize(nat.ptr(vals), nat.ptr(perm), vals.shape[0], vals.shape[1], nat.ptr(p),
                                          nat.ptr(z), nat.stream_handle()), 'st_rank_normalize')
    return (z, p) if want_p else z


def _block_end(G: int, S: int, h: int, lag0: int, want: int) -> int:
    """End of the lag block that starts at lag0: ``want`` lags, fewer when the workspace would pass the cap."""
    L = nat.lib()
    lag1 = min(h, lag0 + want)
    while lag1 - lag0 > FIRST_LAGS and \
            int(L.st_autocov_workspace_bytes(G, S, h, lag0, lag1, 0)) > MAX_WORKSPACE_BYTES:
        lag1 = lag0 + (lag1 - lag0) // 2
    return lag1


def _series_stats(series, stages):
    """What the host needs of a (G, S, h) quantity: ess (G,), and rhat (G,) of it."""
    import torch
    G, S, h = series.shape
    with stages('autocov'):
        lo, hi = torch.aminmax(series.reshape(G, -1), dim=1)
        lag1 = _block_end(G, S, h, 0, FIRST_LAGS)
        ac_d, mu_d, v0_d = autocov(series, 0, lag1)
        const = ((hi - lo) < 1e-15).cpu().numpy()
        ac0 = ac_d.cpu().numpy()
        mu = mu_d.cpu().numpy()
        v0 = v0_d.cpu().numpy()
    ess = np.empty(G)
    rhat = np.empty(G)
    for g in range(G):
        var_mu = float(np.var(mu[g], ddof=1)) if S > 1 else 0.0
        with np.errstate(all='ignore'):
            W = np.mean(v0[g] * h / (h - 1))
            B = h * var_mu
            rhat[g] = np.sqrt((B / W + h - 1) / h)
        if const[g]:
            ess[g] = S * h
            continue
        ac = ac0[g]
        while True:
            with stages('geyer'):
                res = geyer_ess(ac, S, h, var_mu, full=ac.shape[0] >= h)
            if res is not None:
                ess[g] = res[0]
                break
            k = ac.shape[0]
            with stages('autocov'):
                lag1 = _block_end(1, S, h, k, k)
                more, _, _ = autocov(series[g:g + 1], k, lag1)
                ac = np.concatenate([ac, more[0].cpu().numpy()])
    return ess, rhat


def _rhat_only(series, stages):
    import torch  # noqa: F401
    G, S, h = series.shape
    with stages('autocov'):
        _, mu_d, v0_d = autocov(series, 0, 1)
        mu, v0 = mu_d.cpu().numpy(), v0_d.cpu().numpy()
    out = np.empty(G)
    with np.errstate(all='ignore'):
        for g in range(G):
            W = np.mean(v0[g] * h / (h - 1))
            B = h * float(np.var(mu[g], ddof=1))
            out[g] = np.sqrt((B / W + h - 1) / h)
    return out


def _compute(x, want: Sequence[str], stages: Optional[_Stages] = None) -> dict:
    """The requested quantities ('mean', 'sd', 'ess_mean', 'ess_sd', 'ess_bulk', 'ess_tail', 'r_hat') as (d,)
    arrays.  Each transformed series is formed, used and dropped before the next one."""
    import torch
    stages = stages or _Stages(False)
    want = set(want)
    a = _as_chains(x)
    d, C, n = a.shape
    bad = (~torch.isfinite(a).reshape(d, -1).all(dim=1))
    bad_h = bad.cpu().numpy()
    if bad_h.any():
        a = torch.where(bad[:, None, None], torch.zeros((), dtype=a.dtype, device=a.device), a)
    out = {}
    N = C * n
    # mean and sd of all C n values from the chains' own means and lag-0 values
    with stages('autocov'):
        _, mu_d, v0_d = autocov(a, 0, 1)
        mu_c, v0_c = mu_d.cpu().numpy(), v0_d.cpu().numpy()
    mean = np.array([np.mean(mu_c[k]) for k in range(d)])
    ss = np.array([np.sum(v0_c[k] * n) + n * np.sum((mu_c[k] - mean[k]) ** 2) for k in range(d)])
    out['mean'] = mean
    out['sd'] = np.sqrt(ss / (N - 1))
    sp = _split(a)
    if 'ess_mean' in want or 'ess_sd' in want:
        out['ess_mean'], _ = _series_stats(sp, stages)
    if 'ess_sd' in want:
        m = torch.from_numpy(mean).to(a.device)[:, None, None]
        sq = (sp - m) ** 2
        e2, _ = _series_stats(sq, stages)
        del sq
        out['ess_sd'] = np.minimum(out['ess_mean'], e2)
    if 'ess_bulk' in want or 'r_hat' in want:
        with stages('sort'):
            vals, perm = torch.sort(sp.reshape(d, -1), dim=1, stable=True)
        with stages('rank'):
            z = _rank_sorted(vals, perm).reshape(sp.shape)
        del vals, perm
        if 'ess_bulk' in want:
            out['ess_bulk'], r_bulk = _series_stats(z, stages)
        else:
            r_bulk = _rhat_only(z, stages)
        del z
    if 'ess_tail' in want or 'r_hat' in want:
        with stages('sort'):
            allv = torch.sort(a.reshape(d, -1), dim=1).values

        def order_stat(q):
            virt = (N - 1) * q
            j = int(math.floor(virt))
            j2 = min(j + 1, N - 1)
            pair = allv[:, [j, j2]].cpu().numpy()
            return np.array([_lerp_quantile(pair[k, 0], pair[k, 1], virt - j) for k in range(d)])
        if 'ess_tail' in want:
            tails = []
            for q in (0.05, 0.95):
                Q = torch.from_numpy(order_stat(q)).to(a.device)[:, None, None]
                ind = (sp <= Q).to(torch.float64)
                tails.append(_series_stats(ind, stages)[0])
                del ind
            out['ess_tail'] = np.minimum(tails[0], tails[1])
        if 'r_hat' in want:
            mid = allv[:, [(N - 1) // 2, N // 2]].cpu().numpy()
            med = torch.from_numpy(np.array([np.mean(mid[k]) for k in range(d)])).to(a.device)[:, None, None]
            folded = (sp - med).abs()
            with stages('sort'):
                vals, perm = torch.sort(folded.reshape(d, -1), dim=1, stable=True)
            del folded
            with stages('rank'):
                zf = _rank_sorted(vals, perm).reshape(sp.shape)
            del vals, perm
            r_fold = _rhat_only(zf, stages)
            del zf
            with np.errstate(all='ignore'):
                out['r_hat'] = np.where(np.isnan(r_bulk) | np.isnan(r_fold), np.nan, np.maximum(r_bulk, r_fold))
        del allv
    for v in out.values():
        v[bad_h] = np.nan
    return out


def ess(x, method: str = 'bulk') -> np.ndarray:
    """Effective sample size of every variable of ``x`` ((C, n, d) or (n, d); a NumPy array or a float64
    tensor, host or device): ``method`` 'bulk', 'tail', 'mean' or 'sd'."""
    if method not in ('bulk', 'tail', 'mean', 'sd'):
        raise ValueError(f"ess: method {method!r}: expected 'bulk', 'tail', 'mean' or 'sd'")
    return _compute(x, ['ess_' + method])['ess_' + method]


def rhat(x) -> np.ndarray:
    """Rank-normalised split R-hat (the larger of the bulk and the folded value) of every variable."""
    return _compute(x, ['r_hat'])['r_hat']


def _mcse(res: dict, method: str) -> np.ndarray:
    sd = res['sd']
    with np.errstate(all='ignore'):
        if method == 'mean':
            return sd / np.sqrt(res['ess_mean'])
        e = res['ess_sd']
        # sd sqrt(e (1 - 1/E)^(E - 1) - 1): the bracket is about 1 / (2 E), so it is taken as expm1 of the
        # exponent's distance from -1 and not as the difference of two numbers near 1
        return sd * np.sqrt(np.expm1(1 + (e - 1) * np.log1p(-1 / e)))


def mcse(x, method: str = 'mean') -> np.ndarray:
    """Monte-Carlo standard error of the mean ('mean') or of the standard deviation ('sd')."""
    if method not in ('mean', 'sd'):
        raise ValueError(f"mcse: method {method!r}: expected 'mean' or 'sd'")
    return _mcse(_compute(x, ['ess_' + method]), method)


@dataclasses.dataclass
class Summary:
    """The notebook's ``az.summary`` columns (without the hdi pair), one entry per variable."""
    mean: np.ndarray
    sd: np.ndarray
    mcse_mean: np.ndarray
    mcse_sd: np.ndarray
    ess_bulk: np.ndarray
    ess_tail: np.ndarray
    r_hat: np.ndarray
    var_names: Optional[Sequence[str]] = None

    def to_frame(self):
        """A pandas DataFrame with arviz's column names, one row per variable."""
        import pandas as pd
        d = self.mean.shape[0]
        names = list(self.var_names) if self.var_names is not None else [f'x[{k}]' for k in range(d)]
        return pd.DataFrame({c: getattr(self, c) for c in COLUMNS}, index=names)


def summary(x, var_names: Optional[Sequence[str]] = None, _stages: Optional[_Stages] = None) -> Summary:
    """mean, sd, mcse_mean, mcse_sd, ess_bulk, ess_tail and r_hat of every variable of ``x``: (C, n, d) or
    (n, d) chains, a NumPy array or a float64 tensor -- a sampler result's ``.samples`` as it is, on the
    device or not."""
    res = _compute(x, ['ess_mean', 'ess_sd', 'ess_bulk', 'ess_tail', 'r_hat'], _stages)
    d = res['mean'].shape[0]
    if var_names is not None and len(var_names) != d:
        raise ValueError(f'summary: {len(var_names)} names for {d} variables')
    return Summary(res['mean'], res['sd'], _mcse(res, 'mean'), _mcse(res, 'sd'), res['ess_bulk'],
                   res['ess_tail'], res['r_hat'], var_names)
