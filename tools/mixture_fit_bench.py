"""Timing of the Gaussian-mixture fit (st_mixture_em_stats, proxy.fit_mixture) -> profiles/mixture_fit_bench.json.

Per shape n:d:k, in one process, alternating windows of ``--launches`` back-to-back launches between HIP events
(median of ``--reps`` windows; the torch leg gets a tenth of the launches; every leg's window length is recorded
as ``*_window_s``):
  * em_pass_s      -- st_mixture_em_stats alone (both launches) on device-resident rows and parameters;
  * e_step_s       -- st_mixture_logpdf_score at the same shape: the E-step's work alone, with its score output;
  * torch_s        -- the same statistics built from torch ops on the device (broadcast E-step, einsum moments);
  * roofline_s     -- the rows read once (n d 8 bytes) at ``--peak-tbs`` TB/s;
then a whole fit_mixture from host arrays and from a device tensor (wall clock, with its iteration count) and,
where scikit-learn imports, GaussianMixture.fit on the host from the same start (``sklearn_status`` says whether
it was timed, not available, or left out for a shape of more than ``--sklearn-max`` n d k).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'gradient-free-mcmc-postprocessing_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)


def planted(n, d, k, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    a = rng.normal(size=(k, d, d))
    covs = a @ a.transpose(0, 2, 1) / d + 0.5 * np.eye(d)
    means = rng.normal(size=(k, d))
    for c in range(k):
        means[c, c % d] += 3.0 * (c // d + 1) * (1 if (c // d) % 2 == 0 else -1) + 3.0 * (c % d)
    w = rng.dirichlet(np.full(k, 5.0))
    comp = rng.choice(k, size=n, p=w)
    chol = np.linalg.cholesky(covs)
    x = means[comp] + np.einsum('nij,nj->ni', chol[comp], rng.normal(size=(n, d)))
    return x, w, means + 0.3 * rng.normal(size=(k, d)), covs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='500000:4:2,500000:4:8,2000000:4:2,2000000:4:8,500000:16:4')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--fit-reps', type=int, default=3)
    ap.add_argument('--sklearn-max', type=float, default=2e7, help='largest n d k scikit-learn is timed at')
    ap.add_argument('--peak-tbs', type=float, default=8.0, help='HBM peak of the device, TB/s')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mixture_fit_bench.json'))
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit('mixture_fit_bench needs a HIP device: timings on a CPU say nothing about the GPU')
    from stein_thinning import _native as nat
    from stein_thinning import mixture, proxy
    dev = nat.require_device()
    lib = nat.lib()
    try:
        from sklearn.mixture import GaussianMixture
    except ImportError:
        GaussianMixture = None

    def window(fn, launches):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(launches):
            fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) * 1e-3 / launches

    out = {'tool': 'mixture_fit_bench', 'device': torch.cuda.get_device_name(0), 'reps': args.reps,
           'launches_per_window': args.launches, 'peak_tbs': args.peak_tbs,
           'scikit_learn': None if GaussianMixture is None else __import__('sklearn').__version__, 'shapes': []}
    for spec in args.shapes.split(','):
        n, d, k = (int(v) for v in spec.split(':'))
        x, w, means, covs = planted(n, d, k, 100 * d + k)
        log_coef, mu, prec = mixture.mixture_factors(w, means, covs)
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)   # noqa: E731
        xd, cd, md, pd = to(x), to(log_coef), to(mu), to(prec)
        e = 1 + d + d * (d + 1) // 2
        rec_out = torch.zeros(1 + k * e, dtype=torch.float64, device=dev)
        ws = torch.empty(int(lib.st_mixture_em_workspace_bytes(n, d, k)) // 8, dtype=torch.float64, device=dev)
        log_p = torch.empty(n, dtype=torch.float64, device=dev)
        score = torch.empty((n, d), dtype=torch.float64, device=dev)
        stream = nat.stream_handle()

        def run_em():
            nat.check(lib.st_mixture_em_stats(nat.ptr(xd), n, d, k, nat.ptr(cd), nat.ptr(md), nat.ptr(pd), None,
                                              nat.ptr(rec_out), None, nat.ptr(ws), ws.numel() * 8, stream),
                      'st_mixture_em_stats')

        def run_e_step():
            nat.check(lib.st_mixture_logpdf_score(nat.ptr(xd), n, d, k, nat.ptr(cd), nat.ptr(md), nat.ptr(pd),
                                                  nat.ptr(log_p), nat.ptr(score), stream), 'st_mixture_logpdf_score')

        def run_torch():
            dv = xd[None, :, :] - md[:, None, :]                                  # (k, n, d)
            y = torch.einsum('cjk,cnk->cnj', pd, dv)
            l = cd[:, None] - 0.5 * (dv * y).sum(-1)
            lp = torch.logsumexp(l, dim=0)
            r = torch.exp(l - lp)
            return lp.sum(), r.sum(1), torch.einsum('cn,cni->ci', r, dv), torch.einsum('cn,cni,cnj->cij', r, dv, dv)

        legs = {'em_pass_s': run_em, 'e_step_s': run_e_step, 'torch_s': run_torch}
        for fn in legs.values():
            window(fn, 3)
        times = {name: [] for name in legs}
        count = {name: args.launches if name != 'torch_s' else max(2, args.launches // 10) for name in legs}
        for _ in range(args.reps):          # alternating
            for name, fn in legs.items():
                times[name].append(window(fn, count[name]))
        rec = {'n': n, 'd': d, 'k': k}
        for name, v in times.items():
            rec[name] = statistics.median(v)
            rec[name + '_min'], rec[name + '_max'] = min(v), max(v)
            rec[name[:-2] + '_window_s'] = rec[name] * count[name]
        rec['roofline_s'] = 8.0 * n * d / (args.peak_tbs * 1e12)
        rec['em_over_e_step'] = rec['em_pass_s'] / rec['e_step_s']
        rec['torch_over_em'] = rec['torch_s'] / rec['em_pass_s']
        rec['em_over_roofline'] = rec['em_pass_s'] / rec['roofline_s']
        # the timed launch against the torch statistics (another summation order: to rounding)
        run_em()
        got = rec_out.cpu().numpy()
        t_ll, t_n, t_s, t_q = (v.cpu().numpy() for v in run_torch())
        ll, n_c, s_c, q_c = proxy.unpack_em_record(got, k, d)
        rec['max_rel_diff_vs_torch'] = float(max(abs(ll - t_ll) / abs(t_ll), np.max(np.abs(n_c - t_n)) / np.max(np.abs(t_n)),
                                                 np.max(np.abs(q_c - t_q)) / np.max(np.abs(t_q))))

        start = dict(weights_init=np.full(k, 1.0 / k), means_init=means, covs_init=covs, tol=1e-3, max_iter=100)

        def wall(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn()
            torch.cuda.synchronize()
            return time.perf_counter() - t0, res
        wall(lambda: proxy.fit_mixture(xd, k, **start))
        host = [wall(lambda: proxy.fit_mixture(x, k, **start)) for _ in range(args.fit_reps)]
        tens = [wall(lambda: proxy.fit_mixture(xd, k, **start)) for _ in range(args.fit_reps)]
        rec['fit_host_s'] = statistics.median(t for t, _ in host)
        rec['fit_tensor_s'] = statistics.median(t for t, _ in tens)
        rec['fit_n_iter'] = tens[0][1].n_iter
        rec['fit_log_likelihood'] = tens[0][1].log_likelihood
        if GaussianMixture is None:
            rec['sklearn_status'] = 'scikit-learn not available'
        elif n * d * k > args.sklearn_max:
            rec['sklearn_status'] = f'left out: n d k = {n * d * k} exceeds --sklearn-max {args.sklearn_max:g}'
        else:
            rec['sklearn_status'] = 'timed'
            gm = GaussianMixture(k, covariance_type='full', tol=1e-3, max_iter=100, reg_covar=1e-6,
                                 weights_init=start['weights_init'], means_init=means, precisions_init=np.linalg.inv(covs))
            t0 = time.perf_counter()
            gm.fit(x)
            rec['sklearn_fit_s'] = time.perf_counter() - t0
            rec['sklearn_n_iter'] = int(gm.n_iter_)
            rec['sklearn_log_likelihood'] = float(gm.lower_bound_)
        print(json.dumps(rec), flush=True)
        out['shapes'].append(rec)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
