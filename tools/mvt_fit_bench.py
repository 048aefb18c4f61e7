"""Multivariate-t fit timings (one JSON line, also written to --out; needs a GPU).

Shapes n:d = 5e5:4 (the reference's chain), 2e6:4 and 5e5:16 on the seeded t recipe below.  Per shape:
  * value_s / value_grad_s -- st_mvt_moments alone (both launches) on device-resident rows, want_grad 0 / 1;
  * proxy_sum_s   -- the yardstick on the device: one st_proxy_logpdf_grad (Student-t) launch on the same
                     rows followed by torch.sum of its log q -- how the likelihood could be had from the
                     code that existed before the moment kernels;
  * proxy_s       -- that launch alone;
  * nll_and_grad_call_s -- one StudentTLikelihood.nll_and_grad call from Python: parameter upload, the two
                     launches, the copy back, the host algebra (wall clock, median);
  * fit_s / fit_nfev -- a whole fit_mvt (analytic gradient) on the resident rows, and fit_upload_s with
                     the upload of the host array in front;
  * objective_host_s_extrapolated -- the reference's objective (-sum scipy multivariate_t.logpdf) timed on
                     --host-rows rows and scaled by n / rows (labelled: extrapolated, not measured at n).
The device legs alternate in one process after a warm-up; each window is --launches back-to-back calls
between two device events, the per-call time is the window over its calls, the figure the median of
--reps windows.  bytes_s is the rows' bytes (read once) over the kernel time.
"""
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


def t_case(n, d, seed):
    """Seeded t rows: Sigma = (M M^T / d + I) 1e-2, loc = 0.1 N(0, 1), df = 5."""
    import numpy as np
    rng = np.random.default_rng(seed)
    m = rng.normal(size=(d, d))
    sigma = (m @ m.T / d + np.eye(d)) * 1e-2
    loc = 0.1 * rng.normal(size=d)
    g = rng.normal(size=(n, d)) @ np.linalg.cholesky(sigma).T
    return loc + g / np.sqrt(rng.chisquare(5.0, size=n) / 5.0)[:, None], loc, sigma, 5.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='500000:4,2000000:4,500000:16', help='n:d,...')
    ap.add_argument('--reps', type=int, default=20, help='timed windows per device leg (>= 5)')
    ap.add_argument('--launches', type=int, default=50, help='calls per window')
    ap.add_argument('--call-reps', type=int, default=50)
    ap.add_argument('--fit-reps', type=int, default=3)
    ap.add_argument('--host-rows', type=int, default=100000)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mvt_fit_bench.json'))
    args = ap.parse_args()
    if args.reps < 5:
        ap.error('--reps must be >= 5')

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit('mvt_fit_bench needs a HIP device: timings on a CPU say nothing about the GPU')
    from scipy import stats
    from scipy.special import gammaln
    from stein_thinning import _native as nat
    from stein_thinning import proxy
    dev = nat.require_device()
    lib = nat.lib()

    def window(fn, launches):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(launches):
            fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) * 1e-3 / launches

    bounds = dict(mu_bounds=(-1.0, 1.0), a_bounds=(-1.0, 1.0), df_bounds=(2.0, 30.0))
    out = {'tool': 'mvt_fit_bench', 'device': torch.cuda.get_device_name(0), 'reps': args.reps,
           'launches_per_window': args.launches, 'shapes': [],
           'reference_record': 'Gradient_free_Student_t.ipynb prints Wall time: 3min 51s, nfev: 4928, njev: 308 for '
                               'fit_mvt on one chain of 5e5 rows at d = 4 (its own machine; quoted, not measured here)'}
    for spec in args.shapes.split(','):
        n, d = (int(v) for v in spec.split(':'))
        x, loc, sigma, df = t_case(n, d, 100 * d + 7)
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)   # noqa: E731
        xd = to(x)
        lik = proxy.StudentTLikelihood(xd)
        a_up = np.linalg.cholesky(sigma).T
        u = np.triu(np.linalg.inv(a_up))
        par = np.concatenate([loc, a_up[np.triu_indices(d)], [df]])
        lik.nll_and_grad(par)                       # device state, warm
        st = lik._device
        ld, ud = to(loc), to(u)
        stream = nat.stream_handle()

        def run_moments(want_grad):
            nat.check(lib.st_mvt_moments(nat.ptr(xd), n, d, nat.ptr(ld), nat.ptr(ud), df, want_grad, nat.ptr(st['out']),
                                         nat.ptr(st['ws']), st['ws'].numel() * 8, stream), 'st_mvt_moments')

        psd = proxy._psd(sigma, allow_singular=True)
        pd = to(np.linalg.inv(sigma))
        pu = to(psd.U)
        c_log = float(gammaln(0.5 * (df + d)) - gammaln(0.5 * df) - d / 2. * np.log(df * np.pi) - 0.5 * psd.log_pdet)
        log_q = torch.empty(n, dtype=torch.float64, device=dev)
        grad = torch.empty((n, d), dtype=torch.float64, device=dev)

        def run_proxy():
            nat.check(lib.st_proxy_logpdf_grad(nat.ptr(xd), n, d, nat.ptr(ld), nat.ptr(pu), nat.ptr(pd), df, c_log,
                                               nat.ptr(log_q), nat.ptr(grad), stream), 'st_proxy_logpdf_grad')

        def run_proxy_sum():
            run_proxy()
            torch.sum(log_q)

        legs = {'value_s': lambda: run_moments(0), 'value_grad_s': lambda: run_moments(1), 'proxy_s': run_proxy,
                'proxy_sum_s': run_proxy_sum}
        for fn in legs.values():            # warm-up of this shape
            window(fn, 3)
        times = {name: [] for name in legs}
        for _ in range(args.reps):          # alternating
            for name, fn in legs.items():
                times[name].append(window(fn, args.launches))
        rec = {'n': n, 'd': d}
        for name, v in times.items():
            rec[name] = statistics.median(v)
            rec[name + '_min'], rec[name + '_max'] = min(v), max(v)
        rec['bytes'] = 8.0 * n * d
        rec['value_bytes_s'] = rec['bytes'] / rec['value_s']
        rec['value_grad_bytes_s'] = rec['bytes'] / rec['value_grad_s']
        rec['proxy_bytes_s'] = 8.0 * n * (2 * d + 1) / rec['proxy_s']
        rec['proxy_sum_over_value'] = rec['proxy_sum_s'] / rec['value_s']
        rec['proxy_sum_over_value_grad'] = rec['proxy_sum_s'] / rec['value_grad_s']

        # the sums of the timed launches against the proxy launch's log q (the same rows, the same parameters)
        run_moments(1)
        run_proxy()
        torch.cuda.synchronize()
        s0 = float(st['out'][0].cpu())
        total_log_q = float(torch.sum(log_q).cpu())
        mine = n * c_log - 0.5 * (df + d) * s0
        rec['rel_diff_sum_log_q'] = abs(mine - total_log_q) / abs(total_log_q)

        def call():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            lik.nll_and_grad(par)           # returns host numbers: the copy back synchronises
            return time.perf_counter() - t0
        call()
        rec['nll_and_grad_call_s'] = statistics.median([call() for _ in range(args.call_reps)])

        def fit(rows):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = proxy.fit_mvt(rows, **bounds)
            return time.perf_counter() - t0, res
        fit(lik)
        fits = [fit(lik) for _ in range(args.fit_reps)]
        rec['fit_s'] = statistics.median([t for t, _ in fits])
        res = fits[0][1]
        rec['fit_nfev'], rec['fit_nit'], rec['fit_success'], rec['fit_df'] = int(res.nfev), int(res.nit), bool(res.success), float(res.x[-1])
        rec['fit_fun'] = float(res.fun)
        rec['fit_s_over_nfev_calls'] = rec['fit_s'] / (rec['fit_nfev'] * rec['nll_and_grad_call_s'])
        rec['fit_upload_s'] = statistics.median([fit(x)[0] for _ in range(args.fit_reps)])

        rows = min(args.host_rows, n)
        mu_f, scale_f, df_f = proxy.extract_t_params(res.x, d)
        t0 = time.perf_counter()
        host = -np.sum(stats.multivariate_t.logpdf(x[:rows], loc=mu_f, shape=scale_f, df=df_f))
        t_host = time.perf_counter() - t0
        sub = proxy.StudentTLikelihood(xd[:rows])
        rec['host_rows'] = rows
        rec['rel_diff_objective_subset'] = abs(sub.nll(res.x) - host) / abs(host)
        rec['objective_host_subset_s'] = t_host
        rec['objective_host_s_extrapolated'] = t_host * n / rows
        rec['objective_host_extrapolated_over_call'] = rec['objective_host_s_extrapolated'] / rec['nll_and_grad_call_s']
        out['shapes'].append(rec)
        del xd, log_q, grad, lik, sub
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
