"""Gaussian-mixture log density + score timings (one JSON line, also written to --out; needs a GPU).

Shapes n:d:k = 2e6:4:2, 2e6:4:8 and 5e5:50:4 on the seeded mixture recipe below.  Per shape:
  * kernel_s     -- st_mixture_logpdf_score alone on device-resident rows and parameters;
  * k_gaussian_s -- the yardstick on the device: k back-to-back st_proxy_logpdf_grad (Gaussian) launches on
                    the same rows, one per component -- the existing code doing the same per-component
                    product, with k times the memory traffic and no mixing;
  * e2e_s        -- mixture_logpdf_score(host array) -> host arrays: factors, upload, kernel, download;
  * oracle_s_extrapolated -- the NumPy oracle's logpdf + score (oracle.models.make_mvn_mixture: the
                    reference's sums of densities and its four-operand einsum) on one host core, timed on
                    --oracle-rows rows and scaled by n / rows (labelled: extrapolated, not measured at n).
The two device legs alternate in one process after a warm-up; each window is --launches back-to-back
launches between two device events (a single launch is tens of microseconds: one launch per window
would time the clock), the per-launch time is the window over its launches, and the figure is the
median of --reps windows.  bytes_s / flop_s are the algorithm's counts from the shapes over kernel_s.
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


def mixture_case(n, d, k, seed):
    """Seeded mixture and rows: means 2 N(0, 1), cov_c = A A^T / d + 0.3 I, w ~ Dirichlet(2), every row
    from a component drawn with probabilities w, spread x 1.5."""
    import numpy as np
    rng = np.random.default_rng(seed)
    a = rng.normal(size=(k, d, d))
    covs = a @ a.transpose(0, 2, 1) / d + 0.3 * np.eye(d)
    means = 2.0 * rng.normal(size=(k, d))
    w = rng.dirichlet(np.full(k, 2.0))
    comp = rng.choice(k, size=n, p=w)
    chol = np.linalg.cholesky(covs)
    x = np.empty((n, d))
    for c in range(k):
        sel = comp == c
        x[sel] = means[c] + 1.5 * rng.normal(size=(int(sel.sum()), d)) @ chol[c].T
    return x, w, means, covs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='2000000:4:2,2000000:4:8,500000:50:4', help='n:d:k,...')
    ap.add_argument('--reps', type=int, default=20, help='timed windows per device leg (>= 5)')
    ap.add_argument('--launches', type=int, default=50, help='launches per window')
    ap.add_argument('--e2e-reps', type=int, default=5)
    ap.add_argument('--oracle-rows', type=int, default=100000)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mixture_bench.json'))
    args = ap.parse_args()
    if args.reps < 5:
        ap.error('--reps must be >= 5')

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit('mixture_bench needs a HIP device: timings on a CPU say nothing about the GPU')
    from oracle import models
    from stein_thinning import _native as nat
    from stein_thinning import mixture, proxy
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

    out = {'tool': 'mixture_bench', 'device': torch.cuda.get_device_name(0), 'reps': args.reps,
           'launches_per_window': args.launches, 'shapes': []}
    for spec in args.shapes.split(','):
        n, d, k = (int(v) for v in spec.split(':'))
        x, w, means, covs = mixture_case(n, d, k, 100 * d + k)
        log_coef, mu, prec = mixture.mixture_factors(w, means, covs)
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)   # noqa: E731
        xd, cd, md, pd = to(x), to(log_coef), to(mu), to(prec)
        log_p = torch.empty(n, dtype=torch.float64, device=dev)
        score = torch.empty((n, d), dtype=torch.float64, device=dev)
        stream = nat.stream_handle()

        def run_mixture():
            nat.check(lib.st_mixture_logpdf_score(nat.ptr(xd), n, d, k, nat.ptr(cd), nat.ptr(md), nat.ptr(pd),
                                                  nat.ptr(log_p), nat.ptr(score), stream), 'st_mixture_logpdf_score')

        gauss = []   # per component: (loc, U, P, c_log) as gaussian_proxy prepares them
        for c in range(k):
            psd = proxy._psd(covs[c], allow_singular=False)
            gauss.append((to(means[c]), to(psd.U), to(np.linalg.inv(covs[c])),
                          float(psd.rank * proxy._LOG_2PI + psd.log_pdet)))
        log_q = torch.empty(n, dtype=torch.float64, device=dev)
        grad = torch.empty((n, d), dtype=torch.float64, device=dev)

        def run_gaussians():
            for loc, u, p, c_log in gauss:
                nat.check(lib.st_proxy_logpdf_grad(nat.ptr(xd), n, d, nat.ptr(loc), nat.ptr(u), nat.ptr(p), 0.0,
                                                   c_log, nat.ptr(log_q), nat.ptr(grad), stream),
                          'st_proxy_logpdf_grad')

        legs = {'kernel_s': run_mixture, 'k_gaussian_s': run_gaussians}
        for fn in legs.values():            # warm-up of this shape
            window(fn, 3)
        times = {name: [] for name in legs}
        for _ in range(args.reps):          # alternating
            for name, fn in legs.items():
                times[name].append(window(fn, args.launches))
        rec = {'n': n, 'd': d, 'k': k}
        for name, v in times.items():
            rec[name] = statistics.median(v)
            rec[name + '_min'], rec[name + '_max'] = min(v), max(v)
        rec['k_gaussian_over_kernel'] = rec['k_gaussian_s'] / rec['kernel_s']
        # the algorithm's traffic and arithmetic: x read once, log_p and score written once; per row and
        # component the product P_c dev (2 d^2), dev . y and the accumulation (4 d)
        nbytes = 8.0 * n * (2 * d + 1)
        flop = float(n) * k * (2 * d * d + 4 * d)
        rec['bytes'], rec['flop'] = nbytes, flop
        rec['bytes_s'], rec['flop_s'] = nbytes / rec['kernel_s'], flop / rec['kernel_s']

        def e2e():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            mixture.mixture_logpdf_score(x, w, means, covs)   # returns host arrays: the download synchronises
            return time.perf_counter() - t0
        e2e()
        rec['e2e_s'] = statistics.median([e2e() for _ in range(args.e2e_reps)])

        # outputs of the timed launches against the oracle on the subset it is timed on
        rows = min(args.oracle_rows, n)
        _, logpdf, score_fn = models.make_mvn_mixture(w, means, covs)
        try:
            from threadpoolctl import threadpool_limits
            one_core = threadpool_limits(limits=1)
            rec['oracle_threads'] = 1
        except ImportError:
            import contextlib
            one_core = contextlib.nullcontext()
            rec['oracle_threads'] = 'BLAS default (threadpoolctl missing); the einsum is single-threaded'
        with one_core:
            t0 = time.perf_counter()
            want_l = logpdf(x[:rows])
            want_s = score_fn(x[:rows])
            t_oracle = time.perf_counter() - t0
        rec['oracle_rows'] = rows
        rec['oracle_subset_s'] = t_oracle
        rec['oracle_s_extrapolated'] = t_oracle * n / rows
        rec['oracle_extrapolated_over_kernel'] = rec['oracle_s_extrapolated'] / rec['kernel_s']
        rec['oracle_extrapolated_over_e2e'] = rec['oracle_s_extrapolated'] / rec['e2e_s']
        run_mixture()
        torch.cuda.synchronize()
        got_l, got_s = log_p[:rows].cpu().numpy(), score[:rows].cpu().numpy()
        rec['max_rel_err_log_p'] = float(np.abs(got_l - want_l).max() / max(np.abs(want_l).max(), 1.0))
        rec['max_rel_err_score'] = float(np.abs(got_s - want_s).max() / max(np.abs(want_s).max(), 1.0))
        out['shapes'].append(rec)
        del xd, log_p, score, log_q, grad
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
