"""Convergence-diagnostics timings (stein_thinning.convergence, csrc/convergence.hip); one JSON line, also written to
--out; needs a GPU.

Shapes, all device-resident float64 (C, n, 4) tensors of synthetic AR(1) chains (unit innovations):
  * ref_long   -- 5 x 500 000, phi = 0.9999: the reference's random-walk run, which has not converged, so Geyer's
                  truncation lag approaches the series length;
  * ref_short  -- 5 x 10 000, phi = 0.5: a well-mixed gradient-sampler run;
  * starts     -- 65 536 x 256, phi = 0.5: the randomised-starts shape of thin_many (--no-starts leaves it out).
Per shape: ``summary`` once to warm up, then --reps timed calls (median, [min, max]) and one call with the per-stage
split (sort, rank kernel, autocovariance calls with their downloads, host Geyer; each stage closed by a device
synchronisation, so the stages add up to more than the untimed call).  Yardsticks in the same process, for the raw
split chains only (one of the five quantities ``summary`` takes autocovariances of):
  * fft_s      -- every lag of every split chain with torch.fft (zero-padded rfft, |.|^2, irfft) on the device;
  * autocov_all_lags_s -- st_autocov for every lag of the same chains in one call (what the FFT computes);
  * numpy_s    -- the direct float64 sum in NumPy on one host core, timed on ONE series and --numpy-lags lags and
                  EXTRAPOLATED linearly to all series and lags.
--samplers: ess_bulk, ess_tail and r_hat of the reference-shaped mala_sample and hmc_sample runs of the README
(5 chains x 10 000 rows from THETA_INITS), with the run's time and bulk ESS per second."""
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


def ar1(C, n, d, phi, seed):
    import numpy as np
    from scipy.signal import lfilter
    e = np.random.default_rng(seed).standard_normal((C, n, d))
    return lfilter([1.0], [1.0, -phi], e, axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--numpy-lags', type=int, default=64)
    ap.add_argument('--no-starts', action='store_true')
    ap.add_argument('--no-long', action='store_true')
    ap.add_argument('--samplers', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'convergence_bench.json'))
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit('convergence_bench needs a HIP device: timings on a CPU say nothing about the GPU')
    from stein_thinning import _native as nat
    from stein_thinning import convergence as conv
    dev = nat.require_device()

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t, r

    shapes = [('ref_short', 5, 10_000, 0.5)]
    if not args.no_long:
        shapes.append(('ref_long', 5, 500_000, 0.9999))
    if not args.no_starts:
        shapes.append(('starts', 65_536, 256, 0.5))
    out = {'tool': 'convergence_bench', 'device': torch.cuda.get_device_name(0), 'reps': args.reps,
           'first_lags': conv.FIRST_LAGS, 'shapes': []}
    for name, C, n, phi in shapes:
        x = torch.from_numpy(ar1(C, n, 4, phi, 7)).to(dev)
        timed(lambda: conv.summary(x))
        ts, s = [], None
        for _ in range(args.reps):
            t, s = timed(lambda: conv.summary(x))
            ts.append(t)
        st = conv._Stages(True)
        t_staged, _ = timed(lambda: conv.summary(x, _stages=st))
        rec = {'shape': name, 'chains': C, 'rows': n, 'd': 4, 'phi': phi, 'summary_s': statistics.median(ts),
               'summary_min_s': min(ts), 'summary_max_s': max(ts), 'staged_total_s': t_staged,
               'stages_s': st.seconds, 'ess_bulk': s.ess_bulk.tolist(), 'ess_tail': s.ess_tail.tolist(),
               'r_hat': s.r_hat.tolist()}
        # yardsticks on the raw split chains
        sp = conv._split(conv._as_chains(x))
        G, S, h = sp.shape
        nfft = 1 << (2 * h - 1).bit_length()

        def fft_all():
            c = sp - sp.mean(dim=2, keepdim=True)
            f = torch.fft.rfft(c, nfft, dim=2)
            return (torch.fft.irfft(f * f.conj(), nfft, dim=2)[:, :, :h] / h).mean(dim=1)

        def direct_all():
            got = []
            step = h
            L = nat.lib()
            while step > 64 and int(L.st_autocov_workspace_bytes(G, S, h, 0, step, 0)) > conv.MAX_WORKSPACE_BYTES:
                step //= 2
            for l0 in range(0, h, step):
                got.append(conv.autocov(sp, l0, min(h, l0 + step))[0])
            return torch.cat(got, dim=1)
        timed(fft_all)
        tf = [timed(fft_all)[0] for _ in range(args.reps)]
        timed(direct_all)
        td = [timed(direct_all) for _ in range(args.reps)]
        rec['fft_s'] = statistics.median(tf)
        rec['autocov_all_lags_s'] = statistics.median(t for t, _ in td)
        rec['fma_per_s_all_lags'] = G * S * h * (h + 1) / 2 / rec['autocov_all_lags_s']
        one = sp[0, 0].cpu().numpy()
        lags = min(args.numpy_lags, h)
        t0 = time.perf_counter()
        c = one - one.mean()
        for t in range(lags):
            np.dot(c[:h - t], c[t:])
        t_np = time.perf_counter() - t0
        rec['numpy_one_series_s'] = t_np
        rec['numpy_lags_timed'] = lags
        rec['numpy_s'] = t_np * G * S * (h / lags)
        rec['numpy_s_is'] = 'extrapolated from one series and numpy_lags_timed lags, one host core'
        out['shapes'].append(rec)
        print(json.dumps(rec), file=sys.stderr, flush=True)
        del x, sp, td

    if args.samplers:
        from stein_thinning import lotka_volterra as lv
        data = lv.reference_data()
        x0 = np.log(lv.THETA_INITS)
        runs = {
            'mala': lambda rows: lv.mala_sample(x0, rows, 0.003, seed=1, drift_cap=1.0, data=data, max_steps=10_000,
                                                device_out=True),
            'hmc': lambda rows: lv.hmc_sample(x0, rows, 0.001, 4, seed=1, kick_cap=0.5, data=data, max_steps=10_000,
                                              device_out=True),
        }
        out['samplers'] = []
        for name, fn in runs.items():
            fn(2)
            t_run, r = timed(lambda: fn(10_000))
            timed(lambda: conv.summary(r.samples))
            t_sum, s = timed(lambda: conv.summary(r.samples))
            s2 = conv.summary(r.samples[:, 5000:].contiguous())
            rec = {'sampler': name, 'chains': 5, 'rows': 10_000, 'run_s': t_run, 'summary_s': t_sum,
                   'ess_bulk': s.ess_bulk.tolist(), 'ess_tail': s.ess_tail.tolist(), 'r_hat': s.r_hat.tolist(),
                   'mcse_mean': s.mcse_mean.tolist(), 'ess_bulk_per_s': (s.ess_bulk / t_run).tolist(),
                   'second_half': {'ess_bulk': s2.ess_bulk.tolist(), 'ess_tail': s2.ess_tail.tolist(),
                                   'r_hat': s2.r_hat.tolist()}}
            out['samplers'].append(rec)
            print(json.dumps(rec), file=sys.stderr, flush=True)
        out['stan_for_scale'] = 'Sampling.ipynb, Stan HMC: ESS 2700-4100 from 10 000 draws (quoted, not measured)'

    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
