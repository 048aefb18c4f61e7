"""HMC with a dense metric and step-size adaptation (st_lv_hmc_metric_wave, csrc/lv_mcmc.hip): timings against
st_lv_hmc_wave and the reference-shaped adapted run; one JSON line, also written to --out; needs a GPU.

(a) Per chain count (default 5, 64, 1024, 4096), from starts log(THETA) + 0.02 N(0, I), trajectories of --leapfrog (4)
stages, kick cap --cap (0.5), supplied noise, --evals (64) leapfrog stages in all as launches of
lotka_volterra.STEPS_PER_LAUNCH_HMC(L) steps:
  * hmc_s           -- st_lv_hmc_wave at step size --eps (0.001): the yardstick, whose text is the parent's;
  * metric_id_s     -- st_lv_hmc_metric_wave, identity metric, the same eps for every chain, adapt 0 (the same rows);
  * metric_adapt_s  -- st_lv_hmc_metric_wave, a dense metric (--dense-scale times a fixed lower-triangular factor with
                       every entry non-zero), eps = --eps / --dense-scale, adapt 1 from a fresh dual-averaging state.
Every window is the whole run between two device events with a synchronise on the second, after a warm-up of every
leg; the legs alternate in one process and the figure is the median of --reps windows with [min, max].  ms_per_eval =
time / (gradient evaluations, the start row's included).  <leg>_over_hmc is the ratio of the medians;
<leg>_slowdown_beyond_hmc_spread is how far the leg's median lies above the yardstick's slowest window, relative to the
yardstick's median (0 when it does not).
(b) --reference-run: lotka_volterra.hmc_warmup from log(THETA_INITS), 5 chains, --warmup (1000) steps from --eps, then
hmc_metric_sample for --draws (10 000) rows with the adapted step size and metric, L = --leapfrog, --cap, max_steps
10 000; ONE timed run; convergence.summary of the draws, next to the unadapted run's recorded figures."""
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

DENSE = [[1.0, 0.0, 0.0, 0.0], [0.3, 0.9, 0.0, 0.0], [-0.2, 0.25, 1.1, 0.0], [0.15, -0.35, 0.2, 0.8]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--chains', default='5,64,1024,4096')
    ap.add_argument('--leapfrog', type=int, default=4)
    ap.add_argument('--evals', type=int, default=64, help='leapfrog stages per timed window')
    ap.add_argument('--reps', type=int, default=3, help='timed windows per leg')
    ap.add_argument('--eps', type=float, default=0.001)
    ap.add_argument('--cap', type=float, default=0.5)
    ap.add_argument('--dense-scale', type=float, default=0.02)
    ap.add_argument('--target-accept', type=float, default=0.8)
    ap.add_argument('--reference-run', action='store_true')
    ap.add_argument('--warmup', type=int, default=1000)
    ap.add_argument('--draws', type=int, default=10_000)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lv_hmc_adapt_bench.json'))
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit('lv_hmc_adapt_bench needs a HIP device: timings on a CPU say nothing about the GPU')
    from stein_thinning import _native as nat
    from stein_thinning import convergence
    from stein_thinning import lotka_volterra as lv
    dev = nat.require_device()
    L = nat.lib()
    stream = nat.stream_handle()
    data = lv.reference_data()
    t, y, s = lv._settings(data, lv.RTOL, lv.ATOL)
    U, c_log, norm_logc = lv._density_constants(data)
    cinv = np.ascontiguousarray(np.linalg.inv(np.asarray(data.cov, dtype=np.float64)))
    td, yd = (torch.from_numpy(a).to(dev) for a in (t, y))
    n_leapfrog, evals = args.leapfrog, args.evals
    steps = max(1, evals // n_leapfrog)
    spl = lv.STEPS_PER_LAUNCH_HMC(n_leapfrog)
    eps4 = np.full(4, args.eps)
    kick = np.full(4, args.cap)
    tril = np.tril_indices(4)

    def window(fn):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) * 1e-3

    out = {'tool': 'lv_hmc_adapt_bench', 'device': torch.cuda.get_device_name(0), 'reps': args.reps, 'evals': evals,
           'n_leapfrog': n_leapfrog, 'steps': steps, 'eps': args.eps, 'kick_cap': args.cap,
           'dense_scale': args.dense_scale, 'target_accept': args.target_accept, 't_n': int(t.size), 'shapes': []}
    for chains in (int(v) for v in args.chains.split(',') if v):
        rng = np.random.default_rng(chains)
        x0 = torch.from_numpy(np.log(lv.THETA) + 0.02 * rng.normal(size=(chains, 4))).to(dev)
        gen = torch.Generator(device=dev).manual_seed(chains)
        z = torch.randn((chains, steps, 4), dtype=torch.float64, device=dev, generator=gen)
        log_u = torch.rand((chains, steps), dtype=torch.float64, device=dev, generator=gen).log()
        res = {}

        def leg(name, metric, adapt):
            """metric None: st_lv_hmc_wave; else st_lv_hmc_metric_wave with that (4, 4) factor for every chain"""
            words = 16 if metric is None else 24
            state = torch.zeros((chains, words), dtype=torch.float64, device=dev)
            samples = torch.empty((chains, steps + 1, 4), dtype=torch.float64, device=dev)
            grad = torch.empty((chains, steps + 1, 4), dtype=torch.float64, device=dev)
            log_p, alpha, used = (torch.empty((chains, steps + 1), dtype=torch.float64, device=dev) for _ in range(3))
            res[name] = (samples, state)
            if metric is not None:
                e = args.eps if not adapt else args.eps / args.dense_scale
                eps_d = torch.full((chains,), e, dtype=torch.float64, device=dev)
                chol_d = torch.from_numpy(np.tile(np.asarray(metric)[tril], (chains, 1))).to(dev)
                da0 = torch.from_numpy(lv.hmc_adapt_restart(np.full(chains, e))).to(dev)

            def run():
                state.zero_()
                state[:, :4] = x0
                if metric is not None:
                    state[:, 16:21] = da0
                for k0 in range(0, steps, spl):
                    k = min(spl, steps - k0)
                    head = (nat.ptr(state), chains, 0, k0 + 1, k, 1 if k0 == 0 else 0)
                    mid = (0, 1, nat.ptr(z), nat.ptr(log_u), steps, k0, nat.ptr(td), t.size, nat.ptr(yd),
                           s.ctypes.data, U.ctypes.data, c_log, norm_logc, cinv.ctypes.data, lv.MAX_STEPS,
                           nat.ptr(samples), nat.ptr(log_p), nat.ptr(grad))
                    tail = (steps + 1, k0 + 1, stream)
                    if metric is None:
                        nat.check(L.st_lv_hmc_wave(*head, eps4.ctypes.data, kick.ctypes.data, n_leapfrog, *mid, *tail),
                                  'st_lv_hmc_wave')
                    else:
                        nat.check(L.st_lv_hmc_metric_wave(*head, nat.ptr(eps_d), nat.ptr(chol_d), kick.ctypes.data,
                                                          n_leapfrog, 1 if adapt else 0, args.target_accept, *mid,
                                                          nat.ptr(alpha), nat.ptr(used), *tail), 'st_lv_hmc_metric_wave')
            return run

        legs = {'hmc_s': leg('hmc_s', None, False), 'metric_id_s': leg('metric_id_s', np.eye(4), False),
                'metric_adapt_s': leg('metric_adapt_s', args.dense_scale * np.array(DENSE), True)}
        for fn in legs.values():
            window(fn)
        times = {name: [] for name in legs}
        for _ in range(args.reps):
            for name, fn in legs.items():
                times[name].append(window(fn))
        torch.cuda.synchronize()
        n_evals = steps * n_leapfrog + 1
        rec = {'chains': chains, 'evals': n_evals}
        for name, v in times.items():
            key = name[:-2]
            rec[name] = statistics.median(v)
            rec[key + '_min_s'], rec[key + '_max_s'] = min(v), max(v)
            rec[key + '_ms_per_eval'] = rec[name] / n_evals * 1e3
            moved = (res[name][0][:, 1:] != res[name][0][:, :-1]).any(dim=2)
            rec[key + '_acceptance'] = float(moved.double().mean())
            rec[key + '_n_failed'] = int(res[name][1].view(torch.int64)[:, 6].sum())
        rec['metric_id_rows_equal_hmc'] = bool(torch.equal(res['metric_id_s'][0], res['hmc_s'][0]))
        for key in ('metric_id', 'metric_adapt'):
            rec[key + '_over_hmc'] = rec[key + '_s'] / rec['hmc_s']
            rec[key + '_slowdown_beyond_hmc_spread'] = max(0.0, rec[key + '_s'] - rec['hmc_max_s']) / rec['hmc_s']
        out['shapes'].append(rec)
        print(json.dumps(rec), file=sys.stderr, flush=True)
        del res, legs, z, log_u

    if args.reference_run:
        x0 = np.log(lv.THETA_INITS)
        kw = dict(kick_cap=args.cap, data=data, max_steps=10_000, device_out=True)
        lv.hmc_metric_sample(x0, 2, args.eps, np.eye(4), n_leapfrog, seed=1, **kw)          # warm-up: 1 step
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ad = lv.hmc_warmup(x0, args.warmup, args.eps, n_leapfrog, target_accept=args.target_accept, seed=1, **kw)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        run = lv.hmc_metric_sample(ad.last_row.cpu().numpy(), args.draws, ad.step_size, ad.metric_chol, n_leapfrog, seed=2, **kw)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        sm = convergence.summary(run.samples)
        ess = np.asarray(sm.ess_bulk, dtype=np.float64)
        ref = {'chains': 5, 'warmup': args.warmup, 'rows': args.draws, 'n_leapfrog': n_leapfrog, 'eps_start': args.eps,
               'kick_cap': args.cap, 'max_steps': 10_000, 'target_accept': args.target_accept,
               'warmup_s': t1 - t0, 'draws_s': t2 - t1, 'run_s': t2 - t0,
               'windows': [[w.start, w.stop] for w in ad.windows],
               'window_step_sizes': [np.asarray(w.step_size).tolist() for w in ad.windows],
               'step_size': np.asarray(ad.step_size).tolist(), 'metric_chol': np.asarray(ad.metric_chol).tolist(),
               'warmup_n_failed': ad.n_failed.tolist(), 'n_failed_per_chain': run.n_failed.tolist(),
               'acceptance_per_chain': (run.accepted.double() / (args.draws - 1)).tolist(),
               'mean_accept_stat_per_chain': run.accept_stat.mean(dim=1).tolist(),
               'log_p_last_row': run.log_p[:, -1].tolist(),
               'mean': np.asarray(sm.mean).tolist(), 'sd': np.asarray(sm.sd).tolist(),
               'ess_bulk': ess.tolist(), 'ess_tail': np.asarray(sm.ess_tail).tolist(),
               'r_hat': np.asarray(sm.r_hat).tolist(),
               'ess_bulk_per_s_of_run': (ess / (t2 - t0)).tolist(), 'ess_bulk_per_s_of_draws': (ess / (t2 - t1)).tolist(),
               'r_hat_below_1_01': bool(np.all(np.asarray(sm.r_hat) <= 1.01)),
               'unadapted_recorded': 'profiles/convergence_bench.json: ess_bulk 57-99, r_hat 1.04-1.06 '
                                     '(5 x 10 000 rows, eps 0.001, L 4)',
               'stan_notebook': 'ESS 2700-4100 from the same number of draws'}
        out['reference_run'] = ref
        print(json.dumps(ref), file=sys.stderr, flush=True)

    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
