"""The no-U-turn sampler (st_lv_nuts_wave, csrc/lv_mcmc.hip): the cost of a stage against st_lv_hmc_metric_wave, the
longest launch, and the reference-shaped run next to the adapted L = 4 run; one JSON line, also written to --out; needs
a GPU.

(a) Per chain count (default 5, 64, 1024, 4096), from starts log(THETA) + 0.02 N(0, I), the dense metric --dense-scale
times a fixed lower-triangular factor, kick cap --cap, device noise, adapt 0, in one process:
  * metric_s   -- st_lv_hmc_metric_wave, L = 4, 16 steps in launches of STEPS_PER_LAUNCH_HMC(4): 64 stages + the start
                  row = 65 evaluations.  The yardstick: the parent commit's kernel, its text unchanged.
  * nuts_s     -- st_lv_nuts_wave, ONE step of max_depth 6 at the same step size --straight-eps, small enough that no
                  sub-tree turns: every chain runs 63 stages (checked from the n_leapfrog output) + the start row = 64
                  evaluations at points as close to the start as the yardstick's.
  * nuts_mixed_s -- st_lv_nuts_wave, --mixed-steps steps of max_depth 6 at --mixed-eps: trees of every size; reported
                  with the stage counts (the launch waits for the chain with the most stages).
Every window is the whole run between two device events; the legs alternate after a warm-up of each and the figure is
the median of --reps windows with [min, max].  ms_per_eval = time / evaluations; nuts_over_metric is the ratio of the
two ms_per_eval and metric_spread the yardstick's (max - min) / median, the margin the ratio is read against.
  * depth10_s  -- one NUTS step of max_depth 10 at --straight-eps: 1023 stages, the longest launch nuts_sample makes
                  (STEPS_PER_LAUNCH_NUTS(10) = 1); one window per chain count.
(b) --reference-run: nuts_warmup from log(THETA_INITS), 5 chains, --warmup (1000) steps from --eps, then nuts_sample
for --draws (10 000) rows, max_depth 10, --cap, max_steps 10 000: ONE timed run; then hmc_warmup + hmc_metric_sample
with L = 4 in the same way in the same process; convergence.summary of both."""
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
    ap.add_argument('--reps', type=int, default=3, help='timed windows per leg')
    ap.add_argument('--straight-eps', type=float, default=1e-4)
    ap.add_argument('--mixed-eps', type=float, default=0.05)
    ap.add_argument('--mixed-steps', type=int, default=4)
    ap.add_argument('--eps', type=float, default=0.001, help='the reference-shaped run\'s first step size')
    ap.add_argument('--cap', type=float, default=0.5)
    ap.add_argument('--dense-scale', type=float, default=0.02)
    ap.add_argument('--target-accept', type=float, default=0.8)
    ap.add_argument('--reference-run', action='store_true')
    ap.add_argument('--warmup', type=int, default=1000)
    ap.add_argument('--draws', type=int, default=10_000)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lv_nuts_bench.json'))
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit('lv_nuts_bench needs a HIP device: timings on a CPU say nothing about the GPU')
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
    kick = np.full(4, args.cap)
    tril = np.tril_indices(4)
    metric = args.dense_scale * np.array(DENSE)

    def window(fn):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) * 1e-3

    out = {'tool': 'lv_nuts_bench', 'device': torch.cuda.get_device_name(0), 'reps': args.reps,
           'straight_eps': args.straight_eps, 'mixed_eps': args.mixed_eps, 'mixed_steps': args.mixed_steps,
           'kick_cap': args.cap, 'dense_scale': args.dense_scale, 't_n': int(t.size), 'shapes': []}
    for chains in (int(v) for v in args.chains.split(',') if v):
        rng = np.random.default_rng(chains)
        x0 = torch.from_numpy(np.log(lv.THETA) + 0.02 * rng.normal(size=(chains, 4))).to(dev)
        chol_d = torch.from_numpy(np.tile(metric[tril], (chains, 1))).to(dev)
        res = {}

        def leg(name, eps, steps, spl, n_leapfrog=None, max_depth=None):
            """n_leapfrog: st_lv_hmc_metric_wave; max_depth: st_lv_nuts_wave"""
            state = torch.zeros((chains, 24), dtype=torch.float64, device=dev)
            samples = torch.empty((chains, steps + 1, 4), dtype=torch.float64, device=dev)
            grad = torch.empty((chains, steps + 1, 4), dtype=torch.float64, device=dev)
            log_p, alpha, used, depth, stages, div = (torch.zeros((chains, steps + 1), dtype=torch.float64, device=dev)
                                                      for _ in range(6))
            eps_d = torch.full((chains,), eps, dtype=torch.float64, device=dev)
            res[name] = (state, stages, div, depth)

            def run():
                state.zero_()
                state[:, :4] = x0
                for k0 in range(0, steps, spl):
                    k = min(spl, steps - k0)
                    head = (nat.ptr(state), chains, 0, k0 + 1, k, 1 if k0 == 0 else 0, nat.ptr(eps_d), nat.ptr(chol_d),
                            kick.ctypes.data)
                    mid = (0, args.target_accept, 1, 7, None, None, 0, 0, nat.ptr(td), t.size, nat.ptr(yd),
                           s.ctypes.data, U.ctypes.data, c_log, norm_logc, cinv.ctypes.data, lv.MAX_STEPS,
                           nat.ptr(samples), nat.ptr(log_p), nat.ptr(grad), nat.ptr(alpha), nat.ptr(used))
                    tail = (steps + 1, k0 + 1, stream)
                    if max_depth is None:
                        nat.check(L.st_lv_hmc_metric_wave(*head, n_leapfrog, *mid, *tail), 'st_lv_hmc_metric_wave')
                    else:
                        nat.check(L.st_lv_nuts_wave(*head, max_depth, *mid, nat.ptr(depth), nat.ptr(stages),
                                                    nat.ptr(div), *tail), 'st_lv_nuts_wave')
            return run

        legs = {'metric_s': leg('metric_s', args.straight_eps, 16, lv.STEPS_PER_LAUNCH_HMC(4), n_leapfrog=4),
                'nuts_s': leg('nuts_s', args.straight_eps, 1, 1, max_depth=6),
                'nuts_mixed_s': leg('nuts_mixed_s', args.mixed_eps, args.mixed_steps, lv.STEPS_PER_LAUNCH_NUTS(6),
                                    max_depth=6)}
        for fn in legs.values():
            window(fn)
        times = {name: [] for name in legs}
        for _ in range(args.reps):
            for name, fn in legs.items():
                times[name].append(window(fn))
        deep = leg('depth10_s', args.straight_eps, 1, 1, max_depth=10)
        times['depth10_s'] = [window(deep)]
        torch.cuda.synchronize()
        rec = {'chains': chains}
        for name, v in times.items():
            key = name[:-2]
            rec[name] = statistics.median(v)
            rec[key + '_min_s'], rec[key + '_max_s'] = min(v), max(v)
            rec[key + '_n_failed'] = int(res[name][0].view(torch.int64)[:, 6].sum())
            if key != 'metric':
                per_chain = res[name][1][:, 1:].sum(dim=1)
                rec[key + '_stages_per_chain_min'] = int(per_chain.min())
                rec[key + '_stages_per_chain_max'] = int(per_chain.max())
                rec[key + '_stages_per_chain_mean'] = float(per_chain.mean())
                rec[key + '_divergent'] = int(res[name][2][:, 1:].sum())
        rec['metric_evals'] = 65
        rec['metric_ms_per_eval'] = rec['metric_s'] / 65 * 1e3
        rec['nuts_all_chains_63_stages'] = rec['nuts_stages_per_chain_min'] == rec['nuts_stages_per_chain_max'] == 63
        rec['nuts_evals'] = rec['nuts_stages_per_chain_max'] + 1
        rec['nuts_ms_per_eval'] = rec['nuts_s'] / rec['nuts_evals'] * 1e3
        rec['nuts_over_metric'] = rec['nuts_ms_per_eval'] / rec['metric_ms_per_eval']
        rec['metric_spread'] = (rec['metric_max_s'] - rec['metric_min_s']) / rec['metric_s']
        rec['nuts_mixed_ms_per_slowest_chains_eval'] = rec['nuts_mixed_s'] / (rec['nuts_mixed_stages_per_chain_max'] + 1) * 1e3
        rec['depth10_ms_per_eval'] = rec['depth10_s'] / (rec['depth10_stages_per_chain_max'] + 1) * 1e3
        out['shapes'].append(rec)
        print(json.dumps(rec), file=sys.stderr, flush=True)
        del res, legs

    if args.reference_run:
        x0 = np.log(lv.THETA_INITS)
        kw = dict(kick_cap=args.cap, data=data, max_steps=10_000, device_out=True)

        def summary(ad, run, t0, t1, t2):
            sm = convergence.summary(run.samples)
            ess = np.asarray(sm.ess_bulk, dtype=np.float64)
            return {'warmup_s': t1 - t0, 'draws_s': t2 - t1, 'run_s': t2 - t0,
                    'step_size': np.asarray(ad.step_size).tolist(),
                    'warmup_n_failed': ad.n_failed.tolist(), 'n_failed_per_chain': run.n_failed.tolist(),
                    'accepted_share_per_chain': (run.accepted.double() / (args.draws - 1)).tolist(),
                    'mean_accept_stat_per_chain': run.accept_stat.mean(dim=1).tolist(),
                    'log_p_last_row': run.log_p[:, -1].tolist(),
                    'mean': np.asarray(sm.mean).tolist(), 'sd': np.asarray(sm.sd).tolist(),
                    'ess_bulk': ess.tolist(), 'ess_tail': np.asarray(sm.ess_tail).tolist(),
                    'r_hat': np.asarray(sm.r_hat).tolist(),
                    'ess_bulk_per_s_of_run': (ess / (t2 - t0)).tolist(),
                    'ess_bulk_per_s_of_draws': (ess / (t2 - t1)).tolist()}

        lv.nuts_sample(x0, 2, args.eps, max_depth=1, seed=1, **kw)                              # loads the kernel
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ad = lv.nuts_warmup(x0, args.warmup, args.eps, target_accept=args.target_accept, seed=1, **kw)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        run = lv.nuts_sample(ad.last_row.cpu().numpy(), args.draws, ad.step_size, ad.metric_chol, seed=2, **kw)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        nuts = summary(ad, run, t0, t1, t2)
        nuts.update({'max_depth': 10,
                     'tree_depth_histogram': torch.bincount(run.tree_depth.flatten().long(), minlength=11).tolist(),
                     'divergent': int(run.divergent.sum()), 'stages': int(run.n_leapfrog.sum()),
                     'stages_per_chain': run.n_leapfrog.sum(dim=1).tolist(),
                     'mean_stages_per_step': float(run.n_leapfrog.double().mean()),
                     'max_stages_in_a_step': int(run.n_leapfrog.max()),
                     'draws_ms_per_slowest_chains_stage':
                         (t2 - t1) / float(run.n_leapfrog.max(dim=0).values.sum()) * 1e3,
                     'warmup_stages_per_chain': 'not recorded (HmcAdaptation carries no n_leapfrog)',
                     'metric_chol': np.asarray(ad.metric_chol).tolist()})
        print(json.dumps(nuts), file=sys.stderr, flush=True)
        lv.hmc_metric_sample(x0, 2, args.eps, np.eye(4), 4, seed=1, **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ad = lv.hmc_warmup(x0, args.warmup, args.eps, 4, target_accept=args.target_accept, seed=1, **kw)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        run = lv.hmc_metric_sample(ad.last_row.cpu().numpy(), args.draws, ad.step_size, ad.metric_chol, 4, seed=2, **kw)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        hmc = summary(ad, run, t0, t1, t2)
        hmc['n_leapfrog'] = 4
        print(json.dumps(hmc), file=sys.stderr, flush=True)
        out['reference_run'] = {'chains': 5, 'warmup': args.warmup, 'rows': args.draws, 'eps_start': args.eps,
                                'kick_cap': args.cap, 'max_steps': 10_000, 'target_accept': args.target_accept,
                                'nuts': nuts, 'hmc_l4': hmc,
                                'stan_notebook': 'ESS 2700-4100 from the same number of draws (quoted, not measured)'}

    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
