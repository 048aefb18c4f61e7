"""HMC sampler timings (st_lv_hmc_wave, csrc/lv_mcmc.hip); one JSON line, also written to --out; needs a GPU.

Per chain count (default 5, 64, 1024, 4096) and trajectory length L (default 1, 4, 16), from starts
log(THETA) + 0.02 N(0, I) with step size --eps (0.001) and kick cap --cap (0.5), supplied noise, --evals (64)
leapfrog stages in all, i.e. max(1, evals // L) Metropolis steps, as launches of
lotka_volterra.STEPS_PER_LAUNCH_HMC(L) steps:
  * hmc_L<L>_s       -- st_lv_hmc_wave;
  * mala_s           -- st_lv_mala_wave on the same starts and noise, --evals steps (drift cap 1): the cost of one
                        gradient evaluation in the kernel HMC was built from;
  * yardstick_L<L>_s -- what a user could do before the sampler for the same chains: per stage one
                        st_lv_grad_log_posterior_ws launch plus one st_lv_log_target_density launch (2-state
                        integration) plus torch elementwise ops (kicks, clip, position update, exp, kinetic
                        energies, accept) on the same noise.
Every window is the whole run between two device events with a synchronise on the second, after a warm-up of every
leg; the legs alternate in one process and the figure is the median of --reps windows with [min, max].
ms_per_eval = time / (gradient evaluations, the start row's included).  hmc_over_mala_per_eval compares HMC's time
per gradient evaluation with MALA's time per step (one evaluation) of the same run; slowdown_beyond_mala_spread is
how far HMC's median lies above MALA's slowest window, relative to MALA's median (0 when it does not).
sweep: acceptance at 5 chains over --sweep-steps steps for every eps of --eps-sweep and every L (device noise),
over all steps and over the second half.
--reference-run: lotka_volterra.hmc_sample from log(THETA_INITS), 5 chains, --eps, --cap, L = --reference-l,
max_steps 10 000: first ONE launch of STEPS_PER_LAUNCH_HMC(L) steps is timed; the run of 10 000 rows follows, timed
once, only if that launch stays under 0.25 s.
Mixing (effective sample size) is not measured by this tool."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--chains', default='5,64,1024,4096')
    ap.add_argument('--leapfrog', default='1,4,16')
    ap.add_argument('--evals', type=int, default=64, help='leapfrog stages per timed window')
    ap.add_argument('--reps', type=int, default=3, help='timed windows per leg')
    ap.add_argument('--eps', type=float, default=0.001)
    ap.add_argument('--cap', type=float, default=0.5)
    ap.add_argument('--eps-sweep', default='0.0003,0.0005,0.001,0.0015,0.002')
    ap.add_argument('--sweep-steps', type=int, default=128)
    ap.add_argument('--reference-run', action='store_true')
    ap.add_argument('--reference-l', type=int, default=4)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lv_hmc_bench.json'))
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit('lv_hmc_bench needs a HIP device: timings on a CPU say nothing about the GPU')
    from stein_thinning import _native as nat
    from stein_thinning import lotka_volterra as lv
    dev = nat.require_device()
    L = nat.lib()
    stream = nat.stream_handle()
    data = lv.reference_data()
    t, y, s = lv._settings(data, lv.RTOL, lv.ATOL)
    U, c_log, norm_logc = lv._density_constants(data)
    cinv = np.ascontiguousarray(np.linalg.inv(np.asarray(data.cov, dtype=np.float64)))
    td, yd = (torch.from_numpy(a).to(dev) for a in (t, y))
    lengths = [int(v) for v in args.leapfrog.split(',')]
    evals = args.evals
    eps = np.full(4, args.eps)
    kick = np.full(4, args.cap)
    ehw = np.ascontiguousarray(np.concatenate([eps, 0.5 * eps * eps, 0.5 / (eps * eps)]))
    drift = np.ascontiguousarray(1.0 * eps)

    def window(fn):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) * 1e-3

    out = {'tool': 'lv_hmc_bench', 'device': torch.cuda.get_device_name(0), 'reps': args.reps, 'evals': evals,
           'eps': args.eps, 'kick_cap': args.cap, 'mala_drift_cap': 1.0, 't_n': int(t.size), 'shapes': []}
    for chains in (int(v) for v in args.chains.split(',')):
        rng = np.random.default_rng(chains)
        x0 = torch.from_numpy(np.log(lv.THETA) + 0.02 * rng.normal(size=(chains, 4))).to(dev)
        gen = torch.Generator(device=dev).manual_seed(chains)
        z = torch.randn((chains, evals, 4), dtype=torch.float64, device=dev, generator=gen)
        log_u = torch.rand((chains, evals), dtype=torch.float64, device=dev, generator=gen).log()
        res = {}

        def fused(name, n_leapfrog):
            """st_lv_hmc_wave (n_leapfrog >= 1) or st_lv_mala_wave (n_leapfrog = 0) over the same noise rows"""
            steps = evals if n_leapfrog == 0 else max(1, evals // n_leapfrog)
            spl = lv.STEPS_PER_LAUNCH_MALA if n_leapfrog == 0 else lv.STEPS_PER_LAUNCH_HMC(n_leapfrog)
            state = torch.zeros((chains, 16), dtype=torch.float64, device=dev)
            samples = torch.empty((chains, steps + 1, 4), dtype=torch.float64, device=dev)
            grad = torch.empty((chains, steps + 1, 4), dtype=torch.float64, device=dev)
            log_p = torch.empty((chains, steps + 1), dtype=torch.float64, device=dev)
            res[name] = (samples, state, steps)

            def run():
                state.zero_()
                state[:, :4] = x0
                for k0 in range(0, steps, spl):
                    k = min(spl, steps - k0)
                    head = (nat.ptr(state), chains, 0, k0 + 1, k, 1 if k0 == 0 else 0)
                    rest = (0, 1, nat.ptr(z), nat.ptr(log_u), evals, k0, nat.ptr(td), t.size, nat.ptr(yd),
                            s.ctypes.data, U.ctypes.data, c_log, norm_logc, cinv.ctypes.data, lv.MAX_STEPS,
                            nat.ptr(samples), nat.ptr(log_p), nat.ptr(grad), steps + 1, k0 + 1, stream)
                    if n_leapfrog == 0:
                        nat.check(L.st_lv_mala_wave(*head, ehw.ctypes.data, drift.ctypes.data, *rest), 'st_lv_mala_wave')
                    else:
                        nat.check(L.st_lv_hmc_wave(*head, eps.ctypes.data, kick.ctypes.data, n_leapfrog, *rest),
                                  'st_lv_hmc_wave')
            return run

        gout = torch.empty((chains, 4), dtype=torch.float64, device=dev)
        dout = torch.empty(chains, dtype=torch.float64, device=dev)
        status = torch.zeros(chains, dtype=torch.int32, device=dev)
        gwb = int(L.st_lv_grad_workspace_bytes(chains, t.size))
        dwb = int(L.st_lv_log_density_workspace_bytes(chains, t.size))
        gws = torch.empty((gwb + 7) // 8, dtype=torch.float64, device=dev)
        dws = torch.empty((dwb + 7) // 8, dtype=torch.float64, device=dev)

        def gradient(th):
            nat.check(L.st_lv_grad_log_posterior_ws(nat.ptr(th), chains, nat.ptr(td), t.size, nat.ptr(yd), s.ctypes.data,
                                                    cinv.ctypes.data, lv.MAX_STEPS, nat.ptr(gout), nat.ptr(status),
                                                    nat.ptr(gws), gwb, stream), 'st_lv_grad_log_posterior_ws')
            return gout

        def density(p, th):
            nat.check(L.st_lv_log_target_density(nat.ptr(p), nat.ptr(th), chains, nat.ptr(td), t.size, nat.ptr(yd),
                                                 s.ctypes.data, U.ctypes.data, c_log, norm_logc, lv.MAX_STEPS,
                                                 nat.ptr(dout), nat.ptr(status), nat.ptr(dws), dwb, stream),
                      'st_lv_log_target_density')
            return dout

        def yardstick(name, n_leapfrog):
            steps = max(1, evals // n_leapfrog)
            samples = torch.empty((chains, steps + 1, 4), dtype=torch.float64, device=dev)
            epsd, cd = torch.from_numpy(eps).to(dev), torch.from_numpy(kick).to(dev)
            res[name] = (samples, None, steps)

            def hk(g):
                return 0.5 * torch.minimum(torch.maximum(epsd * g, -cd), cd)

            def run():
                x = x0.clone()
                th = torch.exp(x)
                g = (th * gradient(th) - x).clone()
                lp = density(x, th).clone()
                samples[:, 0] = x
                for k in range(steps):
                    q, gq, r = x, g, z[:, k]
                    k0 = 0.5 * (r * r).sum(dim=1)
                    for _ in range(n_leapfrog):
                        rp = r + hk(gq)
                        q = (q + epsd * rp).contiguous()
                        th = torch.exp(q)
                        gq = th * gradient(th) - q
                        lq = density(q, th).clone()
                        r = rp + hk(gq)
                    acc = log_u[:, k] < (lq - lp) + (k0 - 0.5 * (r * r).sum(dim=1))
                    x = torch.where(acc[:, None], q, x)
                    g = torch.where(acc[:, None], gq, g)
                    lp = torch.where(acc, lq, lp)
                    samples[:, k + 1] = x
            return run

        legs = {'mala_s': fused('mala_s', 0)}
        for n in lengths:
            legs[f'hmc_L{n}_s'] = fused(f'hmc_L{n}_s', n)
            legs[f'yardstick_L{n}_s'] = yardstick(f'yardstick_L{n}_s', n)
        for fn in legs.values():
            window(fn)
        times = {name: [] for name in legs}
        for _ in range(args.reps):
            for name, fn in legs.items():
                times[name].append(window(fn))
        torch.cuda.synchronize()
        rec = {'chains': chains}
        for name, v in times.items():
            key = name[:-2]
            steps = res[name][2]
            n = 0 if name == 'mala_s' else int(name.split('_L')[1][:-2])
            n_evals = steps * max(n, 1) + 1
            rec[name] = statistics.median(v)
            rec[key + '_min_s'], rec[key + '_max_s'] = min(v), max(v)
            rec[key + '_steps'], rec[key + '_evals'] = steps, n_evals
            rec[key + '_ms_per_eval'] = rec[name] / n_evals * 1e3
            moved = (res[name][0][:, 1:] != res[name][0][:, :-1]).any(dim=2)
            rec[key + '_acceptance'] = float(moved.double().mean())
            if res[name][1] is not None:
                rec[key + '_n_failed'] = int(res[name][1].view(torch.int64)[:, 6].sum())
        mala_evals = rec['mala_evals']
        for n in lengths:
            key = f'hmc_L{n}'
            rec[key + '_launch_s'] = rec[key + '_s'] * min(lv.STEPS_PER_LAUNCH_HMC(n), rec[key + '_steps']) / rec[key + '_steps']
            rec[key + '_over_mala_per_eval'] = rec[key + '_ms_per_eval'] / rec['mala_ms_per_eval']
            slowest_mala = rec['mala_max_s'] / mala_evals * 1e3
            rec[key + '_slowdown_beyond_mala_spread'] = max(0.0, rec[key + '_ms_per_eval'] - slowest_mala) / rec['mala_ms_per_eval']
            rec[f'yardstick_over_hmc_L{n}'] = rec[f'yardstick_L{n}_s'] / rec[key + '_s']
        out['shapes'].append(rec)
        print(json.dumps(rec), file=sys.stderr, flush=True)
        del res, legs, z, log_u, gws, dws

    sweep = []
    steps = args.sweep_steps
    x5 = np.log(lv.THETA) + 0.02 * np.random.default_rng(5).normal(size=(5, 4))
    for e in (float(v) for v in args.eps_sweep.split(',') if v):
        for n in lengths:
            r = lv.hmc_sample(x5, steps + 1, e, n, seed=1, kick_cap=args.cap, data=data)
            moved = np.any(r.samples[:, 1:] != r.samples[:, :-1], axis=2)
            sweep.append({'eps': e, 'n_leapfrog': n, 'acceptance': float(moved.mean()),
                          'acceptance_second_half': float(moved[:, steps // 2:].mean()),
                          'per_chain': moved.mean(axis=1).tolist(), 'n_failed': int(r.n_failed.sum())})
        print(json.dumps(sweep[-len(lengths):]), file=sys.stderr, flush=True)
    out['sweep'] = {'chains': 5, 'steps': steps, 'kick_cap': args.cap, 'seed': 1, 'runs': sweep}
    out['mixing'] = 'not measured (no effective-sample-size tool)'

    if args.reference_run:
        n = args.reference_l
        spl = lv.STEPS_PER_LAUNCH_HMC(n)
        x0 = np.log(lv.THETA_INITS)
        kw = dict(seed=1, kick_cap=args.cap, data=data, max_steps=10_000, device_out=True)
        lv.hmc_sample(x0, 2, args.eps, n, **kw)                     # warm-up: 1 step
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = lv.hmc_sample(x0, spl + 1, args.eps, n, steps_per_launch=spl, **kw)
        torch.cuda.synchronize()
        ref = {'eps': args.eps, 'kick_cap': args.cap, 'n_leapfrog': n, 'max_steps': 10_000, 'launch_steps': spl,
               'launch_s': time.perf_counter() - t0, 'launch_n_failed': int(r.n_failed.sum())}
        print(json.dumps(ref), file=sys.stderr, flush=True)
        if ref['launch_s'] < 0.25:
            t0 = time.perf_counter()
            r = lv.hmc_sample(x0, 10_000, args.eps, n, **kw)
            torch.cuda.synchronize()
            ref['rows'] = 10_000
            ref['run_s'] = time.perf_counter() - t0
            ref['ms_per_step'] = ref['run_s'] / 9999 * 1e3
            ref['acceptance_per_chain'] = (r.accepted.double() / 9999).tolist()
            ref['n_failed_per_chain'] = r.n_failed.tolist()
            ref['log_p_last_row'] = r.log_p[:, -1].tolist()
        out['reference_run'] = ref

    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
