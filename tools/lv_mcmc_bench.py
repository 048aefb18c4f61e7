"""Random-walk Metropolis sampler timings (st_lv_rwmh, st_lv_rwmh_wave, csrc/lv_mcmc.hip); one JSON line, also
written to --out; needs a GPU.

Per chain count (default 5, 4096, 65536), --steps Metropolis steps (default 256) from starts near log(THETA):
  * fused_device_s   -- one st_lv_rwmh launch, Philox noise drawn in the kernel;
  * fused_supplied_s -- one st_lv_rwmh launch reading z / log_u from device arrays;
  * yardstick_s      -- the same chains from what the library had before the sampler: per step one
                        st_lv_log_target_density launch (two kernels and a (t_n, chains) scratch array) plus torch
                        elementwise propose / exp / accept on device tensors, on the same supplied noise
                        (--no-yardstick leaves this leg, its comparisons and the oracle timing out);
  * wave_device_s, wave_supplied_s -- the two fused legs through st_lv_rwmh_wave (one wave per chain), for chain
                        counts up to 4096 only: beyond that the replicated integrator makes a launch long.
                        wave_over_thread_supplied / _device = wave time / fused time; wave_rows_equal: the share of
                        rows on which the two layouts agree bit for bit on the same supplied noise;
                        wave_max_abs_diff_log_p: the largest difference of log_p between them on such rows (the two
                        summation orders).
The record of the thread layout is profiles/lv_mcmc_bench.json (the defaults); the wave sweep is
  --chains 5,64,256,1024,4096 --no-yardstick --out profiles/lv_mcmc_wave_bench.json
Every window is the whole run of --steps steps between two device events with a synchronise on the second, after a
warm-up of every leg; the legs alternate and the figure is the median of --reps windows.  chain_steps_s =
chains * steps / time; ms_per_step = time / steps; yardstick_over_fused = yardstick_s / fused_supplied_s.
rows_equal: the share of rows on which the yardstick and the fused kernel agree bit for bit (the two sum the
observation terms in different orders, ~1e-13 apart, so a decision may fall differently once in a long while and the
chains part from there; 1.0 is the usual outcome at these lengths); max_abs_diff_log_p_on_equal_rows: the largest
difference of log_p between the two on such rows.
oracle_eval_s: oracle.lv_numpy.log_target_density (scipy) per evaluation on one host core.
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


WAVE_LEG_MAX_CHAINS = 4096


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--chains', default='5,4096,65536')
    ap.add_argument('--steps', type=int, default=256)
    ap.add_argument('--reps', type=int, default=3, help='timed windows per leg')
    ap.add_argument('--oracle-evals', type=int, default=20)
    ap.add_argument('--no-yardstick', action='store_true', help='fused legs only (thread and wave layouts)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lv_mcmc_bench.json'))
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit('lv_mcmc_bench needs a HIP device: timings on a CPU say nothing about the GPU')
    from oracle import lv_numpy as ol
    from stein_thinning import _native as nat
    from stein_thinning import lotka_volterra as lv
    from stein_thinning.proxy import PsdFactor
    dev = nat.require_device()
    L = nat.lib()
    stream = nat.stream_handle()
    data = lv.reference_data()
    t, y, s = lv._settings(data, lv.RTOL, lv.ATOL)
    psd = PsdFactor(np.asarray(data.cov, dtype=np.float64), allow_singular=False)
    c_log = psd.rank * float(np.log(2 * np.pi)) + psd.log_pdet
    U = np.ascontiguousarray(psd.U, dtype=np.float64)
    norm_logc = float(np.log(np.sqrt(2 * np.pi)))
    td, yd = (torch.from_numpy(a).to(dev) for a in (t, y))
    step = np.full(4, 0.0025)
    steps = args.steps

    def window(fn):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) * 1e-3

    out = {'tool': 'lv_mcmc_bench', 'device': torch.cuda.get_device_name(0), 'reps': args.reps, 'steps': steps,
           'step_size': 0.0025, 't_n': int(t.size), 'shapes': []}
    for chains in (int(v) for v in args.chains.split(',')):
        rng = np.random.default_rng(chains)
        x0 = torch.from_numpy(np.log(lv.THETA) + 0.02 * rng.normal(size=(chains, 4))).to(dev)
        gen = torch.Generator(device=dev).manual_seed(chains)
        z = torch.randn((chains, steps, 4), dtype=torch.float64, device=dev, generator=gen)
        log_u = torch.rand((chains, steps), dtype=torch.float64, device=dev, generator=gen).log()
        res = {}

        def fused(mode, name, entry='st_lv_rwmh'):
            state = torch.zeros((chains, 8), dtype=torch.float64, device=dev)
            samples = torch.empty((chains, steps + 1, 4), dtype=torch.float64, device=dev)
            log_p = torch.empty((chains, steps + 1), dtype=torch.float64, device=dev)
            res[name] = (samples, log_p, state)

            def run():
                state.zero_()
                state[:, :4] = x0
                nat.check(getattr(L, entry)(nat.ptr(state), chains, 0, 1, steps, 1, step.ctypes.data, mode, 1,
                                            nat.ptr(z) if mode == 0 else None, nat.ptr(log_u) if mode == 0 else None,
                                            steps, 0, nat.ptr(td), t.size, nat.ptr(yd), s.ctypes.data, U.ctypes.data,
                                            c_log, norm_logc, lv.MAX_STEPS, nat.ptr(samples), nat.ptr(log_p),
                                            steps + 1, 1, stream), entry)
            return run

        def yardstick():
            samples = torch.empty((chains, steps + 1, 4), dtype=torch.float64, device=dev)
            log_p = torch.empty((chains, steps + 1), dtype=torch.float64, device=dev)
            new = torch.empty(chains, dtype=torch.float64, device=dev)
            status = torch.zeros(chains, dtype=torch.int32, device=dev)
            wb = int(L.st_lv_log_density_workspace_bytes(chains, t.size))
            work = torch.empty((wb + 7) // 8, dtype=torch.float64, device=dev)
            stepd = torch.from_numpy(step).to(dev)
            res['yardstick_s'] = (samples, log_p, None)

            def density(p):
                th = torch.exp(p)
                nat.check(L.st_lv_log_target_density(nat.ptr(p), nat.ptr(th), chains, nat.ptr(td), t.size, nat.ptr(yd),
                                                     s.ctypes.data, U.ctypes.data, c_log, norm_logc, lv.MAX_STEPS,
                                                     nat.ptr(new), nat.ptr(status), nat.ptr(work), wb, stream),
                          'st_lv_log_target_density')
                return new

            def run():
                x = x0.clone()
                lp = density(x).clone()
                samples[:, 0], log_p[:, 0] = x, lp
                for k in range(steps):
                    p = x + stepd * z[:, k]
                    lp_new = density(p)
                    acc = log_u[:, k] < lp_new - lp
                    x = torch.where(acc[:, None], p, x)
                    lp = torch.where(acc, lp_new, lp)
                    samples[:, k + 1], log_p[:, k + 1] = x, lp
            return run

        legs = {'fused_device_s': fused(1, 'fused_device_s'), 'fused_supplied_s': fused(0, 'fused_supplied_s')}
        if chains <= WAVE_LEG_MAX_CHAINS:
            legs['wave_device_s'] = fused(1, 'wave_device_s', 'st_lv_rwmh_wave')
            legs['wave_supplied_s'] = fused(0, 'wave_supplied_s', 'st_lv_rwmh_wave')
        if not args.no_yardstick:
            legs['yardstick_s'] = yardstick()
        for fn in legs.values():
            window(fn)
        times = {name: [] for name in legs}
        for _ in range(args.reps):
            for name, fn in legs.items():
                times[name].append(window(fn))
        rec = {'chains': chains, 'chain_steps': chains * steps}
        for name, v in times.items():
            key = name[:-2]
            rec[name] = statistics.median(v)
            rec[key + '_min_s'], rec[key + '_max_s'] = min(v), max(v)
            rec[key + '_ms_per_step'] = rec[name] / steps * 1e3
            rec[key + '_chain_steps_s'] = chains * steps / rec[name]
        torch.cuda.synchronize()
        fs, fl, fstate = res['fused_supplied_s']
        counts = fstate.view(torch.int64)
        rec['acceptance'] = float(counts[:, 5].double().mean()) / steps
        rec['n_failed'] = int(counts[:, 6].sum())
        if 'wave_supplied_s' in legs:
            rec['wave_over_thread_supplied'] = rec['wave_supplied_s'] / rec['fused_supplied_s']
            rec['wave_over_thread_device'] = rec['wave_device_s'] / rec['fused_device_s']
            ws, wl, wstate = res['wave_supplied_s']
            same = (fs == ws).all(dim=2)
            rec['wave_rows_equal'] = float(same.double().mean())
            rec['wave_max_abs_diff_log_p'] = float(torch.where(same, (fl - wl).abs(), torch.zeros_like(fl)).max())
            rec['wave_n_failed'] = int(wstate.view(torch.int64)[:, 6].sum())
        if not args.no_yardstick:
            rec['yardstick_over_fused'] = rec['yardstick_s'] / rec['fused_supplied_s']
            ys, yl, _ = res['yardstick_s']
            rec['rows_equal'] = float((fs == ys).all(dim=2).double().mean())
            # log_p of equal rows: the two summation orders.  The terms of the sum have both signs, so a chain that
            # climbs through log_p = 0 has rows where the sum cancels: the difference is given in absolute terms, beside
            # |log_p| of the row that holds the largest one and the largest |log_p| of the run
            same = (fs == ys).all(dim=2)
            diff = torch.where(same, (fl - yl).abs(), torch.zeros_like(fl))
            worst = int(diff.argmax())
            rec['max_abs_diff_log_p_on_equal_rows'] = float(diff.flatten()[worst])
            rec['abs_log_p_at_that_row'] = float(yl.flatten()[worst].abs())
            rec['max_abs_log_p'] = float(yl.abs().max())
        out['shapes'].append(rec)
        del res, legs, z, log_u

    if not args.no_yardstick:
        lt = np.log(lv.THETA)
        ol.log_target_density(lt, data.t, data.y, data.cov)
        t0 = time.perf_counter()
        for k in range(args.oracle_evals):
            ol.log_target_density(lt + 1e-3 * k, data.t, data.y, data.cov)
        out['oracle_eval_s'] = (time.perf_counter() - t0) / max(args.oracle_evals, 1)
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
