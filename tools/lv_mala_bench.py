"""MALA sampler timings (st_lv_mala_wave, csrc/lv_mcmc.hip); one JSON line, also written to --out; needs a GPU.

Per chain count (default 5, 64, 1024, 4096), --steps Metropolis steps (default 256) from starts
log(THETA) + 0.02 N(0, I), step size --eps (0.003) and drift cap --cap (1.0), every fused leg as a sequence of
launches of --steps-per-launch steps (default lotka_volterra.STEPS_PER_LAUNCH_MALA):
  * mala_device_s   -- st_lv_mala_wave, Philox noise drawn in the kernel;
  * mala_supplied_s -- st_lv_mala_wave reading z / log_u from device arrays;
  * yardstick_s     -- what a user could do before the sampler for the same chains: per step one
                       st_lv_grad_log_posterior_ws launch (the two-phase gradient kernels) plus one
                       st_lv_log_target_density launch (2-state integration) plus torch elementwise ops (drift,
                       clip, proposal, exp, the two quadratic forms, accept) on the same supplied noise;
  * rw_wave_s       -- st_lv_rwmh_wave (random walk, step 0.0025, 2-state integration) on the same noise: what the
                       gradient costs.
Every window is the whole run between two device events with a synchronise on the second, after a warm-up of
every leg; the legs alternate and the figure is the median of --reps windows with [min, max].  ms_per_step = time /
steps; chain_steps_s = chains * steps / time; mala_launch_s = mala_device_s * steps_per_launch / steps.
The yardstick's density is the 2-state one, so its chains part from the fused kernel's; the two are compared at
the FUSED kernel's rows instead: max_rel_diff_grad (per row, relative to the row's largest component) between the
kernel's grad and exp(x) * st_lv_grad_log_posterior_ws, max_abs_diff_log_p / max_rel_diff_log_p between the
kernel's log_p (10-state solution) and st_lv_log_target_density (2-state solution): the latter is the
integrator's tolerance, not rounding.  At most 65 536 rows (every stride-th) are compared.
eps_sweep: acceptance at 5 chains over --steps steps for a few step sizes (device noise), over all steps and
over the second half (the first steps climb from the starts at the capped drift).
--reference-run: lotka_volterra.mala_sample from log(THETA_INITS), 5 chains, step size --eps, drift cap --cap,
max_steps 10 000: first ONE launch of 64 steps is timed; only if it stays under 0.25 s the run of 10 000 rows
follows, timed once."""
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
    ap.add_argument('--steps', type=int, default=256)
    ap.add_argument('--reps', type=int, default=3, help='timed windows per leg')
    ap.add_argument('--eps', type=float, default=0.003)
    ap.add_argument('--cap', type=float, default=1.0)
    ap.add_argument('--steps-per-launch', type=int, default=None)
    ap.add_argument('--eps-sweep', default='0.0005,0.001,0.002,0.003,0.004,0.006')
    ap.add_argument('--reference-run', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lv_mala_bench.json'))
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit('lv_mala_bench needs a HIP device: timings on a CPU say nothing about the GPU')
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
    steps = args.steps
    spl = lv.STEPS_PER_LAUNCH_MALA if args.steps_per_launch is None else args.steps_per_launch
    eps = np.full(4, args.eps)
    ehw = np.ascontiguousarray(np.concatenate([eps, 0.5 * eps * eps, 0.5 / (eps * eps)]))
    clip = np.ascontiguousarray(args.cap * eps)
    rw_step = np.full(4, 0.0025)

    def window(fn):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) * 1e-3

    out = {'tool': 'lv_mala_bench', 'device': torch.cuda.get_device_name(0), 'reps': args.reps, 'steps': steps,
           'steps_per_launch': spl, 'eps': args.eps, 'drift_cap': args.cap, 'rw_step_size': 0.0025,
           't_n': int(t.size), 'shapes': []}
    for chains in (int(v) for v in args.chains.split(',')):
        rng = np.random.default_rng(chains)
        x0 = torch.from_numpy(np.log(lv.THETA) + 0.02 * rng.normal(size=(chains, 4))).to(dev)
        gen = torch.Generator(device=dev).manual_seed(chains)
        z = torch.randn((chains, steps, 4), dtype=torch.float64, device=dev, generator=gen)
        log_u = torch.rand((chains, steps), dtype=torch.float64, device=dev, generator=gen).log()
        res = {}

        def mala(mode, name):
            state = torch.zeros((chains, 16), dtype=torch.float64, device=dev)
            samples = torch.empty((chains, steps + 1, 4), dtype=torch.float64, device=dev)
            grad = torch.empty((chains, steps + 1, 4), dtype=torch.float64, device=dev)
            log_p = torch.empty((chains, steps + 1), dtype=torch.float64, device=dev)
            res[name] = (samples, log_p, grad, state)

            def run():
                state.zero_()
                state[:, :4] = x0
                for k0 in range(0, steps, spl):
                    k = min(spl, steps - k0)
                    nat.check(L.st_lv_mala_wave(
                        nat.ptr(state), chains, 0, k0 + 1, k, 1 if k0 == 0 else 0, ehw.ctypes.data, clip.ctypes.data,
                        mode, 1, nat.ptr(z) if mode == 0 else None, nat.ptr(log_u) if mode == 0 else None, steps, k0,
                        nat.ptr(td), t.size, nat.ptr(yd), s.ctypes.data, U.ctypes.data, c_log, norm_logc,
                        cinv.ctypes.data, lv.MAX_STEPS, nat.ptr(samples), nat.ptr(log_p), nat.ptr(grad), steps + 1,
                        k0 + 1, stream), 'st_lv_mala_wave')
            return run

        def rw_wave():
            state = torch.zeros((chains, 8), dtype=torch.float64, device=dev)
            samples = torch.empty((chains, steps + 1, 4), dtype=torch.float64, device=dev)
            log_p = torch.empty((chains, steps + 1), dtype=torch.float64, device=dev)
            res['rw_wave_s'] = (samples, log_p, None, state)

            def run():
                state.zero_()
                state[:, :4] = x0
                nat.check(L.st_lv_rwmh_wave(nat.ptr(state), chains, 0, 1, steps, 1, rw_step.ctypes.data, 0, 1,
                                            nat.ptr(z), nat.ptr(log_u), steps, 0, nat.ptr(td), t.size, nat.ptr(yd),
                                            s.ctypes.data, U.ctypes.data, c_log, norm_logc, lv.MAX_STEPS,
                                            nat.ptr(samples), nat.ptr(log_p), steps + 1, 1, stream), 'st_lv_rwmh_wave')
            return run

        gout = torch.empty((chains * (steps + 1), 4), dtype=torch.float64, device=dev)
        dout = torch.empty(chains * (steps + 1), dtype=torch.float64, device=dev)
        status = torch.zeros(chains * (steps + 1), dtype=torch.int32, device=dev)

        def gradient(th, n):
            wb = int(L.st_lv_grad_workspace_bytes(n, t.size))
            if res.get('gws_bytes', 0) < wb:
                res['gws'], res['gws_bytes'] = torch.empty((wb + 7) // 8, dtype=torch.float64, device=dev), wb
            nat.check(L.st_lv_grad_log_posterior_ws(nat.ptr(th), n, nat.ptr(td), t.size, nat.ptr(yd), s.ctypes.data,
                                                    cinv.ctypes.data, lv.MAX_STEPS, nat.ptr(gout), nat.ptr(status),
                                                    nat.ptr(res['gws']), wb, stream), 'st_lv_grad_log_posterior_ws')
            return gout[:n]

        def density(p, th, n):
            wb = int(L.st_lv_log_density_workspace_bytes(n, t.size))
            if res.get('dws_bytes', 0) < wb:
                res['dws'], res['dws_bytes'] = torch.empty((wb + 7) // 8, dtype=torch.float64, device=dev), wb
            nat.check(L.st_lv_log_target_density(nat.ptr(p), nat.ptr(th), n, nat.ptr(td), t.size, nat.ptr(yd),
                                                 s.ctypes.data, U.ctypes.data, c_log, norm_logc, lv.MAX_STEPS,
                                                 nat.ptr(dout), nat.ptr(status), nat.ptr(res['dws']), wb, stream),
                      'st_lv_log_target_density')
            return dout[:n]

        def yardstick():
            samples = torch.empty((chains, steps + 1, 4), dtype=torch.float64, device=dev)
            log_p = torch.empty((chains, steps + 1), dtype=torch.float64, device=dev)
            grads = torch.empty((chains, steps + 1, 4), dtype=torch.float64, device=dev)
            epsd, hd, wd = (torch.from_numpy(ehw[4 * q:4 * q + 4].copy()).to(dev) for q in range(3))
            cd = torch.from_numpy(clip).to(dev)
            res['yardstick_s'] = (samples, log_p, grads, None)

            def run():
                x = x0.clone()
                th = torch.exp(x)
                g = (th * gradient(th, chains)).clone()
                lp = density(x, th, chains).clone()
                samples[:, 0], log_p[:, 0], grads[:, 0] = x, lp, g
                for k in range(steps):
                    d = torch.minimum(torch.maximum(hd * g, -cd), cd)
                    p = ((x + d) + epsd * z[:, k]).contiguous()
                    th = torch.exp(p)
                    g_new = th * gradient(th, chains)
                    lp_new = density(p, th, chains)
                    rf = (p - x) - d
                    rr = (x - p) - torch.minimum(torch.maximum(hd * g_new, -cd), cd)
                    qf, qr = (wd * rf * rf).sum(dim=1), (wd * rr * rr).sum(dim=1)
                    acc = log_u[:, k] < (lp_new - lp) + (qf - qr)
                    x = torch.where(acc[:, None], p, x)
                    g = torch.where(acc[:, None], g_new, g)
                    lp = torch.where(acc, lp_new, lp)
                    samples[:, k + 1], log_p[:, k + 1], grads[:, k + 1] = x, lp, g
            return run

        legs = {'mala_device_s': mala(1, 'mala_device_s'), 'mala_supplied_s': mala(0, 'mala_supplied_s'),
                'yardstick_s': yardstick(), 'rw_wave_s': rw_wave()}
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
        rec['mala_launch_s'] = rec['mala_device_s'] * min(spl, steps) / steps
        rec['yardstick_over_mala'] = rec['yardstick_s'] / rec['mala_supplied_s']
        rec['mala_over_rw_wave'] = rec['mala_supplied_s'] / rec['rw_wave_s']
        torch.cuda.synchronize()
        ms, ml, mg, mstate = res['mala_supplied_s']
        counts = mstate.view(torch.int64)
        rec['acceptance'] = float(counts[:, 5].double().mean()) / steps
        rec['n_failed'] = int(counts[:, 6].sum())
        ys, yl, yg, _ = res['yardstick_s']
        moved = (ys[:, 1:] != ys[:, :-1]).any(dim=2)
        rec['yardstick_acceptance'] = float(moved.double().mean())
        rec['rw_wave_acceptance'] = float(res['rw_wave_s'][3].view(torch.int64)[:, 5].double().mean()) / steps
        # the yardstick's two launches at the fused kernel's rows
        # (every stride-th row, at most 65 536 of them: the two workspaces take ~48 KB per row)
        stride = -(-(chains * (steps + 1)) // 65536)
        rows = ms.reshape(-1, 4)[::stride].contiguous()
        th = torch.exp(rows)
        n = rows.shape[0]
        want_g = th * gradient(th, n)
        want_lp = density(rows, th, n)
        gd = (mg.reshape(-1, 4)[::stride] - want_g).abs().amax(dim=1) / want_g.abs().amax(dim=1)
        ld = (ml.reshape(-1)[::stride] - want_lp).abs()
        rec['rows_compared'] = n
        rec['max_rel_diff_grad'] = float(gd.max())
        rec['max_abs_diff_log_p'] = float(ld.max())
        rec['max_rel_diff_log_p'] = float((ld / want_lp.abs()).max())
        rec['max_abs_log_p'] = float(want_lp.abs().max())
        out['shapes'].append(rec)
        print(json.dumps(rec), file=sys.stderr, flush=True)
        del res, legs, z, log_u, gout, dout, status

    sweep = []
    x5 = np.log(lv.THETA) + 0.02 * np.random.default_rng(5).normal(size=(5, 4))
    for e in (float(v) for v in args.eps_sweep.split(',') if v):
        r = lv.mala_sample(x5, steps + 1, e, seed=1, drift_cap=args.cap, data=data)
        moved = np.any(r.samples[:, 1:] != r.samples[:, :-1], axis=2)
        sweep.append({'eps': e, 'acceptance': float(moved.mean()),
                      'acceptance_second_half': float(moved[:, steps // 2:].mean()),
                      'per_chain': moved.mean(axis=1).tolist(), 'n_failed': int(r.n_failed.sum())})
    out['eps_sweep'] = {'chains': 5, 'steps': steps, 'drift_cap': args.cap, 'seed': 1, 'runs': sweep}

    if args.reference_run:
        x0 = np.log(lv.THETA_INITS)
        kw = dict(seed=1, drift_cap=args.cap, data=data, max_steps=10_000, device_out=True)
        lv.mala_sample(x0, 3, args.eps, **kw)                       # warm-up: 2 steps
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = lv.mala_sample(x0, 65, args.eps, steps_per_launch=64, **kw)
        torch.cuda.synchronize()
        ref = {'eps': args.eps, 'drift_cap': args.cap, 'max_steps': 10_000, 'launch_64_steps_s': time.perf_counter() - t0,
               'launch_n_failed': int(r.n_failed.sum())}
        if ref['launch_64_steps_s'] < 0.25:
            t0 = time.perf_counter()
            r = lv.mala_sample(x0, 10_000, args.eps, **kw)
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
