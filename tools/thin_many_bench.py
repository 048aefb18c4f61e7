"""thin_many timings (csrc/many.hip: one workgroup per chain); one JSON document, printed and written to --out;
needs a GPU.

Inputs: device-resident float64 (C, n, 4) chains that look like random-walk Metropolis output (about 75 % repeated
rows) with the score of a Gaussian target, generated on the device from a seed.  Per shape (C, n, m) and
preconditioner, after a warm-up of every leg, the median of --reps windows with [min, max]:
  * stats_s    -- st_chain_stats (device events around the call);
  * median_s   -- 'med' only: st_pdist_many + torch.sort per chunk + the middle values to the host + the per-chain
                  make_precon arithmetic (host clock; ends with the values on the host);
  * greedy_s   -- st_greedy_many alone (device events): chain_steps_s = C m / greedy_s, pair_evals_s =
                  C n m / greedy_s (the diagonal and m - 1 sweeps of n pairs), fp64_peak_share = pair_evals_s * 101
                  fp64 instructions per pair of the exact arithmetic / 39.3e12 lane-instructions
                  per second (256 CUs x 4 SIMDs x 16 lanes at the nominal 2.4 GHz, the 4-cycle fp64 issue peak);
  * thin_many_s -- thinning.thin_many end to end on the device tensors (host clock; the indices are on the host
                  when it returns);
  * yardstick_s -- thinning.thin_chains on the same tensors, chain by chain as before this engine (its defaults:
                  compact arithmetic, dedup and guard on), in the same process and session.  Timed in full for
                  C <= --yardstick-chains (512); for a larger C it is timed on the first 512 chains and multiplied by
                  C / 512: those figures carry "yardstick_extrapolated": true.
The gradient-free row times thin_gf_many against thin_gf_chains the same way (log densities as host arrays).
Both sides return the same indices on the chains the yardstick ran (checked; "same_indices")."""
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

FP64_ISSUE_PEAK = 256 * 4 * 16 * 2.4e9     # lane-instructions per second
EXACT_INSTR_PER_PAIR = 101
SHAPES = '512x1024x20,4096x1024x20,65536x256x20,1024x4096x100'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default=SHAPES, help='comma-separated CxNxM')
    ap.add_argument('--precons', default='id,med')
    ap.add_argument('--gf-shape', default='4096x1024x20', help="the gradient-free row ('' to skip)")
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--yardstick-reps', type=int, default=3)
    ap.add_argument('--yardstick-chains', type=int, default=512)
    ap.add_argument('--seed', type=int, default=20261021)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'thin_many_bench.json'))
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit('thin_many_bench needs a HIP device: timings on a CPU say nothing about the GPU')
    from stein_thinning import _native as nat
    from stein_thinning import thinning as st
    dev = nat.require_device()
    d = 4
    mu = torch.linspace(-1.0, 2.0, d, dtype=torch.float64, device=dev)
    s2 = torch.linspace(0.5, 3.0, d, dtype=torch.float64, device=dev)

    def chains(C, n):
        gen = torch.Generator(device=dev)
        gen.manual_seed(args.seed + C + n)
        moved = torch.rand((C, n, 1), generator=gen, device=dev) < 0.25
        moved[:, :3] = True
        step = torch.randn((C, n, d), generator=gen, device=dev, dtype=torch.float64) * torch.sqrt(s2) * 0.7
        start = mu + torch.randn((C, 1, d), generator=gen, device=dev, dtype=torch.float64)
        x = start + torch.cumsum(torch.where(moved, step, torch.zeros_like(step)), dim=1)
        return x.contiguous(), (-(x - mu) / s2).contiguous()

    def spread(ts):
        return {'median': statistics.median(ts), 'min': min(ts), 'max': max(ts)}

    def events(fn, reps):
        fn()
        out = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            fn()
            b.record()
            b.synchronize()
            out.append(a.elapsed_time(b) * 1e-3)
        return spread(out)

    def clock(fn, reps, warm=1):
        res = None
        for _ in range(warm):
            res = fn()
        out = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn()
            torch.cuda.synchronize()
            out.append(time.perf_counter() - t0)
        return spread(out), res

    def row(C, n, m, precon, gf):
        x, g = chains(C, n)
        rec = {'chains': C, 'n': n, 'n_points': m, 'd': d, 'preconditioner': precon, 'gradient_free': gf}
        rec['plan_threads_rows'] = list(_plan(nat, n, d, gf))
        log_p = log_q = w_dev = None
        if gf:
            log_p = (-0.5 * ((x - mu) ** 2 / s2).sum(-1)).cpu().numpy()
            log_q = (-0.5 * ((x - mu) ** 2 / (1.3 * s2)).sum(-1)).cpu().numpy()
            g = (-(x - mu) / (1.3 * s2)).contiguous()
        rec['stats_s'] = events(lambda: st._many_stats(x, g, True), args.reps)
        _, scl, _ = st._many_stats(x, g, True)
        if precon == 'med':
            rec['median_s'], scales = clock(lambda: st._many_precon_scales(n, d, precon, st._many_medians(x, scl)),
                                            args.reps)
            l, tr = (torch.from_numpy(a).to(dev) for a in scales[:2])
        else:
            l = torch.ones(C, dtype=torch.float64, device=dev)
            tr = torch.full((C,), float(d), dtype=torch.float64, device=dev)
        if gf:
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                w_dev = torch.from_numpy(st._many_gf_weights(log_p, log_q, C, n, None, C)[0]).to(dev)
        idx = torch.empty((C, m), dtype=torch.int32, device=dev)
        L, stream = nat.lib(), nat.stream_handle()

        def greedy():
            nat.check(L.st_greedy_many(nat.ptr(x), nat.ptr(g), nat.ptr(scl), nat.ptr(w_dev), nat.ptr(l), nat.ptr(tr),
                                       C, n, d, m, nat.ptr(idx), None, stream), 'st_greedy_many')
        rec['greedy_s'] = events(greedy, args.reps)
        t = rec['greedy_s']['median']
        rec['chain_steps_s'] = C * m / t
        rec['pair_evals_s'] = C * n * m / t
        rec['fp64_peak_share'] = rec['pair_evals_s'] * EXACT_INSTR_PER_PAIR / FP64_ISSUE_PEAK
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            if gf:
                rec['thin_many_s'], got = clock(lambda: st.thin_gf_many(x, log_p, log_q, g, m, preconditioner=precon),
                                                args.reps)
            else:
                rec['thin_many_s'], got = clock(lambda: st.thin_many(x, g, m, preconditioner=precon), args.reps)
            assert st.last_engine == 'many'
            Y = min(C, args.yardstick_chains)
            xs, gs = [x[c] for c in range(Y)], [g[c] for c in range(Y)]
            if gf:
                yard, want = clock(lambda: st.thin_gf_chains(xs, list(log_p[:Y]), list(log_q[:Y]), gs, m,
                                                             preconditioner=precon), args.yardstick_reps)
            else:
                yard, want = clock(lambda: st.thin_chains(xs, gs, m, preconditioner=precon), args.yardstick_reps)
        rec['same_indices'] = bool(np.array_equal(np.stack(want), got[:Y]))
        rec['yardstick_chains_timed'] = Y
        rec['yardstick_extrapolated'] = Y < C
        rec['yardstick_timed_s'] = yard
        rec['yardstick_s'] = yard['median'] * C / Y
        rec['speedup_end_to_end'] = rec['yardstick_s'] / rec['thin_many_s']['median']
        print(json.dumps(rec), flush=True)
        return rec

    def shape(s):
        return tuple(int(v) for v in s.split('x'))
    rows = []
    for s in args.shapes.split(','):
        for precon in args.precons.split(','):
            rows.append(row(*shape(s), precon, False))
    if args.gf_shape:
        rows.append(row(*shape(args.gf_shape), 'id', True))
    doc = {'tool': 'tools/thin_many_bench.py', 'device': torch.cuda.get_device_name(dev), 'reps': args.reps,
           'yardstick': 'thinning.thin_chains / thin_gf_chains on the same device tensors, same process',
           'fp64_issue_peak_lane_instr_s': FP64_ISSUE_PEAK, 'exact_instr_per_pair': EXACT_INSTR_PER_PAIR,
           'rows': rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')
    print(json.dumps({'written': args.out, 'rows': len(rows)}))


def _plan(nat, n, d, weights):
    import ctypes
    t, r = ctypes.c_int32(0), ctypes.c_int32(0)
    nat.check(nat.lib().st_greedy_many_plan(n, d, 1 if weights else 0, ctypes.byref(t), ctypes.byref(r)),
              'st_greedy_many_plan')
    return t.value, r.value


if __name__ == '__main__':
    main()
