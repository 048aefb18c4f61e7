"""Dense-preconditioner timings against the isotropic launch-per-step path (one JSON line; needs a GPU).

Shapes: the config-2 shape n = 2e5, d = 4, m = 100 and n = 2e6, d = 4, m = 1000, surrogate inputs from
bench.lv_surrogate.  Per shape, on device-resident standardised rows:
  * dense_thin_s  -- the greedy run of thin(..., preconditioner='smpcov') (st_greedy_dense);
  * iso_steps_s   -- DeviceProblem.greedy_steps_launch on the same rows with 'med': the isotropic
                     launch-per-step path the dense kernel is modelled on;
  * thin_e2e_s    -- thin(x, g, m, preconditioner='smpcov') from host arrays, preparation included;
and once: the dense cumulative KSD of 2e5 rows against the isotropic one.
Each shape is warmed up; the two greedy legs alternate in one process; every timed window ends in a
device synchronise; medians of --reps (>= 20) thins.  --iso-only runs the isotropic legs alone, for a
build without the dense entry points (ST_HIP_LIB=<the parent commit's library>): "dense step path =
X x the parent's isotropic step path" compares dense_thin_s here with iso_steps_s there.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--ksd-reps', type=int, default=5)
    ap.add_argument('--ksd-rows', type=int, default=200_000)
    ap.add_argument('--e2e-reps', type=int, default=5)
    ap.add_argument('--shapes', default='200000:100,2000000:1000', help='n:m,...')
    ap.add_argument('--iso-only', action='store_true')
    args = ap.parse_args()
    if args.reps < 20:
        ap.error('--reps must be >= 20')

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit('dense_bench needs a HIP device: timings on a CPU say nothing about the GPU')
    from bench import lv_surrogate
    from stein_thinning import thinning as st
    from stein_thinning.device import DeviceProblem
    from stein_thinning.kernel import make_precon

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()   # inside the window: the launches only enqueue
        return time.perf_counter() - t0

    out = {'tool': 'dense_bench', 'device': torch.cuda.get_device_name(0), 'reps': args.reps,
           'lib': 'ST_HIP_LIB build' if os.environ.get('ST_HIP_LIB') else 'in-tree', 'shapes': []}
    shapes = [tuple(int(v) for v in s.split(':')) for s in args.shapes.split(',')]
    probs = []
    for n, m in shapes:
        x, g, _, _ = lv_surrogate(n, 12345)
        xs, gs = st._validate_and_standardize(x, g, True)
        med = make_precon(xs, 'med')
        iso = DeviceProblem(xs, gs, None, float(med[0, 0]), float(np.trace(med)))
        iso.wait_upload()
        iso_buf = iso.greedy_buffers(m)
        rec = {'n': n, 'd': int(xs.shape[1]), 'm': m}
        legs = {'iso_steps_s': lambda: iso.greedy_steps_launch(m, *iso_buf)}
        if not args.iso_only:
            L = make_precon(xs, 'smpcov')
            dense = DeviceProblem.from_soa(iso.x, iso.g, None, n, 0.0, float(np.trace(L)), linv=L)
            dense_buf = dense.greedy_buffers(m)
            legs['dense_thin_s'] = lambda: dense.greedy_launch(m, *dense_buf)
        for fn in legs.values():           # warm-up of this shape
            timed(fn)
        times = {k: [] for k in legs}
        for _ in range(args.reps):         # alternating
            for k, fn in legs.items():
                times[k].append(timed(fn))
        for k, v in times.items():
            rec[k] = statistics.median(v)
            rec[k + '_min'], rec[k + '_max'] = min(v), max(v)
        rec['iso_first_indices'] = iso_buf[0][:8].cpu().numpy().view(np.uint32).tolist()
        if not args.iso_only:
            rec['dense_first_indices'] = dense_buf[0][:8].cpu().numpy().view(np.uint32).tolist()
            rec['dense_over_iso_steps'] = rec['dense_thin_s'] / rec['iso_steps_s']
            timed(lambda: st.thin(x, g, m, preconditioner='smpcov'))
            rec['thin_e2e_s'] = statistics.median(
                [timed(lambda: st.thin(x, g, m, preconditioner='smpcov')) for _ in range(args.e2e_reps)])
        out['shapes'].append(rec)
        probs.append((iso, None if args.iso_only else dense))
    fits = [p for p in probs if p[0].n >= args.ksd_rows]
    big = fits[0] if fits else max(probs, key=lambda p: p[0].n)
    k = min(args.ksd_rows, big[0].n)
    ksd = {'rows': k, 'reps': args.ksd_reps}
    legs = {'iso_ksd_s': lambda: big[0].ksd(k)}
    if not args.iso_only:
        legs['dense_ksd_s'] = lambda: big[1].ksd(k)
    for fn in legs.values():
        timed(fn)
    times = {name: [] for name in legs}
    for _ in range(args.ksd_reps):
        for name, fn in legs.items():
            times[name].append(timed(fn))
    for name, v in times.items():
        ksd[name] = statistics.median(v)
    if not args.iso_only:
        ksd['dense_over_iso'] = ksd['dense_ksd_s'] / ksd['iso_ksd_s']
    out['ksd'] = ksd
    print(json.dumps(out))


if __name__ == '__main__':
    main()
