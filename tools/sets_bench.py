"""Naive-thinning curves: the set-batched forms against the per-set loop (writes profiles/sets_bench.json
and prints the same JSON line; needs a GPU).

Shapes:
  1. the Gaussian-mixture sample of Gaussian_mixture.ipynb: n = 1000, d = 2, sets naive_idx(1000, m) for
     m = 1..1000 (ksd_naive, naive_st against sample2);
  2. the LV surrogate of bench.py: n = 5e5, d = 4, the 250 thinned_sizes of lotka_volterra/Comparison.ipynb
     (rw_ksd_naive; rw_energy_distance_naive against a 5000-row reference set).
Legs per shape, on ONE resident integrand / cached reference set:
  * ksd_loop_s     -- [stein.ksd(integrand.reindex(set), m)[-1] for set in sets]: what the package offered
                      before the batch (one gather, one small triangle, one read-back per set);
  * ksd_sets_s     -- stein.ksd_sets(integrand, sets);
  * ksd_sets_resident_s -- DeviceProblem.ksd_sets with the concatenated rows already on the device: the
                      batch without the host's index handling and upload;
  * energy_loop_s  -- [sqrt(energy.energy_distance(ref, sample[set])) for set in sets];
  * energy_sets_s  -- energy.energy_distance_sets(ref, sample, sets).
Each shape is warmed up; the two forms of a metric alternate in one process; every timed window ends in
a device synchronise; medians of --reps (>= 20).  Shape 1 also runs the NumPy oracle once
(oracle.stein_numpy: calculate_ksd / energy_distance per set), next to the 1 min 47 s the notebook records
for its ksd_naive line.
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

NOTEBOOK_KSD_NAIVE_S = 107.0   # Gaussian_mixture.ipynb: "1min 47s" for the ksd_naive line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--shapes', default='gm,lv')
    ap.add_argument('--lv-rows', type=int, default=500_000)
    ap.add_argument('--no-oracle', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sets_bench.json'))
    args = ap.parse_args()
    if args.reps < 20:
        ap.error('--reps must be >= 20')

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit('sets_bench needs a HIP device: timings on a CPU say nothing about the GPU')
    from bench import lv_surrogate
    from oracle import models
    from oracle import stein_numpy as o
    from stein_thinning import energy, stein
    from stein_thinning import thinning as st
    from stein_thinning.naive import naive_idx

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()   # inside the window
        return time.perf_counter() - t0

    def shape(name, sample, gradient, ref_points, sizes):
        n = sample.shape[0]
        sets = [naive_idx(n, int(m)) for m in sizes]
        integrand = st._make_stein_integrand(sample, gradient)      # calculate_ksd's: standardised, 'id'
        prob = integrand.device_problem()
        rows_dev = torch.from_numpy(np.concatenate(sets).astype(np.int64)).to(prob.device)
        offsets = np.concatenate([[0], np.cumsum([s.shape[0] for s in sets])]).astype(np.int64)
        ref = energy.point_set(ref_points)
        ref.self_sum()
        rec = {'shape': name, 'n': n, 'd': int(sample.shape[1]), 'sets': len(sets),
               'set_rows': int(sum(s.shape[0] for s in sets)),
               'pairs': int(sum(s.shape[0] * (s.shape[0] - 1) // 2 for s in sets)), 'reference_rows': ref.n}
        res = {}
        legs = {
            'ksd_loop_s': lambda: res.__setitem__('ksd_loop', np.array(
                [stein.ksd(integrand.reindex(s), s.shape[0])[-1] for s in sets])),
            'ksd_sets_s': lambda: res.__setitem__('ksd_sets', stein.ksd_sets(integrand, sets)),
            'ksd_sets_resident_s': lambda: prob.ksd_sets(rows_dev, offsets),
            'energy_loop_s': lambda: res.__setitem__('energy_loop', np.array(
                [np.sqrt(energy.energy_distance(ref_points, sample[s])) for s in sets])),
            'energy_sets_s': lambda: res.__setitem__('energy_sets', energy.energy_distance_sets(ref, sample, sets)),
        }
        for fn in legs.values():           # warm-up of this shape
            timed(fn)
        times = {k: [] for k in legs}
        for _ in range(args.reps):         # alternating
            for k, fn in legs.items():
                times[k].append(timed(fn))
        for k, v in times.items():
            rec[k] = statistics.median(v)
            rec[k + '_min'], rec[k + '_max'] = min(v), max(v)
        rec['ksd_loop_over_sets'] = rec['ksd_loop_s'] / rec['ksd_sets_s']
        rec['energy_loop_over_sets'] = rec['energy_loop_s'] / rec['energy_sets_s']
        rec['ksd_max_rel_diff'] = float(np.max(np.abs(res['ksd_sets'] - res['ksd_loop']) / np.abs(res['ksd_loop'])))
        rec['energy_max_rel_diff'] = float(np.max(np.abs(res['energy_sets'] - res['energy_loop']) /
                                                  np.abs(res['energy_loop'])))
        return rec, sets, res

    out = {'tool': 'sets_bench', 'device': torch.cuda.get_device_name(0), 'reps': args.reps, 'shapes': []}
    for name in args.shapes.split(','):
        if name == 'gm':
            sample, sample2, _, score = models.gm_reference_sample()
            gradient = score(sample)
            rec, sets, res = shape('gm', sample, gradient, sample2, np.arange(1, 1001))
            rec['notebook_ksd_naive_s'] = NOTEBOOK_KSD_NAIVE_S
            if not args.no_oracle:
                t0 = time.perf_counter()
                want = np.array([o.calculate_ksd(sample, gradient, s)[-1] for s in sets])
                rec['oracle_ksd_s'] = time.perf_counter() - t0
                rec['oracle_ksd_max_rel_diff'] = float(np.max(np.abs(res['ksd_sets'] - want) / np.abs(want)))
                t0 = time.perf_counter()
                want = np.array([np.sqrt(o.energy_distance(sample2, sample[s])) for s in sets])
                rec['oracle_energy_s'] = time.perf_counter() - t0
                rec['oracle_energy_max_rel_diff'] = float(np.max(np.abs(res['energy_sets'] - want) / np.abs(want)))
        elif name == 'lv':
            x, g, _, _ = lv_surrogate(args.lv_rows, 12345)
            sizes = np.concatenate([np.linspace(5, 100, 50).astype(int), np.linspace(100, 10_000, 200).astype(int)])
            ref_points, _, _, _ = lv_surrogate(5000, 54321)
            rec, _, _ = shape('lv', x, g, ref_points, sizes)
        else:
            ap.error(f'unknown shape {name!r}')
        out['shapes'].append(rec)
        print(json.dumps(rec), flush=True)
    line = json.dumps(out)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
