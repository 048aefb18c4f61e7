"""The reference's sampling stage at full length: rw_sample from the five theta_inits, 500 000 rows per chain,
layout='wave', device noise -- ONE timed run (host clock around the call, ending in a device synchronise, after a
300-row warm-up of both layouts); one JSON line, also written to --out; needs a GPU.

Beside it, because a launch lasts as long as its slowest chain:
  * single -- each start alone in the wave layout for --single-rows rows: ms per step and acceptance per start;
  * both   -- all five starts for --both-rows rows in the wave and in the thread layout on the same seed: the
              two times, the share of rows equal bit for bit and the largest |log_p| difference on such rows.
              thread_full_run_extrapolated_s = the thread layout's ms per step here times the full row count
              (an EXTRAPOLATION: the thread layout is not run at full length).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'gradient-free-mcmc-postprocessing_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=500000)
    ap.add_argument('--single-rows', type=int, default=50000)
    ap.add_argument('--both-rows', type=int, default=20000)
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lv_mcmc_wave_full_run.json'))
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit('lv_mcmc_full_run needs a HIP device: timings on a CPU say nothing about the GPU')
    from stein_thinning import lotka_volterra as lv
    data = lv.reference_data()
    x0 = np.log(lv.THETA_INITS)

    def timed(x, rows, layout, first_chain=0):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = lv.rw_sample(x, rows, seed=args.seed, data=data, device_out=True, layout=layout, first_chain=first_chain)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    timed(x0, 300, 'wave')
    timed(x0, 300, 'thread')
    out = {'tool': 'lv_mcmc_full_run', 'device': torch.cuda.get_device_name(0), 'seed': args.seed, 'step_size': 0.0025,
           'steps_per_launch_wave': lv.STEPS_PER_LAUNCH_WAVE, 'steps_per_launch_thread': lv.STEPS_PER_LAUNCH}
    dt, r = timed(x0, args.rows, 'wave')
    out['full'] = {'layout': 'wave', 'chains': 5, 'rows': args.rows, 'seconds': dt,
                   'ms_per_step': dt / (args.rows - 1) * 1e3,
                   'acceptance': (r.accepted.double() / (args.rows - 1)).tolist(), 'n_failed': r.n_failed.tolist(),
                   'log_p_last': r.log_p[:, -1].tolist()}
    del r
    out['single'] = []
    for c in range(5):
        dt, r = timed(x0[c:c + 1], args.single_rows, 'wave', first_chain=c)
        out['single'].append({'chain': c, 'theta_init': lv.THETA_INITS[c].tolist(), 'rows': args.single_rows,
                              'seconds': dt, 'ms_per_step': dt / (args.single_rows - 1) * 1e3,
                              'acceptance': float(r.accepted[0]) / (args.single_rows - 1),
                              'log_p_last': float(r.log_p[0, -1])})
    dw, rw = timed(x0, args.both_rows, 'wave')
    dth, rt = timed(x0, args.both_rows, 'thread')
    same = (rw.samples == rt.samples).all(dim=2)
    diff = torch.where(same, (rw.log_p - rt.log_p).abs(), torch.zeros_like(rw.log_p))
    out['both'] = {'rows': args.both_rows, 'wave_s': dw, 'thread_s': dth,
                   'wave_ms_per_step': dw / (args.both_rows - 1) * 1e3,
                   'thread_ms_per_step': dth / (args.both_rows - 1) * 1e3, 'thread_over_wave': dth / dw,
                   'rows_equal': float(same.double().mean()), 'max_abs_diff_log_p_on_equal_rows': float(diff.max()),
                   'max_abs_log_p': float(rt.log_p.abs().max()),
                   'thread_full_run_extrapolated_s': dth / (args.both_rows - 1) * (args.rows - 1)}
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
