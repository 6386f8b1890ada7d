"""Time the time-grid pass of paths() against its yardsticks, per recorded state, at the benchmark's sizes.

For each workload (c2: iso Gaussian 512 x 100 000 fp64; c4: Neal funnel 32 x 1 000 000 fp64; bench.py WORKLOADS) and each
block of K ring slots (--blocks), after one recorded run of K + 1 iterations and with dt = the block's mean holding time:
  the pass alone       DeviceTimeGrid.accumulate(0, K, w_slot0=1) into a grid of K slots.  A grid fills up, so every timed
                       call is reset() + accumulate() and the time of reset() alone (the memset of the grid) is taken off
  the chain pass alone DeviceChainStats.accumulate over the same block (csrc/chainstats.hip)
  K device-to-device slot copies (mjhmc_ring_copy: read + write)
--inner calls per timed window; host clock around calls that end in a device synchronise (both accumulates read a flag
back; the copies and reset() are followed by sync()); median of --reps repetitions after one warm-up.
Bytes of a time-grid call: K slots read once, K dwell vectors read twice (check and pass), the emitted rows written
(counted from the cursors after the call), 24 bytes of clocks and cursors per chain.  Bytes of a chain-pass call: K slots
and K dwell vectors (twice), the chains' sums read and written once.  Each rate is its bytes over its time, the copy's is
2 * slot_bytes over a slot's copy time, and both fractions of the copy rate are reported.
Then the drivers, on fresh samplers: paths(4 K, block=K) and expectations(4 K, block=K) per recorded state.
--replaced: also time the path this replaces once, calculate_autocorrelation on the default (resampling) sampler, which
calls sample(1) once per step with a host draw and a download each, per step.
usage: python tools/timegrid_bench.py [--only c2,c4] [--blocks 8] [--reps 5] [--inner 10] [--n N] [--replaced]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from chainstats_bench import make_sampler, timed, repeated, copy_time   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', default='c2,c4')
    ap.add_argument('--blocks', default='8')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--inner', type=int, default=10, help='calls per timed window of the passes alone and of the slot copy')
    ap.add_argument('--n', type=int, default=0, help='particles (default: the workload\'s)')
    ap.add_argument('--replaced', action='store_true')
    args = ap.parse_args()
    for key in args.only.split(','):
        for K in [int(b) for b in args.blocks.split(',')]:
            smp, w, N = make_sampler(key, args.n)
            dev = smp._dev
            D = w['D']
            dev.ring_alloc(K + 1)
            slot_bytes = dev.ring_slot_bytes()
            Npad = (N + 63) // 64 * 64
            state_bytes = slot_bytes - 8 * Npad
            row_bytes = state_bytes // Npad
            smp._run(K + 1, ring_slot0=0)
            dev.sync()
            est = dev.estimator(False)
            est.accumulate(0, K, w_slot0=1)
            W, _, _, _, n_states = est.read()
            est.close()
            dt = W / n_states
            rec = dict(workload=key, D=D, N=N, block=K, reps=args.reps, inner=args.inner, slot_bytes=slot_bytes, dt=dt)
            tg = dev.time_grid(K, dt)

            def reset_only():
                tg.reset()
                dev.sync()

            def reset_and_pass():
                tg.reset()
                tg.accumulate(0, K, w_slot0=1)

            t_reset = timed(repeated(reset_only, args.inner), args.reps) / args.inner
            t_both = timed(repeated(reset_and_pass, args.inner), args.reps) / args.inner
            t_pass = t_both - t_reset
            _, j = tg.read_clocks()
            covered, max_filled = tg.progress()
            emitted = int(j.astype(np.int64).sum())
            tg.close()
            cs = dev.chain_stats(1)
            t_chain = timed(repeated(lambda: cs.accumulate(0, K, w_slot0=1), args.inner), args.reps) / args.inner
            cs.close()
            t_copy = copy_time(dev, K, args.reps, args.inner) / K
            rec['copy_ms_per_slot'] = 1e3 * t_copy
            rec['copy_GBps_read_plus_write'] = 2 * slot_bytes / t_copy / 1e9
            rec['grid_reset_ms'] = 1e3 * t_reset
            rec['pass_alone_ms_per_state'] = 1e3 * t_pass / K
            rec['emitted_rows_per_state'] = emitted / float(K * N)
            rec['covered'], rec['max_filled'] = covered, max_filled
            rec['pass_bytes_per_call'] = K * state_bytes + 2 * K * Npad * 8 + emitted * row_bytes + 24 * N
            rec['pass_GBps'] = rec['pass_bytes_per_call'] / t_pass / 1e9
            rec['pass_fraction_of_copy_rate'] = rec['pass_GBps'] / rec['copy_GBps_read_plus_write']
            rec['chain_alone_ms_per_state'] = 1e3 * t_chain / K
            # (float64 state: the sums a1, a2 have the state's row layout)
            rec['chain_bytes_per_call'] = K * state_bytes + 2 * K * Npad * 8 + 2 * (2 * state_bytes + Npad * 8)
            rec['chain_GBps'] = rec['chain_bytes_per_call'] / t_chain / 1e9
            rec['chain_fraction_of_copy_rate'] = rec['chain_GBps'] / rec['copy_GBps_read_plus_write']
            del smp, dev
            for name in ('paths', 'expectations'):
                s2, _, _ = make_sampler(key, args.n)
                n_iter = 4 * K
                t0 = time.perf_counter()
                if name == 'paths':
                    p = s2.paths(n_iter, block=K)
                    rec['paths_covered_of_n_grid'] = '%d/%d' % (p.covered, p.n_grid)
                    p.close()
                else:
                    s2.expectations(n_iter, block=K, shift=np.zeros(D))
                s2._dev.sync()
                rec[name + '_ms_per_state'] = 1e3 * (time.perf_counter() - t0) / n_iter
                del s2
            print(json.dumps({k: (round(v, 5) if isinstance(v, float) else v) for k, v in rec.items()}), flush=True)
            if args.replaced and K == 8:
                from mjhmc_amd.misc.autocor import calculate_autocorrelation
                from mjhmc_amd.samplers.markov_jump_hmc import MarkovJumpHMC
                s3, w3, _ = make_sampler(key, args.n)
                d3 = s3.distribution
                del s3
                t0 = time.perf_counter()
                calculate_autocorrelation(MarkovJumpHMC, d3, num_steps=K, epsilon=w3['eps'], beta=w3['beta'],
                                          num_leapfrog_steps=w3['L'], seed=1)
                print(json.dumps(dict(workload=key, steps=K,
                                      replaced_resampling_autocor_ms_per_step=round(1e3 * (time.perf_counter() - t0) / K, 3))),
                      flush=True)


if __name__ == '__main__':
    main()
