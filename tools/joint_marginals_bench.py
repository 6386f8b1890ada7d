"""Time the pair-histogram pass of joint_marginals() against its yardsticks, per recorded state, at the benchmark's sizes.

For each workload (c2: iso Gaussian 512 x 100 000 fp64; c4: Neal funnel 32 x 1 000 000 fp64; bench.py WORKLOADS), each
(P, B) of --cases and a block of K ring slots (--block):
  the pair pass alone, dwell-weighted and with unit weights -- DevicePairHistogram.accumulate (weight check, decision,
  pass), --inner calls per timed window so that a window is tens of milliseconds;
  (a) _run(K + 1, ring_slot0=0) alone and (b) (a) + the pair pass over the block;
  K device-to-device slot copies (mjhmc_ring_copy: read + write) in the same job.
Host clock around calls that end in a device synchronise (accumulate reads a flag back; _run is followed by sync());
median of --reps repetitions after one warm-up.
Bytes: the pass loads 2 P elements and one weight per state, each from a cache line of its own in the worst case, so
`pair_lines_bytes` = K * N * (min(2 P * 64, row bytes) + 8) is an upper bound of what it fetches and `slot_bytes` * K what
a full pass over the ring would; both are printed next to the copy's measured rate.
The pairs are (0, 1), (0, 2), ... (x_0 against x_k: the funnel's diagnostic); the range is the driver's, pooled mean -/+ 8
standard deviations of the block, the quantum 2^(floor(log2(mean weight)) - 24).
--replaced: also time the host route once, sample(K, preserve_order=True) plus np.histogram2d with the dwell weights per
pair, per recorded state.
usage: python tools/joint_marginals_bench.py [--only c2,c4] [--cases 1x64,8x64,8x128] [--block 8] [--reps 5] [--inner 10] [--n N] [--replaced]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from chainstats_bench import make_sampler, timed, repeated, copy_time   # noqa: E402


def host_joint(samples, weights, pairs, lo, hi, bins):
    """what a caller of sample(preserve_order=True) does next: one np.histogram2d per pair, weighted by the dwell times.
    samples (D, N, K), weights (N, K)"""
    w = weights.ravel()
    return [np.histogram2d(samples[i].ravel(), samples[j].ravel(), bins=bins, range=((lo[i], hi[i]), (lo[j], hi[j])), weights=w)[0]
            for i, j in pairs]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', default='c2,c4')
    ap.add_argument('--cases', default='1x64,8x64,8x128', help='P x B, comma separated')
    ap.add_argument('--block', type=int, default=8)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--inner', type=int, default=10, help='calls per timed window of the pass alone and of the slot copy')
    ap.add_argument('--n', type=int, default=0, help='particles (default: the workload\'s)')
    ap.add_argument('--replaced', action='store_true')
    args = ap.parse_args()
    K = args.block
    cases = [tuple(int(v) for v in c.split('x')) for c in args.cases.split(',')]
    for key in args.only.split(','):
        smp, w, N = make_sampler(key, args.n)
        dev = smp._dev
        D = w['D']
        dev.ring_alloc(K + 1)
        est = dev.estimator(False)
        b = ctypes.c_uint64()
        dev.lib.mjhmc_ring_slot_bytes(dev.handle, ctypes.byref(b))
        slot_bytes = int(b.value)
        row_bytes = slot_bytes // ((N + 63) // 64 * 64)

        def run():
            smp._run(K + 1, ring_slot0=0)
            dev.sync()

        run()
        est.accumulate(0, K, w_slot0=1)
        W, S1, S2, _, n_states = est.read()
        est.close()
        mean = S1 / W
        sd = np.sqrt(np.maximum(S2 / W - mean * mean, 0.0))
        lo, hi = mean - 8.0 * sd, mean + 8.0 * sd
        q = 2.0 ** (np.floor(np.log2(W / n_states)) - 24)
        base = dict(workload=key, D=D, N=N, block=K, reps=args.reps, inner=args.inner, slot_bytes=slot_bytes)
        base['a_run_ms_per_state'] = 1e3 * timed(run, args.reps) / (K + 1)
        t_copy = copy_time(dev, K, args.reps, args.inner) / K
        base['copy_ms_per_slot'] = 1e3 * t_copy
        base['copy_GBps_read_plus_write'] = 2 * slot_bytes / t_copy / 1e9
        for P, bins in cases:
            pairs = np.array([(0, 1 + k % (D - 1)) for k in range(P)])
            rec = dict(base, pairs=P, bins=bins, log2_quantum=int(np.log2(q)))
            hist = dev.pair_histogram(pairs, bins, lo[pairs], hi[pairs], q)

            def run_hist():
                smp._run(K + 1, ring_slot0=0)
                hist.accumulate(0, K, w_slot0=1)

            rec['b_run_pairhist_ms_per_state'] = 1e3 * timed(run_hist, args.reps) / (K + 1)
            hist.reset()
            t_hist = timed(repeated(lambda: hist.accumulate(0, K, w_slot0=1), args.inner), args.reps) / args.inner
            unit = dev.pair_histogram(pairs, bins, lo[pairs], hi[pairs], 1.0)
            t_unit = timed(repeated(lambda: unit.accumulate(0, K), args.inner), args.reps) / args.inner
            unit.close()
            rec['pairhist_alone_ms_per_state'] = 1e3 * t_hist / K
            rec['pairhist_unit_alone_ms_per_state'] = 1e3 * t_unit / K
            rec['pairhist_over_copy'] = t_hist / K / t_copy
            rec['pair_lines_bytes'] = K * N * (min(2 * P * 64, row_bytes) + 8)
            rec['pair_lines_GBps_upper'] = rec['pair_lines_bytes'] / t_hist / 1e9
            rec['full_pass_bytes'] = K * slot_bytes
            rec['read_ms'] = 1e3 * timed(hist.read, args.reps)
            hist.close()
            print(json.dumps({k: (round(v, 5) if isinstance(v, float) else v) for k, v in rec.items()}), flush=True)
        del smp, dev
        if args.replaced:
            P, bins = cases[-1]
            pairs = [(0, 1 + k % (D - 1)) for k in range(P)]
            smp, _, _ = make_sampler(key, args.n)
            t0 = time.perf_counter()
            samples = smp.sample(K + 1, preserve_order=True)
            t1 = time.perf_counter()
            weights = np.ones(samples.shape[1:])              # (the dwell times of the run would stand here: same cost)
            host_joint(samples, weights, pairs, lo, hi, bins)
            t2 = time.perf_counter()
            print(json.dumps(dict(workload=key, block=K, pairs=P, bins=bins,
                                  replaced_sample_ms_per_state=round(1e3 * (t1 - t0) / (K + 1), 3),
                                  replaced_numpy_histogram2d_ms_per_state=round(1e3 * (t2 - t1) / (K + 1), 3))), flush=True)
            del smp, samples


if __name__ == '__main__':
    main()
