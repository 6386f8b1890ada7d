"""Time the histogram pass of marginals() against its yardsticks, per recorded state, at the benchmark's sizes.

For each workload (c2: iso Gaussian 512 x 100 000 fp64; c4: Neal funnel 32 x 1 000 000 fp64; bench.py WORKLOADS), each
bin count (--bins) and each block of K ring slots (--blocks):
  (a) _run(K + 1, ring_slot0=0) alone                -- the iterations and their ring writes
  (b) (a) + the histogram pass over the block        -- DeviceHistogram.accumulate (weight check, decision, pass)
  the histogram pass alone, dwell-weighted and with unit weights, and the pooled moment pass alone
  (DeviceEstimator.accumulate), --inner calls per timed window so that a window is tens of milliseconds, and K
  device-to-device slot copies (mjhmc_ring_copy: read + write).
Host clock around calls that end in a device synchronise (both accumulates read a flag back; _run is followed by
sync()); median of --reps repetitions after one warm-up.
Bytes of a histogram call: K slots read once by the pass, K dwell vectors read twice (check and pass); the flush adds at
most 2 x 8 bytes of integer atomics per bin and workgroup and is not counted.  Its rate is those bytes over its time, the
copy's rate is 2 * slot_bytes over a slot's copy time, and the fraction of the two is reported next to the moment pass's
own (K * slot_bytes over its time), measured in the same job.
The range is the driver's: pooled mean -/+ 8 standard deviations of the block, the quantum 2^(floor(log2(mean weight)) - 24).
--replaced: also time the path this replaces once, sample(K, preserve_order=True) plus np.histogram per dimension, per
recorded state (c2 at K = 8: a 3.3 GB array on the host).
usage: python tools/marginals_bench.py [--only c2,c4] [--bins 64,256] [--blocks 8] [--reps 5] [--inner 10] [--n N] [--replaced]"""
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


def host_histograms(samples, lo, hi, bins):
    """what a caller of sample(preserve_order=True) does next for unit weights: one np.histogram per dimension"""
    return [np.histogram(samples[d].ravel(), bins=bins, range=(lo[d], hi[d]))[0] for d in range(samples.shape[0])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', default='c2,c4')
    ap.add_argument('--bins', default='64,256')
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
            est = dev.estimator(False)
            b = ctypes.c_uint64()
            dev.lib.mjhmc_ring_slot_bytes(dev.handle, ctypes.byref(b))
            slot_bytes = int(b.value)
            Npad = (N + 63) // 64 * 64

            def run():
                smp._run(K + 1, ring_slot0=0)
                dev.sync()

            run()
            est.accumulate(0, K, w_slot0=1)
            W, S1, S2, _, n_states = est.read()
            mean = S1 / W
            sd = np.sqrt(np.maximum(S2 / W - mean * mean, 0.0))
            lo, hi = mean - 8.0 * sd, mean + 8.0 * sd
            q = 2.0 ** (np.floor(np.log2(W / n_states)) - 24)
            base = dict(workload=key, D=D, N=N, block=K, reps=args.reps, inner=args.inner, slot_bytes=slot_bytes)
            base['a_run_ms_per_state'] = 1e3 * timed(run, args.reps) / (K + 1)
            t_mom = timed(repeated(lambda: est.accumulate(0, K, w_slot0=1), args.inner), args.reps) / args.inner
            t_copy = copy_time(dev, K, args.reps, args.inner) / K
            base['moments_alone_ms_per_state'] = 1e3 * t_mom / K
            base['copy_ms_per_slot'] = 1e3 * t_copy
            base['copy_GBps_read_plus_write'] = 2 * slot_bytes / t_copy / 1e9
            base['moments_GBps_read'] = K * slot_bytes / t_mom / 1e9
            base['moments_fraction_of_copy_rate'] = base['moments_GBps_read'] / base['copy_GBps_read_plus_write']
            for bins in [int(v) for v in args.bins.split(',')]:
                rec = dict(base, bins=bins, log2_quantum=int(np.log2(q)))
                hist = dev.histogram(bins, lo, hi, q)

                def run_hist():
                    smp._run(K + 1, ring_slot0=0)
                    hist.accumulate(0, K, w_slot0=1)

                rec['b_run_hist_ms_per_state'] = 1e3 * timed(run_hist, args.reps) / (K + 1)
                hist.reset()
                t_hist = timed(repeated(lambda: hist.accumulate(0, K, w_slot0=1), args.inner), args.reps) / args.inner
                unit = dev.histogram(bins, lo, hi, 1.0)
                t_unit = timed(repeated(lambda: unit.accumulate(0, K), args.inner), args.reps) / args.inner
                rec['out_of_range_max'] = float(np.max((unit.read()[0][:, [0, -1]].sum(axis=1)) / float(unit.read()[3])))
                unit.close()
                rec['hist_alone_ms_per_state'] = 1e3 * t_hist / K
                rec['hist_unit_alone_ms_per_state'] = 1e3 * t_unit / K
                rec['hist_bytes_per_call'] = K * slot_bytes + K * Npad * 8
                rec['hist_GBps'] = rec['hist_bytes_per_call'] / t_hist / 1e9
                rec['hist_fraction_of_copy_rate'] = rec['hist_GBps'] / rec['copy_GBps_read_plus_write']
                rec['hist_unit_fraction_of_copy_rate'] = (K * slot_bytes - K * Npad * 8) / t_unit / 1e9 / rec['copy_GBps_read_plus_write']
                rec['read_ms'] = 1e3 * timed(hist.read, args.reps)
                hist.close()
                print(json.dumps({k: (round(v, 5) if isinstance(v, float) else v) for k, v in rec.items()}), flush=True)
            est.close()
            del smp, dev
            if args.replaced and K == 8:
                smp, _, _ = make_sampler(key, args.n)
                t0 = time.perf_counter()
                samples = smp.sample(K, preserve_order=True)
                t1 = time.perf_counter()
                host_histograms(samples, lo, hi, int(args.bins.split(',')[-1]))
                t2 = time.perf_counter()
                print(json.dumps(dict(workload=key, block=K, bins=int(args.bins.split(',')[-1]),
                                      replaced_sample_ms_per_state=round(1e3 * (t1 - t0) / K, 3),
                                      replaced_numpy_histogram_ms_per_state=round(1e3 * (t2 - t1) / K, 3))), flush=True)
                del smp, samples


if __name__ == '__main__':
    main()
