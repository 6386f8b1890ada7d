"""Time the evaluate pass of the device functionals against its yardsticks, per recorded state, at the benchmark's sizes.

For each workload (c2: iso Gaussian 512 x 100 000 fp64; c4: Neal funnel 32 x 1 000 000 fp64; bench.py WORKLOADS), each
block of K ring slots (--blocks) and two functional sets --
  small: J = 1, K = 1     stat x * x, value S[0]
  large: J = 4, K = 8     stats x * x, x, x > 0 ? 1 : 0, d == 0 ? x : 0; values: the four sums, a scaled radius, a product,
                          an indicator and a ratio
--
  the evaluate pass alone (DeviceFunctionals.evaluate: one launch, one flag read back), the pooled moment pass alone on the
  sample ring (DeviceEstimator.accumulate) and K device-to-device slot copies (mjhmc_ring_copy: read + write), --inner calls
  per timed window so that a window is tens of milliseconds;
  expectations(n, of=F) and expectations(n) end to end on twin samplers, per recorded state.
Host clock around calls that end in a device synchronise; median of --reps repetitions after one warm-up.
Bytes of an evaluate call: K state matrices read once, K derived slots (Npad * pitchK * 8 bytes each) written once.  Its rate is
those bytes over its time, the copy's rate is 2 * slot_bytes over a slot's copy time, and the fraction of the two is
reported next to the moment pass's own (K * slot_bytes over its time), measured in the same job.
--replaced: also time the path this replaces once, sample(K, preserve_order=True) plus the same functionals in NumPy.
usage: python tools/functionals_bench.py [--only c2,c4] [--blocks 8] [--reps 5] [--inner 10] [--n N] [--states 16] [--replaced]"""
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

SETS = {
    'small_J1_K1': (['x * x'], ['S[0]'], []),
    'large_J4_K8': (['x * x', 'x', 'x > 0.0 ? 1.0 : 0.0', 'd == 0 ? x : 0.0'],
                    ['S[0]', 'S[1]', 'S[2]', 'S[3]', 'S[0] / (p[0] * p[0])', 'S[1] * S[1]', 'S[0] > p[1] ? 1.0 : 0.0',
                     'S[3] / (S[2] + 1.0)'], [1.3, 2.0]),
}


def host_functionals(samples, params):
    """the large set in NumPy on the (D, N, n) array of sample(preserve_order=True)"""
    S0, S1 = (samples * samples).sum(axis=0), samples.sum(axis=0)
    S2, S3 = (samples > 0.0).sum(axis=0).astype(np.float64), samples[0]
    return np.stack([S0, S1, S2, S3, S0 / (params[0] * params[0]), S1 * S1, np.where(S0 > params[1], 1.0, 0.0), S3 / (S2 + 1.0)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', default='c2,c4')
    ap.add_argument('--blocks', default='8')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--inner', type=int, default=10, help='calls per timed window of the passes alone and of the slot copy')
    ap.add_argument('--n', type=int, default=0, help='particles (default: the workload\'s)')
    ap.add_argument('--states', type=int, default=16, help='recorded states of the end-to-end expectations() runs')
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
            slot_bytes = int(b.value)                                 # the state matrix and its dwell vector: what a copy moves
            state_bytes = slot_bytes - (N + 63) // 64 * 64 * 8        # the state matrix alone: what the evaluate pass reads
            smp._run(K + 1, ring_slot0=0)
            dev.sync()
            base = dict(workload=key, D=D, N=N, block=K, reps=args.reps, inner=args.inner, slot_bytes=slot_bytes, state_bytes=state_bytes)
            est.accumulate(0, K, w_slot0=1)
            t_mom = timed(repeated(lambda: est.accumulate(0, K, w_slot0=1), args.inner), args.reps) / args.inner
            t_copy = copy_time(dev, K, args.reps, args.inner) / K
            base['moments_alone_ms_per_state'] = 1e3 * t_mom / K
            base['copy_ms_per_slot'] = 1e3 * t_copy
            base['copy_GBps_read_plus_write'] = 2 * slot_bytes / t_copy / 1e9
            base['moments_GBps_read'] = K * slot_bytes / t_mom / 1e9
            base['moments_fraction_of_copy_rate'] = base['moments_GBps_read'] / base['copy_GBps_read_plus_write']
            for name, (stats, values, params) in sorted(SETS.items()):
                rec = dict(base, functionals=name)
                fn = dev.functionals(values, stats, params)
                fn.ring_alloc(K)
                fn.evaluate(0, K, 0)
                t_eval = timed(repeated(lambda: fn.evaluate(0, K, 0), args.inner), args.reps) / args.inner
                rec['derived_slot_bytes'] = fn.slot_bytes
                rec['evaluate_alone_ms_per_state'] = 1e3 * t_eval / K
                rec['evaluate_bytes_per_call'] = K * (state_bytes + fn.slot_bytes)
                rec['evaluate_GBps'] = rec['evaluate_bytes_per_call'] / t_eval / 1e9
                rec['evaluate_fraction_of_copy_rate'] = rec['evaluate_GBps'] / rec['copy_GBps_read_plus_write']
                dest = fn.estimator(False)
                dest.accumulate(0, K, w_slot0=1)
                t_dmom = timed(repeated(lambda: dest.accumulate(0, K, w_slot0=1), args.inner), args.reps) / args.inner
                rec['derived_moments_alone_ms_per_state'] = 1e3 * t_dmom / K
                dest.close()
                fn.close()
                print(json.dumps({k: (round(v, 5) if isinstance(v, float) else v) for k, v in rec.items()}), flush=True)
            t_copy2 = copy_time(dev, K, args.reps, args.inner) / K     # the copy again: the job's own spread of the yardstick
            print(json.dumps(dict(workload=key, block=K, copy_GBps_read_plus_write_again=round(2 * slot_bytes / t_copy2 / 1e9, 2))),
                  flush=True)
            est.close()
            del smp, dev
            # end to end, twin samplers: expectations(n) and expectations(n, of=F), blocks of K
            n = args.states
            rec = dict(workload=key, block=K, states=n)
            for name in [None] + sorted(SETS):
                smp, _, _ = make_sampler(key, args.n)
                F = None if name is None else smp.functionals(SETS[name][1], SETS[name][0], SETS[name][2])
                shift = np.zeros(D if F is None else F.n_values)
                smp.expectations(K, block=K, shift=shift, of=F)          # warm-up: ring, kernels, the hipRTC compile
                smp._dev.sync()
                t0 = time.perf_counter()
                smp.expectations(n, block=K, shift=shift, of=F)
                rec['expectations_%s_ms_per_state' % (name or 'plain')] = round(1e3 * (time.perf_counter() - t0) / n, 4)
                del smp
            print(json.dumps(rec), flush=True)
            if args.replaced and K == 8:
                smp, _, _ = make_sampler(key, args.n)
                t0 = time.perf_counter()
                samples = smp.sample(K, preserve_order=True)
                t1 = time.perf_counter()
                g = host_functionals(samples, SETS['large_J4_K8'][2])
                g.mean(axis=(1, 2))
                t2 = time.perf_counter()
                print(json.dumps(dict(workload=key, block=K, replaced_sample_ms_per_state=round(1e3 * (t1 - t0) / K, 3),
                                      replaced_numpy_functionals_ms_per_state=round(1e3 * (t2 - t1) / K, 3))), flush=True)
                del smp, samples, g


if __name__ == '__main__':
    main()
