"""Time the per-chain pass of the convergence diagnostics against its yardsticks, per recorded state, at the benchmark's sizes.

For each workload (c2: iso Gaussian 512 x 100 000 fp64; c4: Neal funnel 32 x 1 000 000 fp64; bench.py WORKLOADS) and
each block of B ring slots (--blocks; 0 = what the device holds next to the split sums, at most --max-block):
  (a) _run(B + 1, ring_slot0=0) alone               -- the iterations and their ring writes
  (b) (a) + the chain pass over the block           -- DeviceChainStats.accumulate
  the chain pass alone and the pooled moment pass alone (DeviceEstimator.accumulate), --inner calls per timed window so
  that a window is tens of milliseconds, and B device-to-device slot copies (mjhmc_ring_copy: read + write).
Host clock around calls that end in a device synchronise (both accumulates read a flag back; _run is followed by
sync()); median of --reps repetitions after one warm-up.
Bytes of a chain pass are known exactly: B slots + B dwell vectors read, a0, a1, a2 of the part read and written once
= B * slot_bytes + 2 * (2 * pitch + 1) * Npad * 8; its rate is those bytes over its time, the copy's rate is 2 *
slot_bytes over a slot's copy time, and the fraction of the two is reported next to the moment pass's own
(B * slot_bytes over its time), measured in the same job.
--replaced: also time the path this replaces once, sample(B, preserve_order=True) plus the NumPy reduction to the
same per-chain sums and their fold, per recorded state (c2 at B = 8: a 3.3 GB array on the host).
usage: python tools/chainstats_bench.py [--only c2,c4] [--blocks 1,8,0] [--reps 5] [--inner 10] [--n N] [--replaced]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench                                                            # noqa: E402  (WORKLOADS, initial_state)
from mjhmc_amd.samplers.markov_jump_hmc import MarkovJumpHMC            # noqa: E402
from mjhmc_amd.misc import distributions as dists                       # noqa: E402


def make_sampler(key, n):
    w = dict(bench.WORKLOADS[key])
    N = n or w['N']
    X0 = bench.initial_state(w, N, 0)
    if w['kind'] == 'iso':
        cls, kw = dists.TestGaussian, dict(ndims=w['D'], nbatch=N, sigma=w['params'][0])
    else:
        cls, kw = dists.Funnel, dict(scale=w['params'][0], nbatch=N, ndims=w['D'])

    class Fixed(cls):
        def gen_init_X(self):
            self.Xinit = X0
    return MarkovJumpHMC(distribution=Fixed(**kw), epsilon=w['eps'], beta=w['beta'], num_leapfrog_steps=w['L'], seed=1,
                         resample=False), w, N


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def repeated(fn, inner):
    def go():
        for _ in range(inner):
            fn()
    return go


def copy_time(dev, B, reps, inner):
    def go():
        for _ in range(inner):
            for k in range(B):
                dev.ring_copy(k + 1, k)           # (the live state sits in slot B: never a destination)
        dev.sync()
    return timed(go, reps) / inner


def host_reduction(samples):
    """what a caller of sample(preserve_order=True) does next: per-chain sums and their fold, (ndims, nbatch, n) in"""
    m = samples.mean(axis=2)
    v = (samples * samples).mean(axis=2) - m * m
    return m.sum(axis=1), (m * m).sum(axis=1), v.sum(axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', default='c2,c4')
    ap.add_argument('--blocks', default='1,8,0')
    ap.add_argument('--max-block', type=int, default=64)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--inner', type=int, default=10, help='calls per timed window of the passes alone and of the slot copy')
    ap.add_argument('--n', type=int, default=0, help='particles (default: the workload\'s)')
    ap.add_argument('--replaced', action='store_true')
    args = ap.parse_args()
    for key in args.only.split(','):
        for B in [int(b) for b in args.blocks.split(',')]:
            smp, w, N = make_sampler(key, args.n)
            dev = smp._dev
            D = w['D']
            dev.ring_alloc(2)
            probe = dev.chain_stats(2)           # (the split sums take their memory before the ring is sized)
            if B == 0:
                B = min(args.max_block, dev.ring_budget_slots(args.max_block + 1, staging=False) - 1)
            probe.close()
            dev.ring_alloc(B + 1)
            cs = dev.chain_stats(2)
            est = dev.estimator(False)
            b = ctypes.c_uint64()
            dev.lib.mjhmc_ring_slot_bytes(dev.handle, ctypes.byref(b))
            slot_bytes = int(b.value)
            Npad = (N + 63) // 64 * 64
            pitch = (slot_bytes // Npad - 8) // 8           # (float64 state: a row of pitch doubles + the dwelling time)
            acc_bytes = (2 * pitch + 1) * Npad * 8

            def run():
                smp._run(B + 1, ring_slot0=0)
                dev.sync()

            def run_chain():
                smp._run(B + 1, ring_slot0=0)
                cs.accumulate(0, B, w_slot0=1)

            rec = dict(workload=key, D=D, N=N, block=B, reps=args.reps, inner=args.inner, slot_bytes=slot_bytes,
                       chain_sums_bytes_per_part=acc_bytes)
            rec['a_run_ms_per_state'] = 1e3 * timed(run, args.reps) / (B + 1)
            rec['b_run_chain_ms_per_state'] = 1e3 * timed(run_chain, args.reps) / (B + 1)
            t_chain = timed(repeated(lambda: cs.accumulate(0, B, w_slot0=1), args.inner), args.reps) / args.inner
            t_mom = timed(repeated(lambda: est.accumulate(0, B, w_slot0=1), args.inner), args.reps) / args.inner
            t_copy = copy_time(dev, B, args.reps, args.inner) / B
            rec['chain_alone_ms_per_state'] = 1e3 * t_chain / B
            rec['moments_alone_ms_per_state'] = 1e3 * t_mom / B
            rec['copy_ms_per_slot'] = 1e3 * t_copy
            rec['copy_GBps_read_plus_write'] = 2 * slot_bytes / t_copy / 1e9
            rec['chain_bytes_per_call'] = B * slot_bytes + 2 * acc_bytes
            rec['chain_GBps'] = rec['chain_bytes_per_call'] / t_chain / 1e9
            rec['chain_fraction_of_copy_rate'] = rec['chain_GBps'] / rec['copy_GBps_read_plus_write']
            rec['moments_GBps_read'] = B * slot_bytes / t_mom / 1e9
            rec['moments_fraction_of_copy_rate'] = rec['moments_GBps_read'] / rec['copy_GBps_read_plus_write']
            rec['fold_ms'] = 1e3 * timed(lambda: cs.read(0), args.reps)
            cs.close()
            est.close()
            del smp, dev
            if args.replaced and B == 8:
                smp, _, _ = make_sampler(key, args.n)
                t0 = time.perf_counter()
                samples = smp.sample(B, preserve_order=True)
                t1 = time.perf_counter()
                host_reduction(samples)
                t2 = time.perf_counter()
                rec['replaced_sample_ms_per_state'] = 1e3 * (t1 - t0) / B
                rec['replaced_numpy_ms_per_state'] = 1e3 * (t2 - t1) / B
                del smp, samples
            print(json.dumps({k: (round(v, 5) if isinstance(v, float) else v) for k, v in rec.items()}), flush=True)


if __name__ == '__main__':
    main()
