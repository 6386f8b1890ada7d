"""Time the device estimator against what it replaces, per recorded state, at the benchmark's sizes.

For each workload (c2: iso Gaussian 512 x 100 000 fp64; c3f64: ProductOfT 512 x 100 000 float64 state; c4: Neal funnel
32 x 1 000 000 fp64; bench.py WORKLOADS) and a block of B ring slots:
  (a) _run(B, ring_slot0=0) alone             -- the iterations and their ring writes
  (b) (a) + the moment pass over the block    -- DeviceEstimator.accumulate
  (c) (a) + moment and covariance pass        -- c2 / c3f64 only (D <= 512 and worth a D x D matrix)
  (d) sample(B, resample=True)                -- record B + 1 states, pick columns on the host, download them
Host clock around calls that end in a device synchronise (accumulate reads its flag back; _run is followed by sync());
median of --reps repetitions after one warm-up, (d) included.  The passes alone are (b) - (a) and (c) - (b); they are also
timed directly, --inner calls per timed window so that a window is tens of milliseconds and not a fraction of one.
Yardsticks: a device-to-device copy of the block's slots (mjhmc_ring_copy: read + write, so a read-only pass at the same HBM rate takes
half its time), and the fp64 vector peak for D (D + 16) / 2 * N multiply-adds per slot (upper-triangle 16 x 16 tiles).
usage: python tools/estimator_bench.py [--only c2,c3f64,c4] [--block 8] [--reps 5] [--inner 25] [--n N]"""
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
import bench                                                            # noqa: E402  (WORKLOADS, pot_model, initial_state)
from mjhmc_amd.samplers.markov_jump_hmc import MarkovJumpHMC            # noqa: E402
from mjhmc_amd.misc import distributions as dists                       # noqa: E402

FP64_VECTOR_PEAK = 78.6e12      # MI355X data sheet, flop/s (a multiply-add is two)


def make_sampler(key, n, resample):
    w = dict(bench.WORKLOADS[key])
    N = n or w['N']
    X0 = bench.initial_state(w, N, 0)
    if w['kind'] == 'iso':
        cls, kw = dists.TestGaussian, dict(ndims=w['D'], nbatch=N, sigma=w['params'][0])
    elif w['kind'] == 'pot':
        W, lognu = bench.pot_model(w['D'])
        cls, kw = dists.ProductOfT, dict(ndims=w['D'], nbasis=w['D'], nbatch=N, lognu=lognu, W=W, state_dtype=w['dtype'])
    else:
        cls, kw = dists.Funnel, dict(scale=w['params'][0], nbatch=N, ndims=w['D'])

    class Fixed(cls):
        def gen_init_X(self):
            self.Xinit = X0
    return MarkovJumpHMC(distribution=Fixed(**kw), epsilon=w['eps'], beta=w['beta'], num_leapfrog_steps=w['L'], seed=1,
                         resample=resample), w, N


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def copy_time(dev, B, reps, inner):
    """B device-to-device slot copies (state and dwelling times: the bytes the moment pass reads, read AND written)"""
    def go():
        for _ in range(inner):
            for k in range(B):
                dev.ring_copy(k + 1, k)           # (the live state sits in slot B: never a destination)
        dev.sync()
    return timed(go, reps) / inner


def repeated(fn, inner):
    def go():
        for _ in range(inner):
            fn()
    return go


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', default='c2,c3f64,c4')
    ap.add_argument('--block', type=int, default=8)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--inner', type=int, default=25, help='calls per timed window of the passes alone and of the slot copy')
    ap.add_argument('--n', type=int, default=0, help='particles (default: the workload\'s)')
    args = ap.parse_args()
    B = args.block
    for key in args.only.split(','):
        smp, w, N = make_sampler(key, args.n, resample=False)
        dev = smp._dev
        D = w['D']
        want_cov = D >= 64
        dev.ring_alloc(B + 1)
        est = dev.estimator(False)
        estc = dev.estimator(True) if want_cov else None

        def run():
            smp._run(B + 1, ring_slot0=0)
            dev.sync()

        def run_moments():
            smp._run(B + 1, ring_slot0=0)
            est.accumulate(0, B, w_slot0=1)

        def run_cov():
            smp._run(B + 1, ring_slot0=0)
            estc.accumulate(0, B, w_slot0=1)

        rec = dict(workload=key, D=D, N=N, block=B, reps=args.reps)
        rec['a_run_ms_per_state'] = 1e3 * timed(run, args.reps) / (B + 1)
        rec['b_run_moments_ms_per_state'] = 1e3 * timed(run_moments, args.reps) / (B + 1)
        rec['moments_alone_ms_per_state'] = 1e3 * timed(repeated(lambda: est.accumulate(0, B, w_slot0=1), args.inner), args.reps) / B / args.inner
        if want_cov:
            rec['c_run_moments_cov_ms_per_state'] = 1e3 * timed(run_cov, args.reps) / (B + 1)
            both = 1e3 * timed(repeated(lambda: estc.accumulate(0, B, w_slot0=1), args.inner), args.reps) / B / args.inner
            rec['cov_alone_ms_per_state'] = both - rec['moments_alone_ms_per_state']
            fma = D * (D + 16) / 2.0 * N
            rec['cov_fraction_of_fp64_vector_peak'] = 2 * fma / (rec['cov_alone_ms_per_state'] * 1e-3) / FP64_VECTOR_PEAK
        b = ctypes.c_uint64()
        dev.lib.mjhmc_ring_slot_bytes(dev.handle, ctypes.byref(b))
        rec['slot_bytes'] = int(b.value)
        t_copy = copy_time(dev, B, args.reps, args.inner) / B
        rec['copy_ms_per_slot'] = 1e3 * t_copy
        rec['copy_GBps_read_plus_write'] = 2 * b.value / t_copy / 1e9
        rec['moments_GBps_read'] = b.value / (rec['moments_alone_ms_per_state'] * 1e-3) / 1e9
        rec['moments_fraction_of_copy_rate'] = rec['moments_GBps_read'] / rec['copy_GBps_read_plus_write']
        est.close()
        if estc is not None:
            estc.close()
        del smp, dev
        # (d) on a fresh sampler: the resampling path allocates its own ring
        smp, _, _ = make_sampler(key, args.n, resample=True)
        np.random.seed(0)
        rec['d_sample_resample_ms_per_state'] = 1e3 * timed(lambda: smp.sample(B), args.reps) / (B + 1)
        del smp
        print(json.dumps({k: (round(v, 5) if isinstance(v, float) else v) for k, v in rec.items()}), flush=True)


if __name__ == '__main__':
    main()
