"""Time the linear-projections pass (csrc/projections.hpp) against its yardsticks, per recorded state, at the benchmark's sizes.

For each workload (c2: iso Gaussian 512 x 100 000 fp64; c4: Neal funnel 32 x 1 000 000 fp64; bench.py WORKLOADS), blocks of
8 ring slots (--block) and K in {1, 8, 64, 512} random directions (K capped at ndims on c4), in ONE job:
  the projections pass alone (DeviceFunctionals.evaluate of sampler.projections(A, b): one launch, one flag read back);
  8 device-to-device slot copies (mjhmc_ring_copy: read + write);
  for K <= 8, the functionals pass that states the same projections as stats p[j * D + d] * x, values S[j];
the three are timed in alternation, --rounds rounds after one warm-up round, --inner calls per timed window (host clock
around calls that end in a device synchronise); the median and the spread (min .. max over the rounds) are printed.
Bytes of a projections call: the state matrices read once, the derived slots (Npad * pitchK * 8 bytes each) written once;
its rate is those bytes over its time next to the copy's (2 * slot_bytes over a slot's copy time).  Float64 instructions: 2 *
N * D * K per state (a rounded product and a rounded sum, nothing fused), over the time.
--replaced: also the NumPy path once per workload -- sample(8, preserve_order=True), then A @ X per recorded state.
usage: python tools/projections_bench.py [--only c2,c4] [--ks 1,8,64,512] [--block 8] [--rounds 5] [--inner 4] [--n N] [--replaced]"""
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
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from chainstats_bench import make_sampler   # noqa: E402


def window(fn, inner, dev):
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    dev.sync()
    return (time.perf_counter() - t0) / inner


def spread(ts, scale):
    return dict(median=round(scale * statistics.median(ts), 5), min=round(scale * min(ts), 5), max=round(scale * max(ts), 5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', default='c2,c4')
    ap.add_argument('--ks', default='1,8,64,512')
    ap.add_argument('--block', type=int, default=8)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--inner', type=int, default=4, help='calls per timed window')
    ap.add_argument('--n', type=int, default=0, help='particles (default: the workload\'s)')
    ap.add_argument('--replaced', action='store_true')
    args = ap.parse_args()
    B = args.block
    for key in [k for k in args.only.split(',') if k]:
        smp, w, N = make_sampler(key, args.n)
        dev, D = smp._dev, w['D']
        dev.ring_alloc(B + 1)
        smp._run(B + 1, ring_slot0=0)
        dev.sync()
        b = ctypes.c_uint64()
        dev.lib.mjhmc_ring_slot_bytes(dev.handle, ctypes.byref(b))
        slot_bytes = int(b.value)                                 # the state matrix and its dwell vector: what a copy moves
        Npad = (N + 63) // 64 * 64
        state_bytes = slot_bytes - Npad * 8                       # the state matrix alone: what the pass reads
        rs = np.random.RandomState(0)

        def copies():
            for k in range(B):
                dev.ring_copy(k + 1, k)                           # (the live state sits in slot B: never a destination)

        for K in sorted(set(min(int(k), D) for k in args.ks.split(','))):
            A, bias = rs.randn(K, D) / np.sqrt(D), rs.randn(K)
            fn = dev.projections(A, bias)
            fn.ring_alloc(B)
            passes = [('projections', lambda: fn.evaluate(0, B, 0)), ('copy', copies)]
            fe = None
            if K <= 8:
                fe = dev.functionals(['S[%d] + p[%d]' % (j, K * D + j) for j in range(K)],
                                     ['p[%d + d] * x' % (j * D) for j in range(K)], np.concatenate([A.ravel(), bias]))
                fe.ring_alloc(B)
                passes.append(('functionals', lambda: fe.evaluate(0, B, 0)))
            times = dict((name, []) for name, _ in passes)
            for r in range(args.rounds + 1):                       # (round 0 warms up: code objects, the hipRTC compile)
                for name, call in passes:
                    t = window(call, args.inner, dev)
                    if r:
                        times[name].append(t)
            t_proj, t_copy = statistics.median(times['projections']), statistics.median(times['copy']) / B
            rec = dict(workload=key, D=D, N=N, K=K, block=B, rounds=args.rounds, inner=args.inner, slot_bytes=slot_bytes,
                       derived_slot_bytes=fn.slot_bytes,
                       projections_ms_per_state=spread(times['projections'], 1e3 / B),
                       copy_ms_per_slot=spread(times['copy'], 1e3 / B),
                       projections_GBps=round(B * (state_bytes + fn.slot_bytes) / t_proj / 1e9, 1),
                       copy_GBps_read_plus_write=round(2 * slot_bytes / t_copy / 1e9, 1),
                       projections_f64_Tinstr_per_s=round(2.0 * B * N * D * K / t_proj / 1e12, 3))
            rec['projections_over_copy_time'] = round(t_proj / B / t_copy, 3)
            if fe is not None:
                rec['functionals_ms_per_state'] = spread(times['functionals'], 1e3 / B)
                rec['projections_over_functionals_time'] = round(t_proj / statistics.median(times['functionals']), 3)
                # the two passes state the same numbers in different summation orders
                got, ref = fn.read(0, 1), fe.read(0, 1)
                rec['max_abs_difference_to_functionals'] = float(np.max(np.abs(got - ref)))
                fe.close()
            print(json.dumps(rec), flush=True)
            fn.close()
        del smp, dev
        if args.replaced:
            smp, _, _ = make_sampler(key, args.n)
            A = np.random.RandomState(0).randn(min(64, D), D) / np.sqrt(D)
            t0 = time.perf_counter()
            samples = smp.sample(B, preserve_order=True)             # (D, N, B)
            t1 = time.perf_counter()
            for k in range(B):
                A.dot(samples[:, :, k])
            t2 = time.perf_counter()
            print(json.dumps(dict(workload=key, block=B, K=A.shape[0], replaced_sample_ms_per_state=round(1e3 * (t1 - t0) / B, 3),
                                  replaced_numpy_matmul_ms_per_state=round(1e3 * (t2 - t1) / B, 3))), flush=True)
            del smp, samples


if __name__ == '__main__':
    main()
