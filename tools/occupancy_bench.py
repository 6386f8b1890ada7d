"""Time the occupancy passes (csrc/occupancy.hip, csrc/occupancy.hpp) against their yardsticks, per recorded state, at the
benchmark's sizes.

For each workload (c2: iso Gaussian 512 x 100 000 fp64; c4: Neal funnel 32 x 1 000 000 fp64; bench.py WORKLOADS), blocks of
8 ring slots (--block) and M in {2, 8, 64} random centres, in ONE job, on the test build of the library (the two passes are
launched apart there, mjhmc_test_occupancy_part; same kernels):
  the label pass alone (occ_label_kernel: the block's states read once, one byte per state written);
  the count pass alone (occ_count_kernel over the block's labels and holding times);
  a whole accumulate call (the weight check and decision, both passes, one flag read back);
  8 device-to-device slot copies (mjhmc_ring_copy: read + write);
  the projections pass at K = M (DeviceFunctionals.evaluate of sampler.projections(A): the same tile, two float64
  instructions per (p, k, d) where the label pass issues three);
timed in alternation, --rounds rounds after one warm-up round, --inner calls per timed window (host clock around calls that
end in a device synchronise); the median and the spread (min .. max over the rounds) are printed, with the ratio of the
label pass to the projections pass (1.5 is the instruction count's) and to a slot copy.
usage: python tools/occupancy_bench.py [--only c2,c4] [--ms 2,8,64] [--block 8] [--rounds 5] [--inner 4] [--n N]"""
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
from energy_observables_bench import hooks_device   # noqa: E402


def window(fn, inner, dev):
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    dev.sync()
    return (time.perf_counter() - t0) / inner


def spread(ts, scale):
    return dict(median=round(scale * statistics.median(ts), 5), min=round(scale * min(ts), 5), max=round(scale * max(ts), 5))


def main():
    from mjhmc_amd import engine
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', default='c2,c4')
    ap.add_argument('--ms', default='2,8,64')
    ap.add_argument('--block', type=int, default=8)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--inner', type=int, default=4, help='calls per timed window')
    ap.add_argument('--n', type=int, default=0, help='particles (default: the workload\'s)')
    args = ap.parse_args()
    B = args.block
    for key in [k for k in args.only.split(',') if k]:
        ctx, dev, w, N = hooks_device(key, args.n, B + 1)
        lib, D = ctx.lib, w['D']
        b = ctypes.c_uint64()
        lib.mjhmc_ring_slot_bytes(dev.handle, ctypes.byref(b))
        slot_bytes = int(b.value)                                 # the state matrix and its dwell vector: what a copy moves
        Npad = (N + 63) // 64 * 64
        state_bytes = slot_bytes - Npad * 8                       # the state matrix alone: what the label pass reads
        mean_w = float(dev.ring_read_dwell(1, 1).mean())
        q = 2.0 ** (np.floor(np.log2(mean_w)) - 24)
        rs = np.random.RandomState(0)
        scale = np.sqrt(np.mean(dev.ring_read(0, 1) ** 2))

        def copies():
            for k in range(B):
                dev.ring_copy(k + 1, k)                           # (the live state sits in slot B: never a destination)

        for M in sorted(set(int(m) for m in args.ms.split(','))):
            C = scale * rs.randn(M, D)
            occ = dev.occupancy(C, None, q)
            fn = dev.projections(rs.randn(M, D) / np.sqrt(D))
            fn.ring_alloc(B)

            def part(which):
                engine.check(lib.mjhmc_test_occupancy_part(occ.handle, 0, 1, B, which), lib)
            passes = [('label', lambda: part(0)), ('count', lambda: part(1)),
                      ('accumulate', lambda: occ.accumulate(0, B, w_slot0=1)), ('copy', copies),
                      ('projections', lambda: fn.evaluate(0, B, 0))]
            times = dict((name, []) for name, _ in passes)
            for r in range(args.rounds + 1):                       # (round 0 warms up: the code objects)
                for name, call in passes:
                    if name == 'accumulate':
                        occ.reset()                                # (the count windows only add: keep W_units off 2^63)
                    t = window(call, args.inner, dev)
                    if r:
                        times[name].append(t)
            med = dict((name, statistics.median(ts)) for name, ts in times.items())
            t_copy = med['copy'] / B
            tables = occ.read()
            rec = dict(workload=key, D=D, N=N, M=M, block=B, rounds=args.rounds, inner=args.inner, slot_bytes=slot_bytes,
                       label_ms_per_state=spread(times['label'], 1e3 / B), count_ms_per_state=spread(times['count'], 1e3 / B),
                       accumulate_ms_per_state=spread(times['accumulate'], 1e3 / B),
                       copy_ms_per_slot=spread(times['copy'], 1e3 / B),
                       projections_ms_per_state=spread(times['projections'], 1e3 / B),
                       label_GBps=round(B * (state_bytes + Npad) / med['label'] / 1e9, 1),
                       copy_GBps_read_plus_write=round(2 * slot_bytes / t_copy / 1e9, 1),
                       label_f64_Tinstr_per_s=round(3.0 * B * N * D * M / med['label'] / 1e12, 3),
                       projections_f64_Tinstr_per_s=round(2.0 * B * N * D * M / med['projections'] / 1e12, 3),
                       label_over_projections_time=round(med['label'] / med['projections'], 3),
                       label_over_copy_time=round(med['label'] / B / t_copy, 3),
                       count_over_copy_time=round(med['count'] / B / t_copy, 3),
                       cells_visited=int(np.sum(tables['count'] > 0)))
            print(json.dumps(rec), flush=True)
            occ.close()
            fn.close()
        del dev


if __name__ == '__main__':
    main()
