"""Grouped linear-model energies on one device: the grouped kernel's expert block against the tall kernel's.

    python tools/linear_grouped_bench.py [--n 65536] [--runs 3] [--reps 5] [--dims 10,300] [--sizes 2,10,16]
                                         [--blocks 8,40] [--out profiles/r21/linear_grouped.md]

Per (D, C): a grouped model whose blocks are all grouped and full -- G = nblk * 8 * floor(16 NB / C) groups, f = -q[0] u
with a one-hot q[0], no plain experts -- against a tall softplus model of the same P and the same number of blocks
(K = nblk * P): one evaluation of E and dE/dX of a recorded state of all --n particles through the sampler's own evaluation
path (the energy observables' evaluate, as tools/linear_tall_bench.py times it), float64 state.  The two models of a pair
are timed alternately, --runs runs each of --reps synchronised calls after a warm-up, and the medians are reported.  Both
are measured at the two block counts of --blocks: the time per block is the difference of the two medians over the
difference of the block counts, which leaves out what a call costs around the kernel's block loop.  One line of JSON per
pair; --out writes the table as Markdown."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SOFTPLUS = ('u > 20.f ? u : log1pf(expf(u))', '1.f/(1.f + expf(-u))')
SOFTMAX = ('-q[0]*u', '-q[0]')


def pad_of(D):
    return 128 if D <= 128 else (256 if D <= 256 else 512)


class Model(object):
    def __init__(self, D, nblk, n, C=None):
        from mjhmc_amd import engine
        ctx = engine.context(0)
        P = pad_of(D)
        rs = np.random.RandomState(D + nblk + (C or 0))
        if C is None:
            K = nblk * P
            W, b = rs.randn(K, D) / np.sqrt(D), 0.1 * rs.randn(K)
            self.en = engine.DeviceEnergy.from_linear_tall(ctx, W, b, *SOFTPLUS)
        else:
            G = nblk * 8 * (16 * (P // 128) // C)
            K = G * C
            W, b = rs.randn(K, D) / np.sqrt(D), 0.1 * rs.randn(K)
            q = np.zeros((1, K))
            q[0, np.arange(G) * C + rs.randint(0, C, size=G)] = 1.0
            self.en = engine.DeviceEnergy.from_linear_grouped(ctx, W, b, (C, G), *SOFTMAX, expert_params=q)
        self.K, self.nblk = K, nblk
        self.s = engine.DeviceSampler(self.en, 0.1 * rs.randn(D, n), seed=11, dtype='float64')
        self.s.ring_alloc(1)
        self.s.set_hparams(0.01, 0, -np.log(1 - 0.1) * 0.5, 1.0)
        self.s.iterate(1, ring_slot0=0)               # a recorded state for the evaluations (tools/linear_tall_bench.py)
        self.eo = self.s.energy_observables()
        self.eo.ring_alloc(1)
        self.ms = []

    def time_eval(self, reps):
        self.eo.evaluate(0, 1)                        # warm-up (each call ends with a synchronising read-back)
        t = time.perf_counter()
        for _ in range(reps):
            self.eo.evaluate(0, 1)
        self.ms.append((time.perf_counter() - t) * 1e3 / reps)

    def median(self):
        return float(np.median(self.ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=65536)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--dims', default='10,300')
    ap.add_argument('--sizes', default='2,10,16')
    ap.add_argument('--blocks', default='8,40')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    n0, n1 = (int(v) for v in a.blocks.split(','))
    rows = []
    for D in (int(v) for v in a.dims.split(',')):
        P = pad_of(D)
        tall = [Model(D, n0, a.n), Model(D, n1, a.n)]
        for C in (int(v) for v in a.sizes.split(',')):
            grouped = [Model(D, n0, a.n, C), Model(D, n1, a.n, C)]
            for m in tall:
                m.ms = []
            for r in range(a.runs):                   # alternating: grouped, tall, grouped, tall, ...
                for g, t in zip(grouped, tall):
                    g.time_eval(a.reps)
                    t.time_eval(a.reps)
            per = lambda pair: (pair[1].median() - pair[0].median()) / (n1 - n0) * 1e3        # noqa: E731  (us per block)
            row = dict(D=D, P=P, C=C, n=a.n, blocks=[n0, n1], slots_used=8 * (16 * (P // 128) // C) * C / float(P),
                       grouped_ms=[m.median() for m in grouped], tall_ms=[m.median() for m in tall],
                       grouped_runs_ms=[m.ms for m in grouped], tall_runs_ms=[m.ms for m in tall],
                       grouped_us_per_block=per(grouped), tall_us_per_block=per(tall), ratio=per(grouped) / per(tall))
            rows.append(row)
            print(json.dumps(row), flush=True)
            del grouped
    if a.out:
        with open(a.out, 'w') as f:
            f.write('# Grouped linear-model kernel: time per expert block against the tall kernel\n\n')
            f.write('`python tools/linear_grouped_bench.py --n %d --runs %d --reps %d --blocks %s`: one evaluation of E and '
                    'dE/dX of %d particles, float64 state; medians of %d alternating runs; the time per block is the '
                    'difference between the %d-block and the %d-block model.\n\n' % (a.n, a.runs, a.reps, a.blocks, a.n, a.runs, n1, n0))
            f.write('| D | P | C | slots used | grouped ms (%d / %d blocks) | tall ms (%d / %d blocks) | grouped us/block | '
                    'tall us/block | ratio |\n|---|---|---|---|---|---|---|---|---|\n' % (n0, n1, n0, n1))
            for r in rows:
                f.write('| %d | %d | %d | %.3f | %.3f / %.3f | %.3f / %.3f | %.1f | %.1f | %.3f |\n'
                        % (r['D'], r['P'], r['C'], r['slots_used'], r['grouped_ms'][0], r['grouped_ms'][1], r['tall_ms'][0],
                           r['tall_ms'][1], r['grouped_us_per_block'], r['tall_us_per_block'], r['ratio']))


if __name__ == '__main__':
    main()
