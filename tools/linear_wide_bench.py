"""Wide linear-model energies on one device: the fused kernel over expert blocks x dim chunks against the
tall kernel's block.

    python tools/linear_wide_bench.py [--n 65536] [--L 20] [--runs 3] [--reps 3] [--models 1024x16384,2048x16384]

Softplus models E = sum_j softplus(w_j.x + b_j), float64 state (the multi-pass path), timed as tools/linear_tall_bench.py
times its models -- every model and the yardstick alternately, run by run, medians of --runs runs after a warm-up:

1. force evaluations alone: one evaluation of E and dE/dX of a recorded state of all --n particles through the sampler's
   own evaluation path (the energy observables' evaluate: the float32 down-cast of the rows, the force kernel, the up-cast
   and one row pass), wall clock around --reps synchronised calls;
2. one MarkovJumpHMC sampling iteration at --L leapfrog steps (HIP events around the call, mjhmc_last_timing).

The yardstick `tall 512x16384` is the tall kernel on a model of the same experts and one chunk of dims, in the same job:
its time per expert block is what a (block, chunk) of the wide kernel is compared against -- the same two GEMMs, plus here
64 KB of x read and 128 KB of dE/dX read-modify-write per (block, chunk).  Per model one line of JSON: ms, ms per
(expert block x dim chunk), and the fraction of the fp32 matrix-core peak for the flops the kernel executes
(4 x 512 nblk x 512 ND per particle and gradient, padding included) and for the flops the model needs (4 D K).  The
iteration's fractions count the forward trajectories only (L gradients per particle)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP32_MFMA_PEAK = 157.3e12     # MI355X, fp32 matrix FLOP/s at 2.4 GHz (tools/linear_bench.py)
SOFTPLUS = ('u > 20.f ? u : log1pf(expf(u))', '1.f/(1.f + expf(-u))')
P = 512


class Model(object):
    def __init__(self, name, D, K, n, wide=True):
        from mjhmc_amd import engine
        ctx = engine.context(0)
        rs = np.random.RandomState(D + K)
        W = rs.randn(K, D) / np.sqrt(D)
        b = 0.1 * rs.randn(K)
        make = engine.DeviceEnergy.from_linear_wide if wide else engine.DeviceEnergy.from_linear_tall
        t0 = time.perf_counter()
        self.en = make(ctx, W, b, *SOFTPLUS)
        self.setup_s = time.perf_counter() - t0
        self.name, self.D, self.K, self.n = name, D, K, n
        self.nblk, self.nd = (K + P - 1) // P, (D + P - 1) // P
        self.s = engine.DeviceSampler(self.en, 0.1 * rs.randn(D, n), seed=11, dtype='float64')
        self.eps = 0.5 / np.sqrt(max(1.0, K / (4.0 * D)))
        self.s.ring_alloc(1)
        self.s.set_hparams(self.eps, 0, -np.log(1 - 0.1) * 0.5, 1.0)
        self.s.iterate(1, ring_slot0=0)               # a recorded state for the evaluations (tools/linear_tall_bench.py)
        self.eo = self.s.energy_observables()
        self.eo.ring_alloc(1)
        self.eval_ms, self.iter_ms = [], []

    def time_eval(self, reps):
        self.eo.evaluate(0, 1)                        # warm-up (each call ends with a synchronising read-back)
        t = time.perf_counter()
        for _ in range(reps):
            self.eo.evaluate(0, 1)
        self.eval_ms.append((time.perf_counter() - t) * 1e3 / reps)

    def time_iter(self, L):
        self.s.set_hparams(self.eps, L, -np.log(1 - 0.1) * 0.5, 1.0)
        self.s.iterate(1)                             # warm-up
        self.s.sync()
        _, done = self.s.iterate(1)
        self.s.sync()
        assert done == 1, 'non-finite rate in %s' % self.name
        self.iter_ms.append(self.s.last_timing()['total_ms'])

    def report(self, L):
        ev, it = float(np.median(self.eval_ms)), float(np.median(self.iter_ms)) if self.iter_ms else None
        cells = self.nblk * self.nd
        padded = 4.0 * P * self.nblk * P * self.nd * self.n
        needed = 4.0 * self.D * self.K * self.n
        out = dict(model=self.name, D=self.D, K=self.K, nblk=self.nblk, nd=self.nd, n=self.n, state='float64',
                   eval_ms=ev, eval_runs_ms=self.eval_ms, eval_ms_per_block_chunk=ev / cells,
                   eval_frac_padded=padded / (ev * 1e-3) / FP32_MFMA_PEAK, eval_frac_needed=needed / (ev * 1e-3) / FP32_MFMA_PEAK,
                   matrix_bytes=2 * cells * P * P * 4, setup_s=self.setup_s)
        if it is not None:
            out.update(L=L, iter_ms=it, iter_runs_ms=self.iter_ms, iter_ms_per_block_chunk_gradient=it / (cells * L),
                       iter_frac_padded=padded * L / (it * 1e-3) / FP32_MFMA_PEAK,
                       iter_frac_needed=needed * L / (it * 1e-3) / FP32_MFMA_PEAK)
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=65536)
    ap.add_argument('--L', type=int, default=20)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--models', default='1024x16384,2048x16384')
    ap.add_argument('--yardstick', default='512x16384')
    ap.add_argument('--no-iterations', action='store_true')
    a = ap.parse_args()
    D, K = (int(v) for v in a.yardstick.split('x'))
    models = [Model('tall %dx%d' % (D, K), D, K, a.n, wide=False)]
    for m in a.models.split(','):
        D, K = (int(v) for v in m.split('x'))
        models.append(Model('wide %dx%d' % (D, K), D, K, a.n))
    for r in range(a.runs):                           # alternating: the yardstick, wide ..., the yardstick, ...
        for m in models:
            m.time_eval(a.reps)
    if not a.no_iterations:
        for r in range(a.runs):
            for m in models:
                m.time_iter(a.L)
    for m in models:
        print(json.dumps(m.report(a.L)), flush=True)


if __name__ == '__main__':
    main()
