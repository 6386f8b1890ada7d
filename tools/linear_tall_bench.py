"""Tall linear-model energies on one device: the fused block kernel against the tile kernels' evaluation.

    python tools/linear_tall_bench.py [--n 65536] [--L 20] [--runs 3] [--reps 5] [--models 512x512,512x4096,...]

Softplus models E = sum_j softplus(w_j.x + b_j), float64 state (the multi-pass path).  Two parts, every model and the
yardstick timed alternately, run by run, medians of --runs runs after a warm-up:

1. force evaluations alone: one evaluation of E and dE/dX of a recorded state of all --n particles through the sampler's
   own evaluation path (the energy observables' evaluate: the float32 down-cast of the rows, the force kernel, the up-cast
   and one row pass -- the same passes around either kernel), wall clock around --reps synchronised calls;
2. one MarkovJumpHMC sampling iteration at --L leapfrog steps (HIP events around the call, mjhmc_last_timing).

The yardstick `tile512` is the <= 512 entry point's model of 512 x 512 experts: lin_eval_kernel, the kernel the tall one is
built from.  Per model one line of JSON: ms, ms per expert block, and the fraction of the fp32 matrix-core peak for the
flops the kernel executes (4 P nblk P per particle and gradient, padding included) and for the flops the model needs
(4 D K).  The iteration's fractions count the forward trajectories only (L gradients per particle), as
tools/linear_bench.py does."""
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


def pad_of(D):
    return 128 if D <= 128 else (256 if D <= 256 else 512)


class Model(object):
    def __init__(self, name, D, K, n, tile=False):
        from mjhmc_amd import engine
        ctx = engine.context(0)
        rs = np.random.RandomState(D + K)
        W = rs.randn(K, D) / np.sqrt(D)
        b = 0.1 * rs.randn(K)
        make = engine.DeviceEnergy.from_linear if tile else engine.DeviceEnergy.from_linear_tall
        t0 = time.perf_counter()
        self.en = make(ctx, W, b, *SOFTPLUS)
        self.setup_s = time.perf_counter() - t0
        self.name, self.D, self.K, self.n = name, D, K, n
        self.P = max(pad_of(D), pad_of(K)) if tile else pad_of(D)
        self.nblk = 1 if tile else (K + self.P - 1) // self.P
        self.s = engine.DeviceSampler(self.en, 0.1 * rs.randn(D, n), seed=11, dtype='float64')
        self.eps = 0.5 / np.sqrt(max(1.0, K / (4.0 * D)))
        self.s.ring_alloc(1)
        # a recorded state for the evaluations.  L = 0 takes the multi-pass path for the yardstick too: its workspace then
        # exists, and an evaluation reuses it like a tall model's instead of allocating its float32 rows per call
        self.s.set_hparams(self.eps, 0, -np.log(1 - 0.1) * 0.5, 1.0)
        self.s.iterate(1, ring_slot0=0)
        self.eo = self.s.energy_observables()
        self.eo.ring_alloc(1)
        self.eval_ms, self.iter_ms = [], []

    def time_eval(self, reps):
        self.eo.evaluate(0, 1)                        # warm-up (each call ends with a synchronising read-back)
        t = time.perf_counter()
        for _ in range(reps):
            self.eo.evaluate(0, 1)
        self.eval_ms.append((time.perf_counter() - t) * 1e3 / reps)

    def time_iter(self, L, steps):
        self.s.set_hparams(self.eps, L, -np.log(1 - 0.1) * 0.5, 1.0)
        self.s.iterate(1)                             # warm-up
        self.s.sync()
        _, done = self.s.iterate(steps)
        self.s.sync()
        assert done == steps, 'non-finite rate in %s' % self.name
        self.iter_ms.append(self.s.last_timing()['total_ms'] / steps)

    def report(self, L):
        ev, it = float(np.median(self.eval_ms)), float(np.median(self.iter_ms)) if self.iter_ms else None
        padded = 4.0 * self.P * self.nblk * self.P * self.n
        needed = 4.0 * self.D * self.K * self.n
        out = dict(model=self.name, D=self.D, K=self.K, P=self.P, nblk=self.nblk, n=self.n, state='float64',
                   eval_ms=ev, eval_runs_ms=self.eval_ms, eval_ms_per_block=ev / self.nblk,
                   eval_frac_padded=padded / (ev * 1e-3) / FP32_MFMA_PEAK, eval_frac_needed=needed / (ev * 1e-3) / FP32_MFMA_PEAK,
                   matrix_bytes=2 * self.nblk * self.P * self.P * 4, setup_s=self.setup_s)
        if it is not None:
            out.update(L=L, iter_ms=it, iter_runs_ms=self.iter_ms, iter_frac_padded=padded * L / (it * 1e-3) / FP32_MFMA_PEAK,
                       iter_frac_needed=needed * L / (it * 1e-3) / FP32_MFMA_PEAK)
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=65536)
    ap.add_argument('--L', type=int, default=20)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--models', default='512x512,512x4096,512x16384,512x65536,32x16384')
    ap.add_argument('--no-iterations', action='store_true')
    a = ap.parse_args()
    models = [Model('tile512', 512, 512, a.n, tile=True)]
    for m in a.models.split(','):
        D, K = (int(v) for v in m.split('x'))
        models.append(Model('tall %dx%d' % (D, K), D, K, a.n))
    for r in range(a.runs):                           # alternating: tile512, tall ..., tile512, ...
        for m in models:
            m.time_eval(a.reps if m.nblk <= 32 else 2)
    if not a.no_iterations:
        for r in range(a.runs):
            for m in models:
                m.time_iter(a.L, 3 if m.nblk <= 8 else 1)
    for m in models:
        print(json.dumps(m.report(a.L)), flush=True)


if __name__ == '__main__':
    main()
