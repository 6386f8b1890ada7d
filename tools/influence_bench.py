"""Data-row influence of a tall linear model on one device: one accumulate call per slot against the
pointwise pass and against one force evaluation of the same model.

    python tools/influence_bench.py [--n 65536] [--runs 3] [--reps 3] [--models 512x65536,32x16384] [--dtype float64]

Softplus models E = sum_j softplus(w_j.x + b_j), one recorded state of all --n particles.  Per model, alternating run by
run, medians of --runs runs after a warm-up, wall clock around --reps synchronised calls (every call ends with its one
read-back):

* `influence`: mjhmc_influence_accumulate of one slot with the value l = -softplus(u) over all K experts -- the moments
  of the state and, panel of P experts by panel, the generated kernel (GEMM 1 and the stored values), the widening of
  the panel for a float64 state, the moment pass on the panel and the cross pass on the float64 matrix cores;
* `pointwise`: mjhmc_pointwise_accumulate of the same slot with the same one value (no log-mean-exp): GEMM 1 per block
  and the reductions, nothing stored;
* `eval` (the yardstick): one evaluation call of E and dE/dX of the same slot through the sampler's own evaluation path
  (lin_tall_eval_kernel: both GEMMs per block), as tools/pointwise_bench.py times it.

One line of JSON per model."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SOFTPLUS = ('u > 20.f ? u : log1pf(expf(u))', '1.f/(1.f + expf(-u))')
VALUE = '-(%s)' % SOFTPLUS[0]


class Model(object):
    def __init__(self, D, K, n, dtype):
        from mjhmc_amd import engine
        ctx = engine.context(0)
        rs = np.random.RandomState(D + K)
        self.W = rs.randn(K, D) / np.sqrt(D)
        self.b = 0.1 * rs.randn(K)
        self.en = engine.DeviceEnergy.from_linear_tall(ctx, self.W, self.b, *SOFTPLUS)
        self.D, self.K, self.n, self.dtype = D, K, n, dtype
        self.s = engine.DeviceSampler(self.en, 0.1 * rs.randn(D, n), seed=11, dtype=dtype)
        self.s.ring_alloc(1)
        self.s.set_hparams(0.1, 0, 0.05, 1.0)          # L = 0: a recorded state, and the multi-pass workspace exists
        self.s.iterate(1, ring_slot0=0)
        self.eo = self.s.energy_observables()
        self.eo.ring_alloc(1)
        self.pw = self.s.pointwise([VALUE], [False])
        t0 = time.perf_counter()
        self.inf = self.s.influence(VALUE)
        self.create_s = time.perf_counter() - t0
        self.P = self.inf.panel_experts
        self.panels = (K + self.P - 1) // self.P
        # the shift a run would use: the means of this slot
        self.pw.accumulate(0, 1)
        Wt, S1 = self.pw.read()[:2]
        self.inf.set_shift(None, S1[0] / Wt)
        self.ms = dict(influence=[], pointwise=[], eval=[])

    def time_once(self, reps):
        for name, call in (('influence', lambda: self.inf.accumulate(0, 1)), ('pointwise', lambda: self.pw.accumulate(0, 1)),
                           ('eval', lambda: self.eo.evaluate(0, 1))):
            call()                                      # warm-up (each call ends with a synchronising read-back)
            t = time.perf_counter()
            for _ in range(reps):
                call()
            self.ms[name].append((time.perf_counter() - t) * 1e3 / reps)

    def report(self):
        med = dict((k, float(np.median(v))) for k, v in self.ms.items())
        t = time.perf_counter()
        C = self.inf.read_cross()
        read_ms = (time.perf_counter() - t) * 1e3
        W = self.inf.read()[0]
        return dict(model='%dx%d' % (self.D, self.K), n=self.n, P=self.P, panels=self.panels, state=self.dtype,
                    influence_ms=med['influence'], influence_runs_ms=self.ms['influence'],
                    influence_ms_per_panel=med['influence'] / self.panels,
                    pointwise_ms=med['pointwise'], pointwise_runs_ms=self.ms['pointwise'],
                    pointwise_ms_per_block=med['pointwise'] / self.panels,
                    eval_ms=med['eval'], eval_runs_ms=self.ms['eval'],
                    influence_over_pointwise=med['influence'] / med['pointwise'], influence_over_eval=med['influence'] / med['eval'],
                    scratch_bytes=self.inf.scratch_bytes, totals_bytes=8 * self.D * self.K, read_cross_ms=read_ms,
                    create_s=self.create_s, finite=bool(np.isfinite(C).all()), checksum=float(np.abs(C).sum() / W))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=65536)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--models', default='512x65536,32x16384')
    ap.add_argument('--dtype', default='float64')
    a = ap.parse_args()
    models = []
    for m in a.models.split(','):
        D, K = (int(v) for v in m.split('x'))
        models.append(Model(D, K, a.n, a.dtype))
    for r in range(a.runs):
        for m in models:
            m.time_once(a.reps)
    for m in models:
        print(json.dumps(m.report()), flush=True)


if __name__ == '__main__':
    main()
