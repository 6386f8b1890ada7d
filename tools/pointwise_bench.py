"""Per-expert statistics of a tall linear model on one device: the pointwise pass against one force
evaluation of the same model, and against the host path.

    python tools/pointwise_bench.py [--n 65536] [--runs 3] [--reps 3] [--models 512x65536,32x16384] [--host-model 32x16384]
                                    [--host-n 4096]

Softplus models E = sum_j softplus(w_j.x + b_j), float64 state (the multi-pass path), one recorded state of all --n
particles.  Per model, alternating run by run, medians of --runs runs after a warm-up, wall clock around --reps
synchronised calls (every call ends with its one read-back):

* `pass`: mjhmc_pointwise_accumulate of one slot with two values -- l = -softplus(u) with its log-mean-exp, and
  sigmoid(u) -- i.e. the narrowing of the slot to float32 rows, the generated kernel (GEMM 1 per block, the values, the
  reductions) and the fold over strips;
* `eval` (the yardstick): one evaluation call of E and dE/dX of the same slot through the sampler's own evaluation path
  (lin_tall_eval_kernel: both GEMMs per block), as tools/linear_tall_bench.py times it.

At --host-model x --host-n, a shape the host holds, also the NumPy path: the slot downloaded (ring_read), u = W X + b and
the same statistics in float64.  One line of JSON per model."""
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
VALUES = ['-(%s)' % SOFTPLUS[0], SOFTPLUS[1]]


def pad_of(D):
    return 128 if D <= 128 else (256 if D <= 256 else 512)


class Model(object):
    def __init__(self, D, K, n):
        from mjhmc_amd import engine
        ctx = engine.context(0)
        rs = np.random.RandomState(D + K)
        self.W = rs.randn(K, D) / np.sqrt(D)
        self.b = 0.1 * rs.randn(K)
        self.en = engine.DeviceEnergy.from_linear_tall(ctx, self.W, self.b, *SOFTPLUS)
        self.D, self.K, self.n = D, K, n
        self.P = pad_of(D)
        self.nblk = (K + self.P - 1) // self.P
        self.s = engine.DeviceSampler(self.en, 0.1 * rs.randn(D, n), seed=11, dtype='float64')
        self.s.ring_alloc(1)
        self.s.set_hparams(0.1, 0, 0.05, 1.0)          # L = 0: a recorded state, and the multi-pass workspace exists
        self.s.iterate(1, ring_slot0=0)
        self.eo = self.s.energy_observables()
        self.eo.ring_alloc(1)
        t0 = time.perf_counter()
        self.pw = self.s.pointwise(VALUES, [True, False])
        self.create_s = time.perf_counter() - t0
        self.pass_ms, self.eval_ms = [], []

    def time_once(self, reps):
        self.pw.accumulate(0, 1)                      # warm-up (each call ends with a synchronising read-back)
        t = time.perf_counter()
        for _ in range(reps):
            self.pw.accumulate(0, 1)
        self.pass_ms.append((time.perf_counter() - t) * 1e3 / reps)
        self.eo.evaluate(0, 1)
        t = time.perf_counter()
        for _ in range(reps):
            self.eo.evaluate(0, 1)
        self.eval_ms.append((time.perf_counter() - t) * 1e3 / reps)

    def host_path(self):
        t = time.perf_counter()
        X = self.s.ring_read(0, 1)
        t_down = time.perf_counter() - t
        u = self.W.dot(X) + self.b[:, None]
        ll = -np.where(u > 20, u, np.log1p(np.exp(np.minimum(u, 20))))
        mean = ll.mean(axis=1)
        var = (ll * ll).mean(axis=1) - mean * mean
        mx = ll.max(axis=1)
        lme = np.log(np.exp(ll - mx[:, None]).mean(axis=1)) + mx
        fit = (1 / (1 + np.exp(-u))).mean(axis=1)
        total = time.perf_counter() - t
        W, S1, S2, lmx, lse, _ = self.pw.read()
        return dict(host_ms=total * 1e3, host_download_ms=t_down * 1e3,
                    host_max_abs_diff_mean=float(np.abs(S1[0] / W - mean).max()), host_checksum=float(var.sum() + lme.sum() + fit.sum()))

    def report(self):
        ps, ev = float(np.median(self.pass_ms)), float(np.median(self.eval_ms))
        gemm1 = 2.0 * self.P * self.nblk * self.P * self.n
        return dict(model='%dx%d' % (self.D, self.K), n=self.n, P=self.P, nblk=self.nblk, values=len(VALUES), state='float64',
                    pass_ms=ps, pass_runs_ms=self.pass_ms, pass_ms_per_block=ps / self.nblk,
                    pass_frac_gemm1_padded=gemm1 / (ps * 1e-3) / FP32_MFMA_PEAK,
                    eval_ms=ev, eval_runs_ms=self.eval_ms, eval_ms_per_block=ev / self.nblk, pass_over_eval=ps / ev,
                    create_s=self.create_s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=65536)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--models', default='512x65536,32x16384')
    ap.add_argument('--host-model', default='32x16384')
    ap.add_argument('--host-n', type=int, default=4096)
    a = ap.parse_args()
    models = []
    for m in a.models.split(','):
        D, K = (int(v) for v in m.split('x'))
        models.append(Model(D, K, a.n))
    for r in range(a.runs):
        for m in models:
            m.time_once(a.reps)
    for m in models:
        print(json.dumps(m.report()), flush=True)
    if a.host_model:
        D, K = (int(v) for v in a.host_model.split('x'))
        h = Model(D, K, a.host_n)
        for r in range(a.runs):
            h.time_once(a.reps)
        h.pw.reset()
        h.pw.accumulate(0, 1)
        out = h.report()
        out.update(h.host_path())
        print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
