"""Per-group statistics of a grouped linear model on one device: the group pointwise pass against one
grouped force evaluation of the same model, and against the tall pointwise pass on a tall model of the same padded width
and block count.

    python tools/group_pointwise_bench.py [--n 65536] [--runs 3] [--reps 3] [--shapes 10x2,10x10,10x16,300x10] [--blocks 8,40]

Per shape D x C and number of grouped blocks nbg: a grouped model of G = nbg * 8 * floor(16 NB / C) groups (every grouped
block full, no plain experts), float64 state (the multi-pass path), one recorded state of all --n particles.  Three call
times, alternating run by run in the same process, medians of --runs runs after a warm-up, wall clock around --reps
synchronised calls (every call ends with its one read-back):

* `pass`: mjhmc_pointwise_accumulate of one slot on the grouped handle with two values -- q[0]*(u - lse) per group with its
  log-mean-exp, and sm per member -- i.e. the narrowing of the slot to float32 rows, the generated kernel (GEMM 1 per block,
  the group terms, the values, the reductions) and the fold over strips;
* `eval`: one evaluation call of E and dE/dX of the same slot through the sampler's own evaluation path
  (lin_grouped_eval_kernel: both GEMMs per block);
* `tall`: the per-expert pass (tools/pointwise_bench.py's two values) on a softplus tall model of nbg blocks of the same P.

One line of JSON per (shape, nbg)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SOFTPLUS = ('u > 20.f ? u : log1pf(expf(u))', '1.f/(1.f + expf(-u))')
TALL_VALUES = ['-(%s)' % SOFTPLUS[0], SOFTPLUS[1]]
GROUP_ENERGY = ('-q[0]*u', '-q[0]')
GROUP_VALUES, GROUP_FLAGS, GROUP_PER = ['q[0]*(u - lse)', 'sm'], [True, False], ['group', 'member']


def pad_of(D):
    return 128 if D <= 128 else (256 if D <= 256 else 512)


class Recorded(object):
    """a sampler with one recorded state of n particles, its evaluation handle and one pointwise handle"""

    def __init__(self, en, D, n, rs, make):
        from mjhmc_amd import engine
        self.s = engine.DeviceSampler(en, 0.1 * rs.randn(D, n), seed=11, dtype='float64')
        self.s.ring_alloc(1)
        self.s.set_hparams(0.1, 0, 0.05, 1.0)          # L = 0: a recorded state, and the multi-pass workspace exists
        self.s.iterate(1, ring_slot0=0)
        self.eo = self.s.energy_observables()
        self.eo.ring_alloc(1)
        self.pw = make(self.s)

    def close(self):
        self.pw.close()
        self.eo.close()
        self.s.close()


def timed(call, reps):
    call()                                            # warm-up (each call ends with a synchronising read-back)
    t = time.perf_counter()
    for _ in range(reps):
        call()
    return (time.perf_counter() - t) * 1e3 / reps


def measure(D, C, nbg, n, runs, reps):
    from mjhmc_amd import engine
    ctx = engine.context(0)
    P = pad_of(D)
    Gl = 16 * (P // 128) // C
    G = nbg * 8 * Gl
    rs = np.random.RandomState(D + 131 * C + nbg)
    K = G * C
    W, b = rs.randn(K, D) / np.sqrt(D), 0.1 * rs.randn(K)
    q = np.zeros((1, K))
    q[0, np.arange(G) * C + rs.randint(0, C, size=G)] = 1.0
    grouped = Recorded(engine.DeviceEnergy.from_linear_grouped(ctx, W, b, (C, G), *GROUP_ENERGY, expert_params=q), D, n, rs,
                       lambda s: s.group_pointwise(GROUP_VALUES, GROUP_FLAGS, GROUP_PER))
    Kt = nbg * P
    tall = Recorded(engine.DeviceEnergy.from_linear_tall(ctx, rs.randn(Kt, D) / np.sqrt(D), 0.1 * rs.randn(Kt), *SOFTPLUS), D, n,
                    rs, lambda s: s.pointwise(TALL_VALUES, [True, False]))
    assert grouped.pw.nexperts == K and tall.pw.nexperts == Kt
    ps, ev, tl = [], [], []
    for _ in range(runs):
        ps.append(timed(lambda: grouped.pw.accumulate(0, 1), reps))
        ev.append(timed(lambda: grouped.eo.evaluate(0, 1), reps))
        tl.append(timed(lambda: tall.pw.accumulate(0, 1), reps))
    grouped.close()
    tall.close()
    p, e, t = (float(np.median(v)) for v in (ps, ev, tl))
    return dict(shape='%dx%d' % (D, C), n=n, P=P, Gl=Gl, G=G, nbg=nbg, state='float64', pass_ms=p, pass_runs_ms=ps,
                pass_ms_per_block=p / nbg, eval_ms=e, eval_runs_ms=ev, eval_ms_per_block=e / nbg, tall_ms=t, tall_runs_ms=tl,
                tall_ms_per_block=t / nbg, pass_over_eval=p / e, pass_over_tall=p / t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=65536)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--shapes', default='10x2,10x10,10x16,300x10')
    ap.add_argument('--blocks', default='8,40')
    a = ap.parse_args()
    for shape in a.shapes.split(','):
        D, C = (int(v) for v in shape.split('x'))
        for nbg in (int(v) for v in a.blocks.split(',')):
            print(json.dumps(measure(D, C, nbg, a.n, a.runs, a.reps)), flush=True)


if __name__ == '__main__':
    main()
