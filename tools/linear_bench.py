"""Linear-model energies against the built-in ProductOfT on one device.

    python tools/linear_bench.py [--n 100000] [--L 20] [--steps 10] [--runs 3]

Times, alternating run by run: ProductOfT 512 x 512 (float64 state) as the built-in energy and as its linear form
(W' = (W / nu)^T, b' = b / nu, q[0] = (nu + 1) / 2, f = q0 log(1 + u^2), f' = 2 q0 u / (1 + u^2)), and a 512-dim
CorrelatedGaussian.  One line of JSON per workload: ms per iteration (median of the runs, each one call of --steps
iterations after a warm-up call), and the fraction of the fp32 matrix-core peak the force's flops need --
4 D K flop per particle and gradient, L gradients per particle per forward trajectory (the inverse-L trajectories the
jump process integrates on top are not counted)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP32_MFMA_PEAK = 157.3e12     # MI355X, fp32 matrix FLOP/s at 2.4 GHz (v_mfma_f32_32x32x2_f32: 256 CUs x 4 SIMDs x 256 flop/clk / 4)


def sampler(kind, D, n, seed=7):
    from mjhmc_amd import engine, _lib
    from mjhmc_amd.misc.distributions import CorrelatedGaussian
    from tests.helpers import ref_init_weights
    ctx = engine.context(0)
    rs = np.random.RandomState(seed)
    X0 = rs.randn(D, n)
    if kind == 'gauss':
        c = CorrelatedGaussian(ndims=D, nbatch=2, seed=1)
        en = engine.DeviceEnergy.from_linear(ctx, c.L.T, np.zeros(D), '0.5f*u*u', 'u')
    else:
        W, lognu = ref_init_weights(D, D)
        W = (W + np.eye(D)).astype(np.float32).astype(np.float64)
        nu = np.exp(lognu).astype(np.float32).astype(np.float64)
        if kind == 'pot':
            params = np.concatenate([[float(D)], W.ravel(), nu, np.zeros(D)])
            en = engine.DeviceEnergy(ctx, _lib.E_PRODUCT_OF_T, D, params)
        else:
            en = engine.DeviceEnergy.from_linear(ctx, (W / nu[None, :]).T, np.zeros(D), 'q[0]*logf(1.f + u*u)',
                                                 '2.f*q[0]*u/(1.f + u*u)', (), ((nu + 1) / 2)[None, :])
    s = engine.DeviceSampler(en, X0, seed=11, dtype='float64')
    return en, s


def time_call(s, steps):
    s.iterate(steps)           # warm-up call (also the clock ramp)
    s.sync()
    t = time.perf_counter()
    s.iterate(steps)
    s.sync()
    return (time.perf_counter() - t) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=100000)
    ap.add_argument('--D', type=int, default=512)
    ap.add_argument('--L', type=int, default=20)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--runs', type=int, default=3)
    a = ap.parse_args()
    D, n = a.D, a.n
    t0 = time.perf_counter()
    built = {k: sampler(k, D, n) for k in ('pot', 'pot_linear', 'gauss')}
    build_s = time.perf_counter() - t0
    for en, s in built.values():
        s.set_hparams(0.05, a.L, -np.log(1 - 0.1) * 0.5, 1.0)
    ms = {k: [] for k in built}
    for r in range(a.runs):                         # alternating: pot, pot_linear, gauss, pot, ...
        for k, (en, s) in built.items():
            ms[k].append(time_call(s, a.steps))
    flops = 4.0 * D * D * n * a.L                   # per iteration, forward trajectories
    for k, v in ms.items():
        med = float(np.median(v))
        print(json.dumps(dict(workload=k, D=D, K=D, n=n, L=a.L, state='float64', ms_per_iter=med, runs_ms=v,
                              fp32_mfma_fraction=flops / (med * 1e-3) / FP32_MFMA_PEAK, setup_s=build_s)))


if __name__ == '__main__':
    main()
