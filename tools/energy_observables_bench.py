"""Time the energy observables [E, grad_sq, virial] against their yardsticks, per recorded state, at the benchmark's sizes.

For each workload (bench.py WORKLOADS; c2: iso Gaussian 512 x 100 000 fp64; c3f64: ProductOfT 512 x 100 000, float64 state
around the float32 force; c4: Neal funnel 32 x 1 000 000 fp64; c5: SparseImageCode 1024 x 200 000 float32 state) and each
block of K ring slots (--blocks), on a sampler of the TEST build of the library (the two halves of an evaluation can be
launched apart there, mjhmc_test_energy_observables_part; same kernels, same flags):
  the evaluation launches alone (the energy family's own kernels on the ring slots, E and dE/dX into the handle's scratch),
  the new reduction kernel alone (energy_observables_kernel: slot + scratch -> derived slot),
  DeviceFunctionals.evaluate (both, plus the flag read-back) and K device-to-device slot copies (mjhmc_ring_copy: read +
  write) in the same job, --inner calls per timed window; host clock around calls that end in a device synchronise, median
  of --reps repetitions after one warm-up.
Bytes of the reduction of one state: the state matrix and the gradient matrix read once, Npad * 32 bytes written; its rate
is those bytes over its time, next to the copy's (2 * slot_bytes over a slot's copy time).
--replaced: also the host path once -- sample(K, preserve_order=True), then distribution.E_val / dEdX_val per recorded
state, then the two sums in NumPy.
--temperature: sampler.temperature(--states) after burn_in() for c5 and c5bf16 (T, stderr, z, ESS of the virial, R-hat of E).
usage: python tools/energy_observables_bench.py [--only c2,c3f64,c4,c5] [--blocks 8] [--reps 5] [--inner 4] [--n N]
                                                 [--replaced] [--temperature] [--states 64]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import bench                                                             # noqa: E402
from chainstats_bench import timed, repeated, copy_time                  # noqa: E402
from mjhmc_amd import engine, _lib                                       # noqa: E402
from mjhmc_amd.misc import distributions as dists                        # noqa: E402
from mjhmc_amd.samplers.markov_jump_hmc import MarkovJumpHMC             # noqa: E402


def make_distribution(key, n):
    w = dict(bench.WORKLOADS[key])
    N = n or w['N']
    X0 = bench.initial_state(w, N, 0)
    if w['kind'] == 'iso':
        cls, kw = dists.TestGaussian, dict(ndims=w['D'], nbatch=N, sigma=w['params'][0])
    elif w['kind'] == 'funnel':
        cls, kw = dists.Funnel, dict(scale=w['params'][0], nbatch=N, ndims=w['D'])
    elif w['kind'] == 'pot':
        W, lognu = bench.pot_model(w['D'])
        cls, kw = dists.ProductOfT, dict(ndims=w['D'], nbasis=w['D'], nbatch=N, lognu=lognu, W=W, state_dtype=w['dtype'])
    else:
        B, y, _ = bench.sic_model()
        cls, kw = dists.SparseImageCode, dict(n_patches=1, n_batches=N, cauchy=True, n_basis=w['D'], basis=B,
                                              imgs=y.reshape(-1, 1), init=X0, state_dtype=w['dtype'])

    class Fixed(cls):
        def gen_init_X(self):
            self.Xinit = X0
    return Fixed(**kw), w, N


def make_sampler(key, n):
    d, w, N = make_distribution(key, n)
    return MarkovJumpHMC(distribution=d, epsilon=w['eps'], beta=w['beta'], num_leapfrog_steps=w['L'], seed=1, resample=False), w, N


def hooks_device(key, n, slots):
    """a DeviceSampler of the test build with `slots` recorded ring slots (its own iterations), and what it was made from"""
    d, w, N = make_distribution(key, n)
    ctx = engine.Context(0, lib=_lib.load_test_hooks())
    kind, params = d.device_energy()
    en = engine.DeviceEnergy(ctx, kind, w['D'], params)
    dev = engine.DeviceSampler(en, np.ascontiguousarray(d.Xinit), seed=1, dtype=w['dtype'], mode=_lib.MODE_MJHMC)
    dev.set_hparams(w['eps'], w['L'], -np.log(1 - w['beta']) * 0.5, 1.0)
    dev.ring_alloc(slots)
    dev.iterate(slots, ring_slot0=0)
    dev.sync()
    return ctx, dev, w, N


def rounded(rec):
    return json.dumps({k: (round(v, 5) if isinstance(v, float) else v) for k, v in rec.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', default='c2,c3f64,c4,c5')
    ap.add_argument('--blocks', default='8')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--inner', type=int, default=4, help='calls per timed window')
    ap.add_argument('--n', type=int, default=0, help='particles (default: the workload\'s)')
    ap.add_argument('--states', type=int, default=64, help='n_iter of the temperature() runs')
    ap.add_argument('--replaced', action='store_true')
    ap.add_argument('--temperature', action='store_true')
    args = ap.parse_args()
    for key in [k for k in args.only.split(',') if k]:
        for K in [int(b) for b in args.blocks.split(',')]:
            ctx, dev, w, N = hooks_device(key, args.n, K + 1)
            lib = ctx.lib
            b = ctypes.c_uint64()
            lib.mjhmc_ring_slot_bytes(dev.handle, ctypes.byref(b))
            slot_bytes = int(b.value)
            Npad = (N + 63) // 64 * 64
            state_bytes = slot_bytes - Npad * 8
            grad_bytes = state_bytes if w['dtype'] != 'bfloat16' else 2 * state_bytes
            fn = dev.energy_observables()
            fn.ring_alloc(K)
            fn.evaluate(0, K, 0)

            def part(which):
                engine.check(lib.mjhmc_test_energy_observables_part(fn.handle, 0, K, 0, which), lib)
            t_eval = timed(repeated(lambda: part(0), args.inner), args.reps) / args.inner
            t_red = timed(repeated(lambda: part(1), args.inner), args.reps) / args.inner
            t_both = timed(repeated(lambda: fn.evaluate(0, K, 0), args.inner), args.reps) / args.inner
            t_copy = copy_time(dev, K, args.reps, args.inner) / K
            red_bytes = state_bytes + grad_bytes + Npad * 32
            rec = dict(workload=key, D=w['D'], N=N, dtype=w['dtype'], block=K, reps=args.reps, inner=args.inner,
                       slot_bytes=slot_bytes, derived_slot_bytes=fn.slot_bytes,
                       evaluation_ms_per_state=1e3 * t_eval / K, reduction_ms_per_state=1e3 * t_red / K,
                       evaluate_call_ms_per_state=1e3 * t_both / K, copy_ms_per_slot=1e3 * t_copy,
                       copy_GBps_read_plus_write=2 * slot_bytes / t_copy / 1e9, reduction_GBps=K * red_bytes / t_red / 1e9)
            rec['reduction_fraction_of_copy_rate'] = rec['reduction_GBps'] / rec['copy_GBps_read_plus_write']
            print(rounded(rec), flush=True)
            fn.close()
            dev.close()
            del dev
            if args.replaced:
                smp, _, _ = make_sampler(key, args.n)
                t0 = time.perf_counter()
                samples = smp.sample(K, preserve_order=True)             # (D, N, K)
                t1 = time.perf_counter()
                acc = np.zeros(3)
                for k in range(K):
                    Xk = np.ascontiguousarray(samples[:, :, k])
                    E = smp.distribution.E_val(Xk)
                    G = smp.distribution.dEdX_val(Xk)
                    acc += [E.sum(), (G * G).sum(), (Xk * G).sum()]
                t2 = time.perf_counter()
                print(json.dumps(dict(workload=key, block=K, replaced_sample_ms_per_state=round(1e3 * (t1 - t0) / K, 3),
                                      replaced_eval_and_numpy_ms_per_state=round(1e3 * (t2 - t1) / K, 3))), flush=True)
                del smp, samples
    if args.temperature:
        for key in ('c5', 'c5bf16'):
            smp, w, N = make_sampler(key, args.n)
            smp.burn_in()
            t0 = time.perf_counter()
            t = smp.temperature(args.states)
            dt = time.perf_counter() - t0
            print(rounded(dict(workload=key, N=N, states=args.states, T=float(t.T), stderr=float(t.stderr), z=float(t.z),
                               ess_virial=float(t.diagnostics.ess[2]), rhat_energy=float(t.rhat_energy),
                               mean_energy=float(t.mean_energy), mean_grad_sq=float(t.mean_grad_sq),
                               temperature_ms_per_state=1e3 * dt / args.states)), flush=True)
            del smp


if __name__ == '__main__':
    main()
