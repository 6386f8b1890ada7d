"""Object wrappers over the C ABI: Context (device), DeviceEnergy, DeviceSampler.

These are plumbing; the reference-shaped API lives in mjhmc_amd.samplers / mjhmc_amd.misc.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import check, check_args, ptr, as_f64

_DTYPES = {'float64': _lib.F64, 'f64': _lib.F64, np.float64: _lib.F64, 'float32': _lib.F32, 'f32': _lib.F32,
           np.float32: _lib.F32, 'bfloat16': _lib.BF16, 'bf16': _lib.BF16}

_contexts = {}


def dtype_code(dtype):
    try:
        return _DTYPES[dtype]
    except KeyError:
        raise ValueError('dtype must be float64, float32 or bfloat16, got %r' % (dtype,))


def _lagcov_args(ndims, max_lag, shift):
    """(max_lag, shift or None, A (max_lag + 1, ndims), S (ndims,)) of a lag_cov call; the range checks are the library's"""
    max_lag = int(max_lag)
    if shift is not None:
        shift = as_f64(shift, (ndims,))
    return max_lag, shift, np.empty((max(max_lag, 0) + 1, ndims)), np.empty(ndims)


class Context(object):
    def __init__(self, device=0, lib=None):
        self.lib = lib if lib is not None else _lib.load()     # lib: _lib.load_test_hooks() in the A/B tests
        h = ctypes.c_void_p()
        check(self.lib.mjhmc_ctx_create(int(device), ctypes.byref(h)), self.lib)
        self.handle = h
        self.device = int(device)

    def info(self):
        name = ctypes.create_string_buffer(256)
        ncu = ctypes.c_int()
        hbm = ctypes.c_uint64()
        check(self.lib.mjhmc_ctx_info(self.handle, name, 256, ctypes.byref(ncu), ctypes.byref(hbm)), self.lib)
        return dict(name=name.value.decode(), n_cu=ncu.value, hbm_bytes=hbm.value)

    def mem_info(self):
        """(free, total) device memory in bytes"""
        f, t = ctypes.c_uint64(), ctypes.c_uint64()
        check(self.lib.mjhmc_mem_info(self.handle, ctypes.byref(f), ctypes.byref(t)), self.lib)
        return int(f.value), int(t.value)

    def autocor(self, samples, linear=False):
        """Lag sums ``out[k] = sum_series sum_t x_t x_{t+k}`` of a host array [n_dims, n_batch, n_samples]
        (circular in time unless ``linear``); see mjhmc_autocor in include/mjhmc_hip.h."""
        samples = np.ascontiguousarray(samples, dtype=np.float64)
        assert samples.ndim == 3
        n = samples.shape[2]
        out = np.empty(n, dtype=np.float64)
        check(self.lib.mjhmc_autocor(self.handle, ptr(samples), int(samples.shape[0] * samples.shape[1]), int(n),
                                     1 if linear else 0, ptr(out)), self.lib)
        return out

    def lag_cov(self, samples, max_lag, shift=None):
        """Per-dimension lag sums of a host array [n_dims, n_batch, n_samples]: ``(A, S)`` with ``A[k, d] = sum_p sum_t u_t
        u_{t+k}`` (linear in time, k = 0 .. max_lag <= min(n_samples - 1, 256)), ``S[d] = sum_p sum_t u_t``, u = x - shift[d]
        (``shift=None``: zeros).  The array is re-tiled on the device and read by the kernels of ``ring_lag_cov``; see
        mjhmc_lagcov in include/mjhmc_hip.h.  A refused argument raises ValueError with the library's message."""
        samples = np.ascontiguousarray(samples, dtype=np.float64)
        if samples.ndim != 3:
            raise ValueError('samples must be [n_dims, n_batch, n_samples], got shape %r' % (samples.shape,))
        D, N, n = samples.shape
        max_lag, shift, A, S = _lagcov_args(D, max_lag, shift)
        check_args(self.lib.mjhmc_lagcov(self.handle, ptr(samples), int(D), int(N), int(n), max_lag, ptr(shift), ptr(A), ptr(S)),
                   self.lib)
        return A, S

    def draw_from(self, rates, unit_exp):
        """Waiting times ``(1 / rate) * e`` (inf where the rate is 0); returns (draws, first_bad) with first_bad = -1
        or the index of the first non-finite rate (mjhmc_draw_from in include/mjhmc_hip.h)."""
        rates = np.ascontiguousarray(rates, dtype=np.float64)
        unit_exp = np.ascontiguousarray(unit_exp, dtype=np.float64)
        assert rates.ndim == 1 and unit_exp.shape == rates.shape
        out = np.empty_like(rates)
        bad = ctypes.c_int64(-1)
        rc = self.lib.mjhmc_draw_from(self.handle, ptr(rates), ptr(unit_exp), int(rates.size), ptr(out), ctypes.byref(bad))
        if rc != _lib.ERR_NONFINITE:
            check(rc, self.lib)
        return out, int(bad.value)

    def min_idx(self, draws):
        """argmin over the rows of a (k, n) float64 array per column, first minimum on ties (mjhmc_min_idx)."""
        draws = np.ascontiguousarray(draws, dtype=np.float64)
        assert draws.ndim == 2 and draws.shape[0] >= 1
        which = np.empty(draws.shape[1], dtype=np.int32)
        check(self.lib.mjhmc_min_idx(self.handle, ptr(draws), int(draws.shape[0]), int(draws.shape[1]), ptr(which)), self.lib)
        return which


TALL_MAX_EXPERTS = 2 ** 20      # mjhmc_energy_create_linear_tall
WIDE_MAX_DIMS = 4096            # mjhmc_energy_create_linear_wide


def linear_arrays(W, b, params=(), expert_params=None, _tall=False, _wide=False):
    """The checked float64 arrays of a linear-model energy: W (K, D), b (K,), params (n,), expert_params (M <= 4, K).
    Raises ValueError on a shape the device form does not take (before any device call)."""
    W = np.ascontiguousarray(W, dtype=np.float64)
    if W.ndim != 2 or W.shape[0] < 1 or W.shape[1] < 1:
        raise ValueError('W must be a (K, D) matrix, got shape %r' % (W.shape,))
    K, D = W.shape
    if _wide:
        if K > TALL_MAX_EXPERTS or D > WIDE_MAX_DIMS:
            raise ValueError('wide linear-model energies take at most 2**20 experts and 4096 dims (W is %d x %d)' % (K, D))
    elif _tall:
        if K > TALL_MAX_EXPERTS or D > 512:
            raise ValueError('tall linear-model energies take at most 2**20 experts and 512 dims (W is %d x %d)' % (K, D))
    elif K > 512 or D > 512:
        raise ValueError('linear-model energies take at most 512 experts and 512 dims (W is %d x %d)' % (K, D))
    b = np.ascontiguousarray(np.zeros(K) if b is None else b, dtype=np.float64)
    if b.shape != (K,):
        raise ValueError('b must have one entry per row of W (%d), got shape %r' % (K, b.shape))
    params = np.ascontiguousarray(np.atleast_1d(np.asarray(params, dtype=np.float64)).ravel())
    q = np.zeros((0, K)) if expert_params is None else np.asarray(expert_params, dtype=np.float64)
    if q.ndim == 1:
        q = q.reshape(1, -1)
    if q.ndim != 2 or q.shape[1] != K or q.shape[0] > 4:
        raise ValueError('expert_params must be (M <= 4, K = %d), got shape %r' % (K, q.shape))
    return W, b, params, np.ascontiguousarray(q)


def tall_linear_arrays(W, b, params=(), expert_params=None):
    """linear_arrays for a tall model (mjhmc_energy_create_linear_tall): W (K, D) with D <= 512 and K <= 2**20."""
    return linear_arrays(W, b, params, expert_params, _tall=True)


def wide_linear_arrays(W, b, params=(), expert_params=None):
    """linear_arrays for a wide model (mjhmc_energy_create_linear_wide): W (K, D) with D <= 4096 and K <= 2**20."""
    return linear_arrays(W, b, params, expert_params, _wide=True)


GROUP_MAX = 16                  # mjhmc_energy_create_linear_grouped: members of a group


def grouped_linear_arrays(W, b, groups, params=(), expert_params=None):
    """linear_arrays for a grouped model (mjhmc_energy_create_linear_grouped) and its checked ``groups`` = (C, G): the first
    G * C rows of W are G groups of C consecutive experts under a log-sum-exp; 2 <= C <= 16, G >= 1, G * C <= K."""
    W, b, params, q = linear_arrays(W, b, params, expert_params, _tall=True)
    try:
        C, G = (int(v) for v in groups)
    except (TypeError, ValueError):
        raise ValueError('groups must be (C, G): the group size and the number of groups, got %r' % (groups,))
    if C < 2 or C > GROUP_MAX:
        raise ValueError('a grouped linear model takes groups of 2 to %d experts, got C = %d' % (GROUP_MAX, C))
    if G < 1 or G * C > W.shape[0]:
        raise ValueError('a grouped linear model needs 1 <= G and G * C <= K: got G = %d, C = %d, K = %d' % (G, C, W.shape[0]))
    return W, b, params, q, (C, G)


def grouped_linear_layout(ndims, nexperts, groups, lib=None):
    """The storage order of a grouped model (mjhmc_linear_grouped_layout; needs no device): int64 (n_slots,), the caller's
    expert of every slot, -1 for padding."""
    lib = lib or _lib.load()
    C, G = groups
    n = ctypes.c_int64(0)
    check(lib.mjhmc_linear_grouped_layout(int(ndims), int(nexperts), int(C), int(G), None, ctypes.byref(n)), lib)
    out = np.empty(n.value, dtype=np.int64)
    check(lib.mjhmc_linear_grouped_layout(int(ndims), int(nexperts), int(C), int(G), ptr(out), ctypes.byref(n)), lib)
    return out


def context(device=0):
    """Process-wide context per device index."""
    if device not in _contexts:
        _contexts[device] = Context(device)
    return _contexts[device]


class DeviceEnergy(object):
    """(kind, ndims, float64 params) resident on one device."""

    def __init__(self, ctx, kind, ndims, params):
        self.ctx = ctx
        self.kind = int(kind)
        self.ndims = int(ndims)
        self.params = np.ascontiguousarray(np.atleast_1d(params), dtype=np.float64)
        h = ctypes.c_void_p()
        check(ctx.lib.mjhmc_energy_create(ctx.handle, self.kind, self.ndims, ptr(self.params), self.params.size,
                                          ctypes.byref(h)), ctx.lib)
        self.handle = h

    @classmethod
    def from_expr(cls, ctx, ndims, energy_expr, grad_expr, params=(), stats=(), energy0_expr=None):
        """An energy given as C expressions of ``x`` (coordinate), ``d`` (its index), ``p[k]`` (float64 parameters) and,
        when ``stats`` are given, ``S[k]`` (per-particle sums of the stat expressions):
            E(x) = energy0_expr(S) + sum_d energy_expr(x_d, d, S),   dE/dx_d = grad_expr(x_d, d, S);
        compiled with hipRTC around the engine's kernel templates (mjhmc_energy_create_expr[_coupled],
        include/mjhmc_hip.h)."""
        self = cls.__new__(cls)
        self.ctx = ctx
        self.kind = _lib.E_USER_EXPR
        self.ndims = int(ndims)
        self.params = np.ascontiguousarray(np.atleast_1d(np.asarray(params, dtype=np.float64)).ravel())
        stats = [stats] if isinstance(stats, str) else list(stats)
        h = ctypes.c_void_p()
        check(ctx.lib.mjhmc_energy_create_expr_coupled(
            ctx.handle, self.ndims, ';'.join(str(t) for t in stats).encode() if stats else None, str(energy_expr).encode(),
            str(energy0_expr).encode() if energy0_expr else None, str(grad_expr).encode(),
            ptr(self.params) if self.params.size else None, self.params.size, _lib.KERNEL_HEADERS.encode(), ctypes.byref(h)), ctx.lib)
        self.handle = h
        return self

    @classmethod
    def from_linear(cls, ctx, W, b, energy_expr, grad_expr, params=(), expert_params=None):
        """A linear-model energy on the ProductOfT matrix-core tile kernels (mjhmc_energy_create_linear,
        include/mjhmc_hip.h):  E(x) = sum_j f(u_j, j),  u = W x + b,  dE/dx = W^T f'(u);  W (K, D), b (K,), f / f'
        C expressions of ``u``, ``j``, ``p[k]`` (``params``) and ``q[m]`` (row m of ``expert_params``, (M <= 4, K)),
        evaluated in float32.  1 <= D, K <= 512."""
        return cls._linear(ctx, 'mjhmc_energy_create_linear', linear_arrays(W, b, params, expert_params), energy_expr, grad_expr)

    @classmethod
    def from_linear_tall(cls, ctx, W, b, energy_expr, grad_expr, params=(), expert_params=None):
        """The same form with more experts than the tile kernels hold (mjhmc_energy_create_linear_tall): W (K, D),
        1 <= D <= 512, 1 <= K <= 2**20, the experts in blocks of the padded D under one fused matrix-core kernel; ``j`` in
        the expressions is the global expert index.  Samplers of it run the engine's multi-pass path."""
        self = cls._linear(ctx, 'mjhmc_energy_create_linear_tall', tall_linear_arrays(W, b, params, expert_params), energy_expr,
                           grad_expr)
        self.tall = True
        return self

    @classmethod
    def from_linear_wide(cls, ctx, W, b, energy_expr, grad_expr, params=(), expert_params=None):
        """The same form with more dims than the tile kernels hold (mjhmc_energy_create_linear_wide): W (K, D),
        1 <= D <= 4096, 1 <= K <= 2**20, blocks of 512 experts x chunks of 512 dims under one fused matrix-core kernel; ``j``
        in the expressions is the global expert index.  Samplers of it run the engine's multi-pass path."""
        self = cls._linear(ctx, 'mjhmc_energy_create_linear_wide', wide_linear_arrays(W, b, params, expert_params), energy_expr,
                           grad_expr)
        self.wide = True
        return self

    @classmethod
    def from_linear_grouped(cls, ctx, W, b, groups, energy_expr, grad_expr, params=(), expert_params=None):
        """The tall form with a log-sum-exp over groups of experts (mjhmc_energy_create_linear_grouped):
            E(x) = sum_j f(u_j, j) + sum_{g<G} LSE_{c<C} u_{gC+c},   dE/dx = W^T (f'(u) + softmax within the groups);
        ``groups`` = (C, G): the first G * C rows of W are G groups of C consecutive experts (softmax regression: a data
        row per group, a class per member), the rest plain experts; 2 <= C <= 16, D <= 512, K <= 2**20.  ``j`` in the
        expressions is the caller's expert index.  Samplers of it run the engine's multi-pass path."""
        W, b, params, q, groups = grouped_linear_arrays(W, b, groups, params, expert_params)
        self = cls._linear(ctx, 'mjhmc_energy_create_linear_grouped', (W, b, params, q), energy_expr, grad_expr, groups)
        self.tall = True
        self.groups = groups
        return self

    @classmethod
    def _linear(cls, ctx, create, arrays, energy_expr, grad_expr, groups=()):
        """Behind from_linear, from_linear_tall, from_linear_wide and from_linear_grouped: the checked arrays (W, b, params, expert_params)
        handed to the entry point ``create``, which takes ``groups`` (C, G; the grouped form alone) behind b."""
        W, b, params, q = arrays
        self = cls.__new__(cls)
        self.ctx = ctx
        self.kind = _lib.E_LINEAR_EXPR
        self.nexperts, self.ndims = W.shape
        self.params = params
        self.W, self.b, self.expert_params = W, b, q
        h = ctypes.c_void_p()
        check(getattr(ctx.lib, create)(
            ctx.handle, self.ndims, self.nexperts, ptr(W), ptr(b), *groups, str(energy_expr).encode(), str(grad_expr).encode(),
            ptr(params) if params.size else None, params.size, ptr(q) if q.size else None, q.shape[0],
            _lib.KERNEL_HEADERS.encode(), ctypes.byref(h)), ctx.lib)
        self.handle = h
        return self

    @classmethod
    def host(cls, ctx, ndims, energy_func, energy_grad_func):
        """An energy only the caller can evaluate (MJHMC_E_HOST, include/mjhmc_hip.h): two opaque Python callables
        ``energy_func(X (D,n)) -> (n,) or (1,n)`` and ``energy_grad_func(X) -> (D,n)`` (README.md:27-36).  Samplers of it
        (HostEnergySampler) keep the state and the whole jump process on the device and call back once per leapfrog step."""
        self = cls(ctx, _lib.E_HOST, ndims, np.zeros(0))
        self.energy_func, self.energy_grad_func = energy_func, energy_grad_func
        return self

    def host_E(self, X):
        e = np.asarray(self.energy_func(X), dtype=np.float64).reshape(-1)
        if e.shape != (X.shape[1],):
            raise ValueError('energy_func must return one energy per column: got %r for X %r' % (e.shape, X.shape))
        return np.ascontiguousarray(e)

    def host_grad(self, X):
        g = np.asarray(self.energy_grad_func(X), dtype=np.float64)
        if g.shape != X.shape:
            raise ValueError('energy_grad_func must return an array shaped like X: got %r for X %r' % (g.shape, X.shape))
        return np.ascontiguousarray(g)

    def eval(self, X, want_E=True, want_grad=True, dtype='float64'):
        X = as_f64(X)
        if X.ndim != 2 or X.shape[0] != self.ndims:
            raise ValueError('X must be (ndims, n)')
        if self.kind == _lib.E_HOST:                       # the callables ARE the energy
            return (self.host_E(X) if want_E else None), (self.host_grad(X) if want_grad else None)
        n = X.shape[1]
        E = np.empty(n) if want_E else None
        G = np.empty((self.ndims, n)) if want_grad else None
        if n:
            check(self.ctx.lib.mjhmc_eval(self.handle, dtype_code(dtype), ptr(X), n, ptr(E), ptr(G)), self.ctx.lib)
        return E, G

    def leapfrog(self, X, V, epsilon, n_steps, want_grad=True, dtype='float64'):
        """n_steps leapfrog steps from (X, V) in the reference's operation order (hmc_state.py:86-100).
        Returns (X', V', EX' (n,), EV' (n,), dEdX' or None)."""
        if self.kind == _lib.E_HOST:
            raise NotImplementedError('the stand-alone leapfrog operator needs a device energy; opaque callables have none')
        X = as_f64(X)
        V = as_f64(V, X.shape)
        if X.ndim != 2 or X.shape[0] != self.ndims:
            raise ValueError('X must be (ndims, n)')
        n = X.shape[1]
        Xo, Vo = np.empty_like(X), np.empty_like(X)
        EX, EV = np.empty(n), np.empty(n)
        G = np.empty_like(X) if want_grad else None
        if n:
            check(self.ctx.lib.mjhmc_leapfrog(self.handle, dtype_code(dtype), ptr(X), ptr(V), n, float(epsilon), int(n_steps),
                                              ptr(Xo), ptr(Vo), ptr(EX), ptr(EV), ptr(G)), self.ctx.lib)
        return Xo, Vo, EX, EV, G

    def __del__(self):
        try:
            if getattr(self, 'handle', None):
                self.ctx.lib.mjhmc_energy_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


class DeviceSampler(object):
    """One shard of particle columns on one GPU."""

    def __init__(self, energy, Xinit, Vinit=None, seed=0, first_particle_id=0, dtype='float64',
                 mode=_lib.MODE_MJHMC):
        self.energy = energy
        self.ctx = energy.ctx
        self.lib = self.ctx.lib
        X = as_f64(Xinit)
        if X.ndim != 2 or X.shape[0] != energy.ndims:
            raise ValueError('Xinit must be (ndims, nparticles)')
        self.ndims, self.nparticles = X.shape
        V = None if Vinit is None else as_f64(Vinit, X.shape)
        h = ctypes.c_void_p()
        check(self.lib.mjhmc_sampler_create(self.ctx.handle, energy.handle, self.nparticles, int(first_particle_id),
                                            dtype_code(dtype), ptr(X), ptr(V), ctypes.c_uint64(int(seed) & (2 ** 64 - 1)),
                                            int(mode), ctypes.byref(h)), self.lib)
        self.handle = h
        self.ring_slots = 0

    def set_hparams(self, epsilon, num_leapfrog_steps, p_r, beta=1.0, p_flip=0.5):
        check(self.lib.mjhmc_set_hparams(self.handle, float(epsilon), int(num_leapfrog_steps), float(p_r), float(beta),
                                         float(p_flip)), self.lib)

    def iterate(self, n_iter=1, replay_normal=None, replay_exp=None, replay_unif=None, ring_slot0=-1):
        """Returns (list of IterStats for the attempts made, n_done)."""
        D, N = self.ndims, self.nparticles
        rn = None if replay_normal is None else as_f64(replay_normal).reshape(n_iter, D, N)
        re = None if replay_exp is None else as_f64(replay_exp).reshape(n_iter, 3, N)
        ru = None if replay_unif is None else as_f64(replay_unif).reshape(n_iter, 2 * N + 1)
        stats = (_lib.IterStats * n_iter)()
        done = ctypes.c_int()
        check(self.lib.mjhmc_iterate(self.handle, int(n_iter), ptr(rn), ptr(re), ptr(ru), int(ring_slot0), stats,
                                     ctypes.byref(done)), self.lib)
        n_done = done.value
        attempts = n_done + 1 if n_done < n_iter else n_iter
        return [stats[i] for i in range(attempts)], n_done

    def iterate_download(self, n_iter, ring_slot0, out, k0=0):
        """n_iter iterations into ring slots [ring_slot0, ring_slot0 + n_iter), each slot brought to
        out[:, (k0 + i) * N : (k0 + i + 1) * N] while the following iterations run (mjhmc_iterate_download).  ``out``: the
        C-contiguous float64 array (ndims, n_total * nparticles) of the whole run.  Returns (stats, n_done)."""
        D, N = self.ndims, self.nparticles
        if out.dtype != np.float64 or not out.flags.c_contiguous or out.ndim != 2 or out.shape[0] != D or out.shape[1] % N:
            raise ValueError('out must be a C-contiguous float64 array (ndims, n_total * nparticles)')
        stats = (_lib.IterStats * n_iter)()
        done = ctypes.c_int()
        check(self.lib.mjhmc_iterate_download(self.handle, int(n_iter), int(ring_slot0), ptr(out), out.shape[1] // N, int(k0), stats,
                                              ctypes.byref(done)), self.lib)
        n_done = done.value
        attempts = n_done + 1 if n_done < n_iter else n_iter
        return [stats[i] for i in range(attempts)], n_done

    def ring_slot_bytes(self):
        """device bytes of one ring slot (a padded state matrix + its dwelling times)"""
        b = ctypes.c_uint64()
        check(self.lib.mjhmc_ring_slot_bytes(self.handle, ctypes.byref(b)), self.lib)
        return int(b.value)

    def ring_budget_slots(self, n_wanted, share=0.6, staging=True, extra_bytes=0, reserve_bytes=0):
        """How many whole-state ring slots (of n_wanted) the device can take: those it already has, or `share` of the free
        memory -- at least 2 (an iteration reads one slot and writes the next).  ``staging``: every slot also gets a staging
        copy in the host layout (mjhmc_iterate_download: the streamed sample()); a ring that is recorded and then read or
        gathered from needs none.  ``extra_bytes``: what else a slot costs (a slot of a derived ring, DeviceFunctionals).
        ``reserve_bytes``: free memory spoken for (a time grid that is created once its dt is known)."""
        per = self.ring_slot_bytes() + (8 * self.ndims * self.nparticles if staging else 0) + int(extra_bytes)
        free, _ = self.ctx.mem_info()
        fit = max(int(share * max(free - int(reserve_bytes), 0) // per) + self.ring_slots, 2)
        return min(int(n_wanted), fit)

    def reset_flf_cache(self):
        check(self.lib.mjhmc_reset_flf_cache(self.handle), self.lib)

    def checkpoint(self):
        check(self.lib.mjhmc_checkpoint(self.handle), self.lib)

    def restore(self):
        check(self.lib.mjhmc_restore(self.handle), self.lib)

    def rollback(self):
        check(self.lib.mjhmc_rollback(self.handle), self.lib)

    def get_tick(self):
        t = ctypes.c_uint64()
        check(self.lib.mjhmc_get_tick(self.handle, ctypes.byref(t)), self.lib)
        return int(t.value)

    def set_tick(self, tick):
        check(self.lib.mjhmc_set_tick(self.handle, ctypes.c_uint64(int(tick))), self.lib)

    def advance_tick(self, n=1):
        check(self.lib.mjhmc_advance_tick(self.handle, int(n)), self.lib)

    def read(self, field, out=None):
        D, N = self.ndims, self.nparticles
        if out is not None:
            if field not in (_lib.F_X, _lib.F_V, _lib.F_DEDX) or out.shape != (D, N) or out.dtype != np.float64 or not out.flags.c_contiguous:
                raise ValueError('out: a C-contiguous float64 (ndims, nparticles) array for a matrix field')
        elif field in (_lib.F_X, _lib.F_V, _lib.F_DEDX):
            out = np.empty((D, N))
        elif field in (_lib.F_CACHE, _lib.F_TRANS):
            out = np.empty(N, dtype=np.uint8)
        else:
            out = np.empty(N)
        check(self.lib.mjhmc_read(self.handle, int(field), ptr(out), out.nbytes), self.lib)
        return out

    def write(self, field, arr):
        if field == _lib.F_HFLF:
            a = as_f64(np.asarray(arr, dtype=np.float64).reshape(-1), (self.nparticles,))
        else:
            a = as_f64(arr, (self.ndims, self.nparticles))
        check(self.lib.mjhmc_write(self.handle, int(field), ptr(a), a.nbytes), self.lib)

    def ring_alloc(self, n_slots):
        check(self.lib.mjhmc_ring_alloc(self.handle, int(n_slots)), self.lib)
        self.ring_slots = max(self.ring_slots, int(n_slots))

    def ring_read_dwell(self, slot0, n):
        out = np.empty((n, self.nparticles))
        check(self.lib.mjhmc_ring_read_dwell(self.handle, int(slot0), int(n), ptr(out)), self.lib)
        return out

    def ring_gather(self, idx):
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        out = np.empty((self.ndims, idx.size))
        if idx.size:
            check(self.lib.mjhmc_ring_gather(self.handle, ptr(idx), idx.size, ptr(out)), self.lib)
        return out

    def ring_read(self, slot0, n, stacked=False, out=None):
        """``out``: a caller-owned C-contiguous float64 array of the result's shape to fill (a ring of samples is GBs: a
        fresh array per call costs an allocation and a page fault per 4 KiB of it)."""
        shape = (self.ndims, self.nparticles, n) if stacked else (self.ndims, n * self.nparticles)
        if out is None:
            out = np.empty(shape)
        elif out.shape != shape or out.dtype != np.float64 or not out.flags.c_contiguous:
            raise ValueError('out must be a C-contiguous float64 array of shape %r' % (shape,))
        check(self.lib.mjhmc_ring_read(self.handle, int(slot0), int(n), 1 if stacked else 0, ptr(out)), self.lib)
        return out

    def ring_moments(self, slot0, n, shift=0.0):
        """(sum (x - shift), sum (x - shift)^2) over all state elements of ring slots [slot0, slot0 + n)."""
        a, b = ctypes.c_double(), ctypes.c_double()
        check(self.lib.mjhmc_ring_moments(self.handle, int(slot0), int(n), float(shift), ctypes.byref(a), ctypes.byref(b)), self.lib)
        return a.value, b.value

    def ring_autocor(self, slot0, n, linear=False):
        """Lag sums over time of ring slots [slot0, slot0 + n), summed over all state elements."""
        out = np.empty(int(n), dtype=np.float64)
        check(self.lib.mjhmc_ring_autocor(self.handle, int(slot0), int(n), 1 if linear else 0, ptr(out)), self.lib)
        return out

    def ring_lag_cov(self, slot0, n, max_lag, shift=None):
        """Per-dimension lag sums over time of ring slots [slot0, slot0 + n): ``(A (max_lag + 1, ndims), S (ndims,))``, see
        mjhmc_ring_lagcov in include/mjhmc_hip.h.  A refused argument raises ValueError with the library's message."""
        max_lag, shift, A, S = _lagcov_args(self.ndims, max_lag, shift)
        check_args(self.lib.mjhmc_ring_lagcov(self.handle, int(slot0), int(n), max_lag, ptr(shift), ptr(A), ptr(S)), self.lib)
        return A, S

    def ring_copy(self, src_slot, dst_slot):
        """Ring slot ``src_slot`` (state and dwelling times) copied to ``dst_slot`` on the device."""
        check(self.lib.mjhmc_ring_copy(self.handle, int(src_slot), int(dst_slot)), self.lib)

    def estimator(self, want_cov=False):
        """A weighted-moment accumulator over blocks of this sampler's ring (mjhmc_estimator_*): the sums stay on the
        device between ``accumulate`` calls, ``read`` is the only download.  The ring must exist (ring_alloc)."""
        return DeviceEstimator(self, want_cov)

    def chain_stats(self, n_parts=1):
        """Per-chain weighted sums over blocks of this sampler's ring (mjhmc_chainstats_*): what R-hat and the
        multi-chain effective sample size are made of.  ``n_parts`` = 2 keeps the two halves of a run apart (split
        R-hat).  The ring must exist (ring_alloc); the sums take n_parts * (2 * row pitch + 1) * Npad * 8 bytes."""
        return DeviceChainStats(self, n_parts)

    def histogram(self, bins, lo, hi, quantum=1.0):
        """Weighted marginal histograms over blocks of this sampler's ring (mjhmc_histogram_*): ``bins`` bins between
        ``lo`` and ``hi`` (scalars or ndims-vectors) plus an underflow and an overflow bin per dimension, integer counts
        and integer masses in units of ``quantum`` (a power of two).  The ring must exist (ring_alloc)."""
        return DeviceHistogram(self, bins, lo, hi, quantum)

    def pair_histogram(self, pairs, bins, lo, hi, quantum=1.0):
        """Weighted joint histograms of ``pairs`` [(i, j), ...] of state dimensions over blocks of this sampler's ring
        (mjhmc_pairhist_*): ``bins`` bins per axis between ``lo`` and ``hi`` (scalars or (P, 2) arrays, column 0 the i
        axis) plus an outer bin at either end of an axis, integer counts and integer masses in units of ``quantum`` (a
        power of two).  The ring must exist (ring_alloc)."""
        return DevicePairHistogram(self, pairs, bins, lo, hi, quantum)

    def occupancy(self, centres, r2=None, q=1.0):
        """Cell occupancy and transition counts of the chains over linked blocks of this sampler's ring (mjhmc_occupancy_*):
        the Voronoi cells of ``centres`` (M, ndims), 1 <= M <= 64, cut to balls of squared radius ``r2`` (an M-vector, +inf
        for none, or None), plus the cell "outside"; integer counts and integer masses in units of ``q`` (a power of
        two).  The ring must exist (ring_alloc)."""
        return DeviceOccupancy(self, centres, r2, q)

    def functionals(self, values, stats=(), params=()):
        """K values g[k] = value_k(S; p) of every recorded state, S[j] = sum_d stat_j(x_d, d; p): C expressions evaluated on
        the device into a derived ring that the estimators read (mjhmc_functionals_*).  The ring must exist (ring_alloc)."""
        return DeviceFunctionals(self, values, stats, params)

    def energy_observables(self):
        """DeviceFunctionals whose K = 3 values of every recorded state are [E, grad_sq, virial]: the potential energy as
        this sampler's evaluation kernel returns it, |dE/dX|^2 and x . dE/dX of the same evaluation
        (mjhmc_functionals_create_energy).  The ring must exist (ring_alloc); a host-evaluated energy is refused."""
        return DeviceFunctionals.energy(self)

    def projections(self, A, b=None, link=None, params=()):
        """DeviceFunctionals whose K values of every recorded state are g = link(A x + b): ``A`` (K, ndims) float64, ``b``
        (K,) or None, ``link`` one C expression of ``u``, ``k`` and ``p[m]`` or None for the identity, ``params`` the float64
        ``p`` (mjhmc_functionals_create_linear; 1 <= K <= 512).  The ring must exist (ring_alloc)."""
        return DeviceFunctionals.linear(self, A, b, link, params)

    def time_grid(self, n_grid, dt):
        """The jump process of every chain sampled at t_j = j * dt, j < n_grid, into a grid ring of this sampler's slot
        layout (mjhmc_timegrid_*): a fair sample with its time order kept.  The ring must exist (ring_alloc)."""
        return DeviceTimeGrid(self, n_grid, dt)

    def stein(self, c):
        """The kernel Stein discrepancy of one recorded ensemble against exp(-E) (mjhmc_stein_*): IMQ base kernel
        (c^2 + |x-y|^2)^(-1/2), pair pass on the device.  The ring must exist (ring_alloc); a host-evaluated energy is
        refused."""
        return DeviceStein(self, c)

    def cross_moments(self):
        """The sums of the control variates dE/dX over blocks of this sampler's ring (mjhmc_crossmoments_*): moments and
        covariance of the gradient, moments of the state and the ndims x ndims cross moments between them.  The ring must
        exist (ring_alloc); ndims <= 512; a host-evaluated energy is refused."""
        return DeviceCrossMoments(self)

    def pointwise(self, values, log_mean_exp=None):
        """Per-expert sums of 1 .. 4 value expressions h_m(u, j) of a linear-model energy over blocks of this sampler's
        ring (mjhmc_pointwise_*): u = W x + b on the matrix cores, float64 sums per expert, a log-mean-exp where
        ``log_mean_exp`` (one flag per value) asks.  The ring must exist (ring_alloc); another energy is refused."""
        return DevicePointwise(self, values, log_mean_exp)

    def group_pointwise(self, values, log_mean_exp=None, per=None):
        """Per-group ("per data row") sums of 1 .. 4 value expressions of a GROUPED linear-model energy over blocks of this
        sampler's ring (mjhmc_pointwise_create_grouped): the values see ``lse``, ``sm`` and ``c`` beside ``u``, ``j``,
        ``p[k]``, ``q[m]``; ``per`` gives each value's kind, 'group' (the default: summed over the group's members) or
        'member'.  The ring must exist (ring_alloc); an energy that is not a grouped linear model is refused."""
        return DevicePointwise(self, values, log_mean_exp, per=per, grouped=True)

    def influence(self, value, experts=None):
        """The cross moments of the state with one value h(u, j) per expert of a linear-model energy over blocks of this
        sampler's ring (mjhmc_influence_*): what Cov(x_d, h(u_j)) is made of.  ``experts``: (j0, j1), None for all.  The
        ring must exist (ring_alloc); another energy is refused."""
        return DeviceInfluence(self, value, experts)

    def last_timing(self):
        t, k, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_int()
        check(self.lib.mjhmc_last_timing(self.handle, ctypes.byref(t), ctypes.byref(k), ctypes.byref(n)), self.lib)
        return dict(total_ms=t.value, jump_kernel_ms=k.value, n_jump_launches=n.value)

    def set_timing(self, on):
        """the HIP-event pair around a call's launches (last_timing): ~8 us of every call; on by default"""
        check(self.lib.mjhmc_set_timing(self.handle, 1 if on else 0), self.lib)

    def sync(self):
        check(self.lib.mjhmc_sync(self.handle), self.lib)

    def close(self):
        if getattr(self, 'handle', None):
            self.lib.mjhmc_sampler_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _RingHandle(object):
    """The lifecycle every ring-statistics handle shares: created on the sampler's ring or, with ``on``, on the derived
    ring of a DeviceFunctionals, and closed once.  ``_kind`` names the mjhmc_<kind>_* entry points."""
    _kind = None
    on = None

    def _create(self, dev, on, *args, checker=check):
        """mjhmc_<kind>_create(dev, *args, &handle), or mjhmc_<kind>_create_on(on, *args, &handle); ``checker``:
        check_args where the wrapper promises ValueError for a refused argument"""
        self.dev, self.lib, self.on = dev, dev.lib, on
        h = ctypes.c_void_p()
        create = getattr(self.lib, 'mjhmc_%s_create%s' % (self._kind, '' if on is None else '_on'))
        checker(create((dev if on is None else on).handle, *(args + (ctypes.byref(h),))), self.lib)
        self.handle = h

    def _call(self, name, *args):
        check(getattr(self.lib, 'mjhmc_%s_%s' % (self._kind, name))(self.handle, *args), self.lib)

    def close(self):
        if getattr(self, 'handle', None) and getattr(self.dev, 'handle', None) and \
                (getattr(self, 'on', None) is None or self.on.handle):   # (a closed sampler or functionals freed it already)
            getattr(self.lib, 'mjhmc_%s_destroy' % self._kind)(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _RingAccumulator(_RingHandle):
    """A handle whose sums stay on the device between ``accumulate`` calls over blocks of the ring, until ``reset``"""

    def reset(self):
        self._call('reset')

    def accumulate(self, x_slot0, n, w_slot0=-1):
        """States of ring slots [x_slot0, x_slot0 + n), weights of dwell slots [w_slot0, w_slot0 + n) (-1: unit weights;
        a jump sampler's time average takes w_slot0 = x_slot0 + 1).  What a class refuses is in its own docstring."""
        self._call('accumulate', int(x_slot0), int(w_slot0), int(n))


class DeviceEstimator(_RingAccumulator):
    """W = sum w, S1 = sum w (x - c), S2 = sum w (x - c)^2 and, with ``want_cov``, C = sum w (x - c)(x - c)^T over the
    (slot, particle) states of the ring blocks given to ``accumulate``; float64 throughout, bit-identical from run to run."""
    _kind = 'estimator'

    def __init__(self, dev, want_cov=False, on=None):
        """``on``: a DeviceFunctionals of ``dev`` whose derived ring the states are read from (its K values are the
        dimensions; x_slot0 then counts derived slots, w_slot0 still the sampler's dwell slots)"""
        self.want_cov = bool(want_cov)
        self.ndims = dev.ndims if on is None else on.n_values
        self._create(dev, on, 1 if want_cov else 0)

    def set_shift(self, c=None):
        c = None if c is None else as_f64(np.asarray(c, dtype=np.float64).reshape(-1), (self.ndims,))
        check(self.lib.mjhmc_estimator_set_shift(self.handle, ptr(c)), self.lib)

    def read(self):
        """(W, S1 (D,), S2 (D,), C (D, D) or None, n_states)"""
        D = self.ndims
        W, n = ctypes.c_double(), ctypes.c_int64()
        S1, S2 = np.empty(D), np.empty(D)
        C = np.empty((D, D)) if self.want_cov else None
        check(self.lib.mjhmc_estimator_read(self.handle, ctypes.byref(W), ptr(S1), ptr(S2), ptr(C), ctypes.byref(n)), self.lib)
        return W.value, S1, S2, C, int(n.value)


class DeviceCrossMoments(_RingAccumulator):
    """The sums of the control variates g = dE/dX (include/mjhmc_hip.h: mjhmc_crossmoments_*): W = sum w, Sg = sum w g,
    S2g = sum w g^2, Cgg = sum w g g^T (the gradient about 0, its known mean), Sb = sum w (b - cb), S2b = sum w (b - cb)^2 and
    Cgb = sum w g (b - cb)^T over the (slot, particle) states given to ``accumulate``, b the state itself or, with ``on``,
    the K values of a DeviceFunctionals; float64 throughout, bit-identical from run to run and whatever the blocks.
    ``accumulate``: a weight that is not finite raises and adds nothing; a state, gradient or energy that is not finite
    raises naming the slot, and the handle refuses until ``reset``."""
    _kind = 'crossmoments'

    def __init__(self, dev, on=None):
        """``on``: a DeviceFunctionals of ``dev`` whose derived ring b is read from (x_slot0 then counts slots of both rings)"""
        self._create(dev, on)
        d, k = ctypes.c_int(), ctypes.c_int()
        self._call('info', ctypes.byref(d), ctypes.byref(k))
        self.ndims, self.n_values = int(d.value), int(k.value)

    def set_shift(self, cb=None):
        cb = None if cb is None else as_f64(np.asarray(cb, dtype=np.float64).reshape(-1), (self.n_values,))
        self._call('set_shift', ptr(cb))

    def read(self):
        """(W, Sg (D,), S2g (D,), Sb (K,), S2b (K,), Cgg (D, D), Cgb (D, K), n_states)"""
        D, K = self.ndims, self.n_values
        W, n = ctypes.c_double(), ctypes.c_int64()
        Sg, S2g, Sb, S2b, Cgg, Cgb = np.empty(D), np.empty(D), np.empty(K), np.empty(K), np.empty((D, D)), np.empty((D, K))
        self._call('read', ctypes.byref(W), ptr(Sg), ptr(S2g), ptr(Sb), ptr(S2b), ptr(Cgg), ptr(Cgb), ctypes.byref(n))
        return W.value, Sg, S2g, Sb, S2b, Cgg, Cgb, int(n.value)


POINTWISE_MAX_VALUES = 4


def pointwise_args(values, log_mean_exp=None):
    """(the ';'-separated bytes of 1 .. 4 value expressions, the log-mean-exp bit mask) of a DevicePointwise; ValueError
    for no value, more than 4, an empty one or one with a semicolon, and for flags that do not pair with the values"""
    values = [values] if isinstance(values, str) else [str(v) for v in values]
    if not 1 <= len(values) <= POINTWISE_MAX_VALUES:
        raise ValueError('the pointwise statistics take 1 to %d value expressions, got %d' % (POINTWISE_MAX_VALUES, len(values)))
    flags = [False] * len(values) if log_mean_exp is None else [bool(f) for f in np.atleast_1d(log_mean_exp)]
    if len(flags) != len(values):
        raise ValueError('log_mean_exp must have one flag per value (%d), got %d' % (len(values), len(flags)))
    return join_exprs(values), sum(1 << m for m, f in enumerate(flags) if f)


def pointwise_check(ndims, nexperts, values):
    """Compile the pointwise kernel of an (ndims, nexperts) linear model around ``values`` with no device
    (mjhmc_pointwise_check); a refused or uncompilable expression raises ValueError with the compiler's message."""
    check_args(_lib.load().mjhmc_pointwise_check(int(ndims), int(nexperts), pointwise_args(values)[0],
                                                 _lib.KERNEL_HEADERS.encode()))


GROUP_POINTWISE_KINDS = ('group', 'member')


def group_pointwise_args(values, log_mean_exp=None, per=None):
    """(the ';'-separated bytes of 1 .. 4 value expressions, the log-mean-exp bit mask, the per-member bit mask) of a
    grouped DevicePointwise; ValueError as pointwise_args, and for a ``per`` that does not pair with the values or holds a
    word other than 'group' / 'member' (None: every value per group)"""
    exprs, lme = pointwise_args(values, log_mean_exp)
    n = 1 if isinstance(values, str) else len(values)
    kinds = ['group'] * n if per is None else ([per] if isinstance(per, str) else [str(k) for k in per])
    if len(kinds) != n:
        raise ValueError('per must have one kind per value (%d), got %d' % (n, len(kinds)))
    for k in kinds:
        if k not in GROUP_POINTWISE_KINDS:
            raise ValueError("per: a value is per 'group' or per 'member', got %r" % (k,))
    return exprs, lme, sum(1 << m for m, k in enumerate(kinds) if k == 'member')


def group_pointwise_check(ndims, nexperts, groups, values, per=None):
    """Compile the per-group kernel of an (ndims, nexperts) linear model with ``groups`` = (C, G) around ``values`` with no
    device (mjhmc_pointwise_grouped_check); a refused or uncompilable expression raises ValueError with the compiler's
    message."""
    exprs, _, member = group_pointwise_args(values, None, per)
    check_args(_lib.load().mjhmc_pointwise_grouped_check(int(ndims), int(nexperts), int(groups[0]), int(groups[1]), exprs,
                                                         member, _lib.KERNEL_HEADERS.encode()))


class DevicePointwise(_RingAccumulator):
    """Per expert j of a linear-model energy and per value m: W = sum w, S1 = sum w t, S2 = sum (w t) t and, where
    ``log_mean_exp`` asks, (mx, se) with mx = max t and se = sum w exp(t - mx), t = h_m(u_j, j) over the (slot, particle)
    states of the ring blocks given to ``accumulate`` (include/mjhmc_hip.h: mjhmc_pointwise_*).  u = W x + b is formed on
    the matrix cores and never stored; float64 sums, bit-identical from run to run and whatever the blocks.
    ``accumulate``: a weight that is negative or not finite, or a value that is not finite at a state of positive weight,
    raises EngineError (status -5) and adds nothing."""
    _kind = 'pointwise'

    def __init__(self, dev, values, log_mean_exp=None, per=None, grouped=False):
        """``grouped``: the per-group pass of a grouped linear model (mjhmc_pointwise_create_grouped) with the kinds ``per``
        of its values -- the same handle with columns in place of experts: ``nexperts`` is G C when a value is per member
        and G otherwise, a per-group value fills the first G columns of its row and the rest read as empty"""
        if grouped:
            exprs, mask, member = group_pointwise_args(values, log_mean_exp, per)
            self.member_mask = member
            self._create_grouped(dev, exprs, mask, member)
        else:
            exprs, mask = pointwise_args(values, log_mean_exp)
            self._create(dev, None, exprs, mask, _lib.KERNEL_HEADERS.encode(), checker=check_args)
        m, k, t = ctypes.c_int(), ctypes.c_int64(), ctypes.c_int()
        self._call('info', ctypes.byref(m), ctypes.byref(k), ctypes.byref(t))
        self.n_values, self.nexperts, self.strip_tiles = int(m.value), int(k.value), int(t.value)

    def _create_grouped(self, dev, exprs, mask, member):
        self.dev, self.lib, self.on = dev, dev.lib, None
        h = ctypes.c_void_p()
        check_args(self.lib.mjhmc_pointwise_create_grouped(dev.handle, exprs, mask, member, _lib.KERNEL_HEADERS.encode(),
                                                           ctypes.byref(h)), self.lib)
        self.handle = h

    def read(self):
        """(W, S1 (M, K), S2 (M, K), lme_max (M, K), lme_sum (M, K), n_states)"""
        shape = (self.n_values, self.nexperts)
        W, n = ctypes.c_double(), ctypes.c_int64()
        S1, S2, mx, se = np.empty(shape), np.empty(shape), np.empty(shape), np.empty(shape)
        self._call('read', ctypes.byref(W), ptr(S1), ptr(S2), ptr(mx), ptr(se), ctypes.byref(n))
        return W.value, S1, S2, mx, se, int(n.value)


def influence_args(value):
    """the bytes of the ONE value expression of a DeviceInfluence; ValueError for none, an empty one or more than one"""
    values = [value] if isinstance(value, str) else [str(v) for v in value]
    if len(values) != 1:
        raise ValueError('the influence pass takes one value expression per pass, got %d' % len(values))
    return join_exprs(values)


def influence_check(ndims, nexperts, value):
    """Compile the stored-values kernel of an (ndims, nexperts) linear model around ``value`` with no device
    (mjhmc_influence_check); a refused or uncompilable expression raises ValueError with the compiler's message."""
    check_args(_lib.load().mjhmc_influence_check(int(ndims), int(nexperts), influence_args(value),
                                                 _lib.KERNEL_HEADERS.encode()))


class DeviceInfluence(_RingAccumulator):
    """The cross moments of the state with ONE value t_j = h(u_j, j) per expert j0 <= j < j1 of a linear-model energy
    (include/mjhmc_hip.h: mjhmc_influence_*): W = sum w, Sx = sum w (x - cx), S2x = sum w (x - cx)^2, St = sum w (t - ct),
    S2t = sum w (t - ct)^2 and Cxt = sum w x (t - ct)^T over the (slot, particle) states given to ``accumulate``.  u = W x + b
    is formed on the matrix cores panel of experts by panel; float64 sums, bit-identical from run to run and whatever the
    blocks.  ``accumulate``: a weight that is negative or not finite raises EngineError (status -5) and adds nothing; a
    value that is not finite at a state of positive weight raises naming the lowest expert, and the handle refuses until
    ``reset``."""
    _kind = 'influence'

    def __init__(self, dev, value, experts=None):
        expr = influence_args(value)
        if experts is None:                                # all of them (an energy without experts is refused by name below)
            experts = (0, int(getattr(dev.energy, 'nexperts', 0)))
        self._create(dev, None, expr, int(experts[0]), int(experts[1]), _lib.KERNEL_HEADERS.encode(), checker=check_args)
        d, a, b, p, sb = ctypes.c_int(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int(), ctypes.c_int64()
        self._call('info', ctypes.byref(d), ctypes.byref(a), ctypes.byref(b), ctypes.byref(p), ctypes.byref(sb))
        self.ndims, self.experts = int(d.value), (int(a.value), int(b.value))
        self.panel_experts, self.scratch_bytes = int(p.value), int(sb.value)
        self.n_values = self.experts[1] - self.experts[0]

    def set_shift(self, cx=None, ct=None):
        """the shifts of the state sums and of the value sums (None: zero); only while the handle is empty"""
        cx = None if cx is None else as_f64(np.asarray(cx, dtype=np.float64).reshape(-1), (self.ndims,))
        ct = None if ct is None else as_f64(np.asarray(ct, dtype=np.float64).reshape(-1), (self.n_values,))
        check_args(self.lib.mjhmc_influence_set_shift(self.handle, ptr(cx), ptr(ct)), self.lib)

    def read(self):
        """(W, Sx (D,), S2x (D,), St (J,), S2t (J,), n_states), J = j1 - j0"""
        D, J = self.ndims, self.n_values
        W, n = ctypes.c_double(), ctypes.c_int64()
        Sx, S2x, St, S2t = np.empty(D), np.empty(D), np.empty(J), np.empty(J)
        self._call('read', ctypes.byref(W), ptr(Sx), ptr(S2x), ptr(St), ptr(S2t), ctypes.byref(n))
        return W.value, Sx, S2x, St, S2t, int(n.value)

    def read_cross(self, ja=None, jb=None):
        """Cxt (D, jb - ja): the columns of the experts ja <= j < jb (None: the handle's own range)"""
        ja = self.experts[0] if ja is None else int(ja)
        jb = self.experts[1] if jb is None else int(jb)
        if not self.experts[0] <= ja < jb <= self.experts[1]:
            raise ValueError('columns [%d, %d) are not a range inside the experts [%d, %d)' % ((ja, jb) + self.experts))
        C = np.empty((self.ndims, jb - ja))
        self._call('read_cross', ja, jb, ptr(C))
        return C


class DeviceChainStats(_RingAccumulator):
    """Per chain (particle) p and part h: a0 = sum_k w, a1 = sum_k w (x - c), a2 = sum_k w (x - c)^2 over the states
    of the ring blocks given to ``accumulate``, in float64 and in a fixed operation order (include/mjhmc_hip.h:
    mjhmc_chainstats_accumulate): bit-identical to the same float64 operations on the host, whatever the blocks."""
    _kind = 'chainstats'

    def __init__(self, dev, n_parts=1, on=None):
        """``on``: a DeviceFunctionals of ``dev`` whose derived ring the states are read from (see DeviceEstimator)"""
        self.n_parts = int(n_parts)
        self.ndims, self.nparticles = (dev.ndims if on is None else on.n_values), dev.nparticles
        self._create(dev, on, self.n_parts)

    def set_shift(self, c=None):
        c = None if c is None else as_f64(np.asarray(c, dtype=np.float64).reshape(-1), (self.ndims,))
        check(self.lib.mjhmc_chainstats_set_shift(self.handle, ptr(c)), self.lib)

    def accumulate(self, x_slot0, n, w_slot0=-1, part=0):
        """States of ring slots [x_slot0, x_slot0 + n) added to the chains' sums of ``part``, weights of dwell slots
        [w_slot0, w_slot0 + n) (-1: unit weights; a jump sampler's time average takes w_slot0 = x_slot0 + 1)."""
        check(self.lib.mjhmc_chainstats_accumulate(self.handle, int(part), int(x_slot0), int(w_slot0), int(n)), self.lib)

    def read(self, part=0):
        """The fold of one part over its chains: (n_chains, n_states_per_chain, Sw, Sm (D,), Sq (D,), Sv (D,)) = the
        number of chains, the states each has, and the sums over chains of a0, of the chain means m = a1 / a0, of m^2
        and of the chain variances a2 / a0 - m^2."""
        D = self.ndims
        M, n, Sw = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_double()
        Sm, Sq, Sv = np.empty(D), np.empty(D), np.empty(D)
        check(self.lib.mjhmc_chainstats_read(self.handle, int(part), ctypes.byref(M), ctypes.byref(n), ctypes.byref(Sw),
                                             ptr(Sm), ptr(Sq), ptr(Sv)), self.lib)
        return int(M.value), int(n.value), Sw.value, Sm, Sq, Sv

    def read_chains(self, part=0):
        """(a0 (N,), a1 (D, N), a2 (D, N)): the per-chain sums themselves, an O(N * D) download"""
        D, N = self.ndims, self.nparticles
        a0, a1, a2 = np.empty(N), np.empty((D, N)), np.empty((D, N))
        check(self.lib.mjhmc_chainstats_read_chains(self.handle, int(part), ptr(a0), ptr(a1), ptr(a2)), self.lib)
        return a0, a1, a2


class DeviceHistogram(_RingAccumulator):
    """Per dimension d and bin b: count[d][b] states and mass[d][b] = sum of rint(w / quantum) over the (slot, particle)
    states of the ring blocks given to ``accumulate`` whose element x_d falls into bin b -- b = 0 below ``lo`` (and NaN),
    bins + 1 from ``hi`` on, 1 + int((x - lo) * (bins / (hi - lo))) between (include/mjhmc_hip.h: mjhmc_histogram_create).
    Integer sums: bit-identical from run to run, whatever the blocks.  ``accumulate``: a refused block (a weight that is
    not finite, negative or too large for the quantum) raises and adds nothing."""
    _kind = 'histogram'

    def __init__(self, dev, bins, lo, hi, quantum=1.0, on=None):
        """``on``: a DeviceFunctionals of ``dev`` whose derived ring the states are read from (see DeviceEstimator)"""
        self.ndims, self.bins, self.quantum = (dev.ndims if on is None else on.n_values), int(bins), float(quantum)
        self.lo = as_f64(np.broadcast_to(np.asarray(lo, dtype=np.float64), (self.ndims,)))
        self.hi = as_f64(np.broadcast_to(np.asarray(hi, dtype=np.float64), (self.ndims,)))
        self._create(dev, on, self.bins, ptr(self.lo), ptr(self.hi), self.quantum)

    def read(self):
        """(count (D, bins + 2) uint64, mass (D, bins + 2) uint64 in units of the quantum, W_units, n_states)"""
        shape = (self.ndims, self.bins + 2)
        count, mass = np.empty(shape, dtype=np.uint64), np.empty(shape, dtype=np.uint64)
        W, n = ctypes.c_uint64(), ctypes.c_int64()
        check(self.lib.mjhmc_histogram_read(self.handle, ptr(count), ptr(mass), ctypes.byref(W), ctypes.byref(n)), self.lib)
        return count, mass, int(W.value), int(n.value)


class DeviceTimeGrid(_RingAccumulator):
    """Per chain p a clock T[p] and a cursor j[p]; ``accumulate`` walks a block of ring slots in order and copies the state
    that holds at t_j = j * dt into grid slot j for every grid point its holding time covers (include/mjhmc_hip.h:
    mjhmc_timegrid_accumulate).  Grid, clocks and cursors are bit-identical to that sequence of float64 operations on the
    host, whatever the blocks."""
    _kind = 'timegrid'

    def __init__(self, dev, n_grid, dt):
        self.ndims, self.nparticles = dev.ndims, dev.nparticles
        self.n_grid, self.dt = int(n_grid), float(dt)
        self._create(dev, None, self.n_grid, self.dt)

    def accumulate(self, x_slot0, n, w_slot0=-1):
        """States of ring slots [x_slot0, x_slot0 + n), holding times of dwell slots [w_slot0, w_slot0 + n) (-1: unit holding
        times; a jump sampler takes w_slot0 = x_slot0 + 1).  A refused block (a holding time that is not finite or is
        negative) raises and changes nothing."""
        self._call('accumulate', int(x_slot0), int(n), int(w_slot0))

    def progress(self):
        """(covered, max_filled): the grid slots complete for every chain, and for the chain that got furthest"""
        c, m = ctypes.c_int(), ctypes.c_int()
        check(self.lib.mjhmc_timegrid_progress(self.handle, ctypes.byref(c), ctypes.byref(m)), self.lib)
        return int(c.value), int(m.value)

    def read_clocks(self):
        """(T (N,) float64, j (N,) int32)"""
        T, j = np.empty(self.nparticles), np.empty(self.nparticles, dtype=np.int32)
        check(self.lib.mjhmc_timegrid_read_clocks(self.handle, ptr(T), ptr(j)), self.lib)
        return T, j

    def read(self, slot0, n, stacked=True):
        """grid slots [slot0, slot0 + n): (ndims, nparticles, n) if ``stacked``, else (ndims, n * nparticles) time-major"""
        n = int(n)
        out = np.empty((self.ndims, self.nparticles, n) if stacked else (self.ndims, n * self.nparticles))
        check(self.lib.mjhmc_timegrid_read(self.handle, int(slot0), n, 1 if stacked else 0, ptr(out)), self.lib)
        return out

    def autocor(self, slot0, n, linear=False):
        """Lag sums over time of grid slots [slot0, slot0 + n) (all of them covered), summed over all state elements."""
        out = np.empty(int(n), dtype=np.float64)
        check(self.lib.mjhmc_timegrid_autocor(self.handle, int(slot0), int(n), 1 if linear else 0, ptr(out)), self.lib)
        return out

    def lag_cov(self, slot0, n, max_lag, shift=None):
        """Per-dimension lag sums over time of grid slots [slot0, slot0 + n) (all of them covered): ``(A (max_lag + 1, ndims),
        S (ndims,))``, see mjhmc_grid_lagcov in include/mjhmc_hip.h.  A refused argument raises ValueError with the
        library's message."""
        max_lag, shift, A, S = _lagcov_args(self.ndims, max_lag, shift)
        check_args(self.lib.mjhmc_grid_lagcov(self.handle, int(slot0), int(n), max_lag, ptr(shift), ptr(A), ptr(S)), self.lib)
        return A, S


class DeviceStein(_RingHandle):
    """``evaluate`` returns (W, W2, S, Sd) of one ring slot: W = sum w, W2 = sum w^2, S = sum_ij w_i w_j k_p(x_i, x_j), Sd its
    diagonal, k_p the Stein kernel of the IMQ base kernel with scale ``c`` (include/mjhmc_hip.h: mjhmc_stein_evaluate).
    Float64 throughout, no floating-point atomics: bit-identical from run to run."""
    _kind = 'stein'

    def __init__(self, dev, c):
        self.c = float(c)
        self._create(dev, None, self.c, checker=check_args)

    def evaluate(self, x_slot, w_slot=-1, n_use=None):
        """The first ``n_use`` particles (default: all) of ring slot ``x_slot`` with the weights of dwell slot ``w_slot`` (-1:
        unit weights; a jump sampler takes w_slot = x_slot + 1).  A weight, state or gradient that is not finite raises
        EngineError (status -5) with a message that says which."""
        n_use = self.dev.nparticles if n_use is None else int(n_use)
        out = np.empty(4, dtype=np.float64)
        check_args(self.lib.mjhmc_stein_evaluate(self.handle, int(x_slot), int(w_slot), n_use, ptr(out)), self.lib)
        return tuple(float(v) for v in out)


class DevicePairHistogram(_RingAccumulator):
    """Per pair p = (i, j) and cell (b_j, b_i): count[p][b_j][b_i] states and mass[p][b_j][b_i] = sum of rint(w / quantum)
    over the (slot, particle) states of the ring blocks given to ``accumulate`` whose elements x_i, x_j fall into bins b_i,
    b_j of their axes -- per axis the bins of DeviceHistogram (include/mjhmc_hip.h: mjhmc_pairhist_create).  Integer sums:
    bit-identical from run to run, whatever the blocks.  ``accumulate`` refuses what DeviceHistogram's refuses."""
    _kind = 'pairhist'

    def __init__(self, dev, pairs, bins, lo, hi, quantum=1.0, on=None):
        """``on``: a DeviceFunctionals of ``dev`` whose derived ring the states are read from (see DeviceEstimator)"""
        self.ndims, self.bins, self.quantum = (dev.ndims if on is None else on.n_values), int(bins), float(quantum)
        self.pairs = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
        self.n_pairs = P = self.pairs.shape[0]
        self.lo = as_f64(np.broadcast_to(np.asarray(lo, dtype=np.float64), (P, 2)))
        self.hi = as_f64(np.broadcast_to(np.asarray(hi, dtype=np.float64), (P, 2)))
        self._create(dev, on, P, ptr(self.pairs), self.bins, ptr(self.lo), ptr(self.hi), self.quantum)

    def read(self):
        """(count (P, bins + 2, bins + 2) uint64, mass likewise in units of the quantum, W_units, n_states); the last
        axis is the pair's first dimension"""
        shape = (self.n_pairs, self.bins + 2, self.bins + 2)
        count, mass = np.empty(shape, dtype=np.uint64), np.empty(shape, dtype=np.uint64)
        W, n = ctypes.c_uint64(), ctypes.c_int64()
        check(self.lib.mjhmc_pairhist_read(self.handle, ptr(count), ptr(mass), ctypes.byref(W), ctypes.byref(n)), self.lib)
        return count, mass, int(W.value), int(n.value)


class DeviceOccupancy(_RingAccumulator):
    """Per cell a of the M + 1 cells (the Voronoi cells of the M centres, cut to the balls of squared radius ``r2`` where
    one is given, and cell M, "outside"): count[a] states, mass[a] = sum of rint(w / q), and per pair of cells trans[a][b]
    consecutive states of one chain, over the ring blocks given to ``accumulate`` in chain order; per chain the number of
    switches and the cells seen (include/mjhmc_hip.h: mjhmc_occupancy_create).  Integer sums: bit-identical from run to
    run, whatever the blocks.  ``accumulate`` refuses what DeviceHistogram's refuses, and a refused block leaves the
    chains where they were."""
    _kind = 'occupancy'

    def __init__(self, dev, centres, r2=None, q=1.0, on=None):
        """``on``: a DeviceFunctionals of ``dev`` whose derived ring the states are read from (see DeviceEstimator)"""
        self.centres = np.ascontiguousarray(np.asarray(centres, dtype=np.float64))
        if self.centres.ndim != 2:
            raise ValueError('centres must be (M, K), got an array of shape %r' % (self.centres.shape,))
        self.n_centres, self.ndims = self.centres.shape
        self.r2 = None if r2 is None else as_f64(np.broadcast_to(np.asarray(r2, dtype=np.float64), (self.n_centres,)))
        self.quantum = float(q)
        self.nparticles = dev.nparticles
        self._create(dev, on, self.n_centres, self.ndims, ptr(self.centres), ptr(self.r2), self.quantum, checker=check_args)

    def accumulate(self, x_slot0, n, w_slot0=-1, linked=False):
        """``linked``: slot ``x_slot0`` follows the last state of the previous block (its pair is counted); False starts
        new chains there"""
        self._call('accumulate', int(x_slot0), int(w_slot0), int(n), 1 if linked else 0)

    def read(self, chains=False):
        """dict of uint64 arrays: count, mass, from_count, from_mass (M + 1,), trans (M + 1, M + 1), chains_by_switches
        (17,), chains_by_cells (M + 1,), and the ints W_units, n_states; ``chains=True`` adds switches (N,) uint32 and
        visited (N,) uint64, an O(N) download"""
        C, N = self.n_centres + 1, self.nparticles
        out = dict((k, np.zeros(C, dtype=np.uint64)) for k in ('count', 'mass', 'from_count', 'from_mass', 'chains_by_cells'))
        out['trans'] = np.zeros((C, C), dtype=np.uint64)
        out['chains_by_switches'] = np.zeros(17, dtype=np.uint64)
        sw = np.zeros(N, dtype=np.uint32) if chains else None
        vis = np.zeros(N, dtype=np.uint64) if chains else None
        W, n = ctypes.c_uint64(), ctypes.c_int64()
        self._call('read', ptr(out['count']), ptr(out['mass']), ptr(out['from_count']), ptr(out['from_mass']), ptr(out['trans']),
                   ctypes.byref(W), ptr(out['chains_by_switches']), ptr(out['chains_by_cells']), ptr(sw), ptr(vis), ctypes.byref(n))
        out['W_units'], out['n_states'] = int(W.value), int(n.value)
        if chains:
            out['switches'], out['visited'] = sw, vis
        return out

    def read_labels(self, n):
        """(n, N) uint8: the labels of the first ``n`` slots of the last block given to ``accumulate``"""
        out = np.zeros((int(n), self.nparticles), dtype=np.uint8)
        self._call('read_labels', int(n), ptr(out))
        return out

    def info(self):
        """(M, K, the slots the label scratch holds)"""
        m, k, sl = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        self._call('info', ctypes.byref(m), ctypes.byref(k), ctypes.byref(sl))
        return int(m.value), int(k.value), int(sl.value)


def join_exprs(exprs):
    """one expression or a sequence of them -> the ';'-separated bytes the C ABI takes (None for none)"""
    exprs = [exprs] if isinstance(exprs, str) else list(exprs)
    for e in exprs:
        if ';' in str(e) or not str(e).strip():
            raise ValueError('an expression is empty or holds a semicolon: %r' % (e,))
    return ';'.join(str(e) for e in exprs).encode() if exprs else None


class DeviceFunctionals(_RingHandle):
    """K float64 values of every recorded state of a sampler, g[k] = value_k(S; p) with S[j] = sum_d stat_j(x_d, d; p),
    evaluated by one device pass from blocks of the sampler's ring into a derived ring of K-dimensional states
    (include/mjhmc_hip.h: mjhmc_functionals_create).  ``estimator``, ``chain_stats``, ``histogram`` and ``pair_histogram`` give the sampler's
    accumulators on the derived ring: their ``x_slot0`` counts derived slots, ``w_slot0`` the sampler's dwell slots."""
    _kind = 'functionals'

    def __init__(self, dev, values, stats=(), params=(), _energy=False, _linear=None):
        self.dev, self.lib = dev, dev.lib
        self.nparticles = dev.nparticles
        self.params = np.ascontiguousarray(np.atleast_1d(np.asarray(params, dtype=np.float64)).ravel())
        h = ctypes.c_void_p()
        if _linear is not None:
            A, b, link = _linear
            A = np.ascontiguousarray(np.asarray(A, dtype=np.float64))
            if A.ndim != 2 or A.shape[1] != dev.ndims:
                raise ValueError('A must be (K, ndims = %d), got %r' % (dev.ndims, A.shape))
            if b is not None:
                b = np.ascontiguousarray(np.broadcast_to(np.asarray(b, dtype=np.float64), (A.shape[0],)))
            check_args(self.lib.mjhmc_functionals_create_linear(dev.handle, A.shape[0], ptr(A), ptr(b),
                                                                None if link is None else str(link).encode(),
                                                           ptr(self.params) if self.params.size else None, self.params.size,
                                                           _lib.KERNEL_HEADERS.encode(), ctypes.byref(h)), self.lib)
        elif _energy:
            # (its fixed scratch -- dE/dX and E of one slot, at most about two slots' bytes -- is taken here, from the 40 %
            # of free memory that ring_budget_slots(share=0.6) leaves beside the rings)
            check(self.lib.mjhmc_functionals_create_energy(dev.handle, ctypes.byref(h)), self.lib)
        else:
            check(self.lib.mjhmc_functionals_create(dev.handle, join_exprs(stats), join_exprs(values),
                                                    ptr(self.params) if self.params.size else None, self.params.size,
                                                    _lib.KERNEL_HEADERS.encode(), ctypes.byref(h)), self.lib)
        self.handle = h
        k, b = ctypes.c_int(), ctypes.c_uint64()
        self._call('info', ctypes.byref(k), ctypes.byref(b))
        self.n_values, self.slot_bytes = int(k.value), int(b.value)
        self.ring_slots = 0

    @classmethod
    def energy(cls, dev):
        """the energy observables [E, grad_sq, virial] of ``dev``'s recorded states (mjhmc_functionals_create_energy): the
        same handle family, filled by the sampler's own evaluation kernels instead of compiled expressions"""
        return cls(dev, (), _energy=True)

    @classmethod
    def linear(cls, dev, A, b=None, link=None, params=()):
        """the linear projections g = link(A x + b) of ``dev``'s recorded states (mjhmc_functionals_create_linear): the
        same handle family, filled by the small-GEMM kernel of csrc/projections.hpp"""
        return cls(dev, (), params=params, _linear=(A, b, link))

    def ring_alloc(self, n_slots):
        """at least ``n_slots`` derived slots; a ring that grows is a new ring (handles created on the old one refuse)"""
        self._call('ring_alloc', int(n_slots))
        self.ring_slots = max(self.ring_slots, int(n_slots))

    def evaluate(self, x_slot0, n, out_slot0=0):
        """derived slots [out_slot0, out_slot0 + n) from the sampler's ring slots [x_slot0, x_slot0 + n); raises
        EngineError (MJHMC_ERR_NONFINITE) naming the value when one is not finite"""
        self._call('evaluate', int(x_slot0), int(n), int(out_slot0))

    def read(self, slot0, n):
        """(K, n, N): the values of derived slots [slot0, slot0 + n)"""
        out = np.empty((self.n_values, int(n), self.nparticles))
        self._call('read', int(slot0), int(n), ptr(out))
        return out

    def estimator(self, want_cov=False):
        return DeviceEstimator(self.dev, want_cov, on=self)

    def chain_stats(self, n_parts=1):
        return DeviceChainStats(self.dev, n_parts, on=self)

    def histogram(self, bins, lo, hi, quantum=1.0):
        return DeviceHistogram(self.dev, bins, lo, hi, quantum, on=self)

    def pair_histogram(self, pairs, bins, lo, hi, quantum=1.0):
        return DevicePairHistogram(self.dev, pairs, bins, lo, hi, quantum, on=self)

    def occupancy(self, centres, r2=None, q=1.0):
        """the sampler's DeviceOccupancy with the cells in the space of the K values of this derived ring"""
        return DeviceOccupancy(self.dev, centres, r2, q, on=self)

    def cross_moments(self):
        """the sampler's DeviceCrossMoments with b the K values of this derived ring (K <= 512)"""
        return DeviceCrossMoments(self.dev, on=self)


class HostEnergySampler(DeviceSampler):
    """DeviceSampler for an energy given as opaque Python callables (DeviceEnergy.host): ``iterate`` has the contract of
    the device's mjhmc_iterate, but every sampling iteration is driven from here through mjhmc_traj_begin / _step /
    _finish -- the callables are called once per leapfrog step on the proposal columns (N + n_cold of them), everything
    else (state, leapfrog arithmetic, jump decision, commit, counters, sample ring) runs on the device."""

    def __init__(self, energy, Xinit, Vinit=None, seed=0, first_particle_id=0, dtype='float64', mode=_lib.MODE_MJHMC):
        if dtype_code(dtype) != _lib.F64:
            raise ValueError('host-evaluated energies run in float64')
        super(HostEnergySampler, self).__init__(energy, Xinit, Vinit, seed, first_particle_id, 'float64', mode)
        self._L = 5
        self._set_energy(as_f64(Xinit))

    def _set_energy(self, X):
        E, G = self.energy.host_E(X), self.energy.host_grad(X)
        check(self.lib.mjhmc_host_set_energy(self.handle, ptr(E), ptr(G)), self.lib)

    def set_hparams(self, epsilon, num_leapfrog_steps, p_r, beta=1.0, p_flip=0.5):
        super(HostEnergySampler, self).set_hparams(epsilon, num_leapfrog_steps, p_r, beta, p_flip)
        self._L = int(num_leapfrog_steps)

    def write(self, field, arr):
        super(HostEnergySampler, self).write(field, arr)
        if field == _lib.F_X:                              # HMCState(X): E and dE/dX of the new positions (hmc_state.py:30-38)
            self._set_energy(as_f64(arr, (self.ndims, self.nparticles)))

    def _attempt(self, rn, re, ru, ring_slot):
        n = ctypes.c_int64()
        check(self.lib.mjhmc_traj_begin(self.handle, ctypes.byref(n)), self.lib)
        X = np.empty((self.ndims, n.value))
        g = None
        for _ in range(self._L):
            check(self.lib.mjhmc_traj_step(self.handle, ptr(g), 0, ptr(X)), self.lib)
            g = self.energy.host_grad(X)
        check(self.lib.mjhmc_traj_step(self.handle, ptr(g), 1, None), self.lib)
        if self._L == 0:                                   # no step was taken: the end points are the start points
            X0 = self.read(_lib.F_X)
            X = np.concatenate([X0, X0[:, np.isnan(self.read(_lib.F_HFLF))]], axis=1)[:, :n.value]
        E = self.energy.host_E(X)
        st = _lib.IterStats()
        check(self.lib.mjhmc_traj_finish(self.handle, ptr(E), ptr(rn), ptr(re), ptr(ru), int(ring_slot), ctypes.byref(st)),
              self.lib)
        return st

    def iterate(self, n_iter=1, replay_normal=None, replay_exp=None, replay_unif=None, ring_slot0=-1):
        D, N = self.ndims, self.nparticles
        rn = None if replay_normal is None else as_f64(replay_normal).reshape(n_iter, D, N)
        re = None if replay_exp is None else as_f64(replay_exp).reshape(n_iter, 3, N)
        ru = None if replay_unif is None else as_f64(replay_unif).reshape(n_iter, 2 * N + 1)
        stats, done = [], 0
        for i in range(n_iter):
            st = self._attempt(None if rn is None else np.ascontiguousarray(rn[i]), None if re is None else np.ascontiguousarray(re[i]),
                               None if ru is None else np.ascontiguousarray(ru[i]), ring_slot0 + i if ring_slot0 >= 0 else -1)
            stats.append(st)
            if st.nonfinite:
                break
            done += 1
        return stats, done

    def iterate_download(self, n_iter, ring_slot0, out, k0=0):
        """(the caller's callables pace this sampler: the slots are read once the iterations are done)"""
        stats, done = self.iterate(n_iter, ring_slot0=ring_slot0)
        N = self.nparticles
        for i in range(done):
            out[:, (k0 + i) * N:(k0 + i + 1) * N] = self.ring_read(ring_slot0 + i, 1)
        return stats, done

    def last_timing(self):
        return dict(total_ms=0.0, jump_kernel_ms=0.0, n_jump_launches=0)


def make_sampler(energy, *args, **kwargs):
    """DeviceSampler, or HostEnergySampler for an energy only the caller can evaluate."""
    cls = HostEnergySampler if energy.kind == _lib.E_HOST else DeviceSampler
    return cls(energy, *args, **kwargs)
