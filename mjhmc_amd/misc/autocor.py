"""Analysis harness around the hot path (mjhmc/misc/autocor.py): the sample-generation driver
(:213-261) and the autocorrelation that every experiment computes from its output (:37-117, :177-211).

The reference performs one host round trip per step (``samples[:, :, t] = smp.sample(1)`` and a read of the
distribution's counters) and then transforms the (n_dims, n_batch, n_samples) host array with mklfft.
Here the whole run is one batched device call, the per-step counter trace is rebuilt from the kernels'
exact tallies, and the autocorrelation is taken from the device-resident sample ring (batched hipFFT
between two fused kernels, mjhmc_amd/csrc/autocor.hip) - the samples only travel to the host if the
caller asks for them."""
import numpy as np

from .. import engine
from ..samplers.markov_jump_hmc import ContinuousTimeHMC


def fft_autocor(samples, device=0):
    """mjhmc/misc/autocor.py:37-49: autocorrelation by the cross-correlation theorem.

    samples: [n_dims, n_batch, n_samples] -> autocor [n_samples], normalised to 1 at lag 0."""
    samples = np.asarray(samples)
    assert samples.ndim == 3
    sums = engine.context(device).autocor(samples, linear=False)
    return sums / sums[0]


def _lag_means(sums, n_series, n_samples):
    """np.mean(samples[:, :, :-k] * samples[:, :, k:]) for every lag k from the linear lag sums."""
    return sums / (float(n_series) * (n_samples - np.arange(n_samples)))


def slow_autocorrelation(samples, e_evals, grad_evals, half_window=False, device=0):
    """mjhmc/misc/autocor.py:177-211 (zero-mean assumption, window truncated like the reference)."""
    n_dims, n_batch, n_samples = samples.shape
    c = _lag_means(engine.context(device).autocor(samples, linear=True), n_dims * n_batch, n_samples)
    n_lags = (n_samples // 2) - 1 if half_window else n_samples - 1
    c = c[:n_lags]
    return c / c[0], e_evals, grad_evals


def autocorrelation(samples, e_evals, grad_evals, half_window=True, normalize=True, cached_var=None,
                    brute_force=False, use_tf=False, device=0):
    """mjhmc/misc/autocor.py:52-117.  ``brute_force`` selects the lag-product estimator the reference
    compiles with theano / tensorflow (``use_tf`` only chose between those two and is ignored)."""
    n_dims, n_batch, n_samples = samples.shape
    if brute_force:
        c = _lag_means(engine.context(device).autocor(samples, linear=True), n_dims * n_batch, n_samples)
        max_t = (n_samples // 2) - 1 if half_window else n_samples - 1
        ac_squeeze = c[1:max_t]
        var = c[0] if cached_var is None else cached_var
        if normalize:
            autocor = np.vstack((1., (ac_squeeze / var).reshape(-1, 1)))
        else:
            autocor = np.vstack((var, ac_squeeze.reshape(-1, 1)))
        if half_window:
            e_evals = e_evals[:int(n_samples / 2) - 1]
            grad_evals = grad_evals[:int(n_samples / 2) - 1]
        else:
            e_evals = e_evals[:-1]
            grad_evals = grad_evals[:-1]
    else:
        autocor = fft_autocor(samples, device=device)
        assert autocor.shape == e_evals.shape
        assert e_evals.shape == grad_evals.shape
    return autocor, e_evals, grad_evals


def integrated_autocorrelation_time(A, n, n_chains):
    """Per-dimension autocorrelation, integrated autocorrelation time and truncation window from centred linear lag sums.

    A: (K + 1, D) float64, ``A[k, d] = sum over chains and t < n - k of u_t u_{t+k}`` with u the series minus its mean
    (``Paths.lag_cov``, ``DeviceTimeGrid.lag_cov``: the sums of all ``n_chains`` chains over ``n`` grid points).
    Returns ``(rho (K + 1, D), tau (D,), window (D,) int, converged (D,) bool)``:

      rho[k]   = (A[k] / (n_chains (n - k))) / (A[0] / (n_chains n))                  lag-product means over the one of lag 0
      Gamma_m  = rho[2m] + rho[2m + 1],  m < M = (K + 1) // 2                         Geyer's sums of adjacent pairs
      m*       = the first m with Gamma_m <= 0 (initial positive sequence), or M if there is none: the window was too
                 short and converged[d] = False
      Gamma'_m = min(Gamma'_{m-1}, Gamma_m),  m < m*                                  (initial monotone sequence)
      tau      = -1 + 2 sum_{m < m*} Gamma'_m                                         in grid steps
      window   = 2 m*                                                                 the lags that entered tau

    m* = 0 (no pair at all: K = 0, or a first pair that is not positive) gives tau = NaN and converged = False.  A dimension
    with A[0] = 0 (a constant series) or a sum that is not finite gives NaN throughout, window 0 and converged = False,
    without floating-point warnings.  The effective sample size of a dimension is n_chains n / tau."""
    A = np.asarray(A, dtype=np.float64)
    if A.ndim == 1:
        A = A[:, None]
    if A.ndim != 2 or A.shape[0] < 1:
        raise ValueError('A must be (max_lag + 1, ndims), got shape %r' % (A.shape,))
    K, D = A.shape[0] - 1, A.shape[1]
    n, n_chains = int(n), int(n_chains)
    if n_chains < 1 or n < K + 1:
        raise ValueError('need n_chains >= 1 and n > max_lag = %d, got n_chains = %d, n = %d' % (K, n_chains, n))
    ok = np.isfinite(A).all(axis=0) & (A[0] > 0)
    safe = np.where(ok, A, 1.0)
    k = np.arange(K + 1, dtype=np.float64)[:, None]
    rho = np.where(ok, (safe / (n_chains * (n - k))) / (safe[0] / (float(n_chains) * n)), np.nan)
    M = (K + 1) // 2
    tau = np.full(D, np.nan)
    window = np.zeros(D, dtype=np.int64)
    converged = np.zeros(D, dtype=bool)
    if M == 0:
        return rho, tau, window, converged
    gamma = np.where(ok, rho[0:2 * M:2] + rho[1:2 * M:2], 0.0)          # (M, D); a dead dimension stops at m* = 0
    stop = gamma <= 0
    m_star = np.where(stop.any(axis=0), np.argmax(stop, axis=0), M)
    mono = np.minimum.accumulate(gamma, axis=0)
    inside = np.arange(M)[:, None] < m_star[None, :]
    total = np.where(inside, mono, 0.0).sum(axis=0)
    live = ok & (m_star > 0)
    tau = np.where(live, -1.0 + 2.0 * total, np.nan)
    window = np.where(ok, 2 * m_star, 0).astype(np.int64)
    converged = live & (m_star < M)
    return rho, tau, window, converged


def calculate_autocorrelation(sampler, distribution, num_steps=None, num_grad_steps=None, sample_steps=1,
                              half_window=False, use_cached_var=False, replay=None, **kwargs):
    """mjhmc/misc/autocor.py:10-35.  Returns (autocor, e_evals, grad_evals).

    When the run is recorded in the device ring (every sampler except a resampling jump sampler) the
    autocorrelation is computed there and the (n_dims, n_batch, n_samples) block is never downloaded."""
    smp, samples, e_evals, grad_evals, n_keep = _generate(sampler, distribution, num_steps, num_grad_steps,
                                                          download=False, replay=replay, **kwargs)
    if samples is not None:
        return autocorrelation(samples, e_evals, grad_evals, half_window)
    sums = smp._dev.ring_autocor(0, n_keep, linear=False)
    if smp._comm is not None:
        sums = smp._comm.allreduce_f64(sums)          # column shards add their lag sums
    autocor = sums / sums[0]
    assert autocor.shape == e_evals.shape
    return autocor, e_evals, grad_evals


def calculate_time_autocorrelation(sampler, distribution, num_steps, dt=None, n_grid=None, **kwargs):
    """The autocorrelation of the jump process itself, in process time: ``sampler.paths(num_steps, n_grid, dt)`` samples
    every chain on the grid t_j = j dt on the device (a state counts for as long as it is held), and the curve is
    ``fft_autocor`` along the covered part of that grid.  Returns (autocor [covered], grad_evals [covered]) with
    ``grad_evals[k] = k * dt * grad_evals_per_time``, the gradient evaluations per particle that lag k costs.

    The reference has no counterpart: its figures take the curve of ``resample=False`` (every state once, which its own
    docstring calls biased), and ``calculate_autocorrelation`` on a resampling sampler draws step by step on the host.
    A jump sampler's ``resample`` flag plays no part here: it only says what ``sample()`` returns."""
    smp = sampler(distribution=distribution, **kwargs)
    distribution.E_count = 0
    distribution.dEdX_count = 0
    paths = smp.paths(int(num_steps), n_grid=n_grid, dt=dt)
    try:
        autocor = paths.autocor()
    finally:
        paths.close()
    grad_evals = np.arange(autocor.size) * paths.dt * paths.grad_evals_per_time
    return autocor, grad_evals


def generate_samples(sampler, distribution, num_steps=None, num_grad_steps=None, replay=None, **kwargs):
    """Same contract as the reference:

    Returns (samples [n_dims, n_batch, n_samples], e_evals [n_samples], grad_evals [n_samples]) where
    ``grad_evals[t] = distribution.dEdX_count / n_batch`` after step t (counters reset after construction).
    ``replay``: recorded random numbers, one entry per iteration as ``sampling_iteration(replay=...)`` takes them
    (parity tests against the reference's own generate_samples, tests/golden/g9_*)."""
    _, samples, e_evals, grad_evals, _ = _generate(sampler, distribution, num_steps, num_grad_steps,
                                                   download=True, replay=replay, **kwargs)
    return samples, e_evals, grad_evals


def _generate(sampler, distribution, num_steps, num_grad_steps, download, replay=None, **kwargs):
    """(sampler, samples or None, e_evals, grad_evals, n_keep).  ``samples`` is None when ``download`` is
    false and ring slots [0, n_keep) hold the run."""
    assert (((num_steps is None) and (num_grad_steps is not None)) or
            (num_steps is not None) and (num_grad_steps is None))
    smp = sampler(distribution=distribution, **kwargs)
    num_steps = int(num_steps or num_grad_steps / smp.grad_per_sample_step + 100)
    n_batch = distribution.nbatch
    # the reference calls distribution.reset() here: counters to zero (its init_X re-run does not touch
    # the already built sampler state)
    distribution.E_count = 0
    distribution.dEdX_count = 0

    if isinstance(smp, ContinuousTimeHMC) and smp.resample:
        # sample(1) with dwell-time resampling is two iterations plus a host-side draw per step: keep the
        # reference's step structure literally (each step is still device work)
        n_dims = distribution.ndims
        samples = np.zeros((n_dims, n_batch, num_steps))
        grad_evals = np.zeros(num_steps)
        e_evals = np.zeros(num_steps)
        for t_idx in range(num_steps):
            samples[:, :, t_idx] = smp.sample(1)
            grad_evals[t_idx] = distribution.dEdX_count / float(n_batch)
            e_evals[t_idx] = distribution.E_count / float(n_batch)
            if (num_grad_steps is not None) and grad_evals[t_idx] >= num_grad_steps:
                k = t_idx + 1
                return smp, samples[:, :, :k], e_evals[:k], grad_evals[:k], k
        if num_grad_steps is not None:
            assert grad_evals[-1] >= num_grad_steps
        return smp, samples, e_evals, grad_evals, num_steps

    smp._record(num_steps, replay)                                         # one batched launch sequence
    trace = np.cumsum(smp.eval_trace(num_steps), axis=0)
    e_evals = trace[:, 0] / float(n_batch)
    grad_evals = trace[:, 1] / float(n_batch)
    n_keep = num_steps
    if num_grad_steps is not None:
        hit = np.nonzero(grad_evals >= num_grad_steps)[0]
        assert hit.size, 'the run ended before num_grad_steps gradient evaluations per particle'
        n_keep = int(hit[0]) + 1                                           # the reference stops at the first hit
    samples = smp._stack(n_keep, True) if download else None
    return smp, samples, e_evals[:n_keep], grad_evals[:n_keep], n_keep
