"""The statistics of a recorded run: the block walk through the device ring, the driver every ring statistic runs, and
the methods built on them, as a mixin of the samplers.

Belongs here: what runs iterations through the ring and accumulates on the device -- ``_ring_blocks``, ``RecordedRun``
and ``RecordedStatistics``.  Does not belong here: the samplers themselves (markov_jump_hmc.py), what a method is asked
for or refuses (requests.py) and what it returns (results.py).
"""
from __future__ import print_function

import numpy as np

from .. import _lib
from .. import engine
from .requests import (EnergyObservables, Functionals, Projections, _GROUPED_PER_EXPERT, _SUMS_NOT_REDUCED, checked_n_iter,
                       group_pointwise_request, influence_request, pointwise_request, refuse_grouped, refuse_host_energy,
                       refuse_sharded, refuse_wide)
from .results import (ControlVariateExpectations, Diagnostics, Expectations, Influence, JointMarginals, Marginals, Occupancy,
                      Paths, PointwiseStatistics, SteinDiscrepancy, Temperature, Waic)


def dwell_quantum(W, n_states):
    """The unit the jump samplers count holding times in: 2^(floor(log2(mean weight of the first block)) - 24)"""
    return 2.0 ** (np.floor(np.log2(W / n_states)) - 24)


def _ring_blocks(sampler, segments, block):
    """The block walk of expectations() and diagnostics(): runs sum(segments) states of every particle through the
    ring, at most ``block`` at a time and never across a segment boundary, and yields ``(segment, k)`` when the next k
    states sit in ring slots 0 .. k - 1 -- for the jump samplers with their holding times in dwell slots 1 .. k (the
    run's first block runs k + 1 iterations; every later one starts from a copy of the last state in the lead slot)."""
    lead = 1 if sampler._dwell_weighted else 0
    done = last = 0
    for seg, length in enumerate(segments):
        seg_done = 0
        while seg_done < length:
            k = min(block, length - seg_done)
            if not lead:
                sampler._run(k, ring_slot0=0, keep_trace=done > 0)
            elif done == 0:
                sampler._run(k + 1, ring_slot0=0)          # states in slots 0 .. k, their holding times in 1 .. k (+ the next block's)
            else:
                sampler._dev.ring_copy(last, 0)            # the state whose holding time the first iteration of this block draws
                sampler._run(k, ring_slot0=1, keep_trace=True)
            yield seg, k
            last, done, seg_done = k, done + k, seg_done + k


class RecordedRun(object):
    """The protocol every ring statistic runs, once: choose the block, size the ring, open ``of`` on it, walk
    ``_ring_blocks``, publish, and close what was opened.

        with self._RecordedRun(self, [n_iter], block, of, reserve_bytes) as run:
            h = run.own(run.src.estimator(cov))        # closed on any exit, latest first, then the ``of`` handle
            for seg, k in run.blocks():                # the block sits in slots 0 .. k - 1, ``of`` evaluated
                h.accumulate(0, k, w_slot0=run.w_slot0)
            run.finish()                               # _publish, the dwelling times; then read the sums

    ``reserve_bytes``: a number, or a callable that is asked only when the block comes from the budget.  ``src``: the
    sampler's device or, with ``of``, its derived ring; ``lead``: 1 for the jump samplers (the lead slot).
    ``early(run)``: handles that must exist before the budget is taken, because it is to count them (two-stage start:
    ``head`` is what it returned on the final ring); ``early_keeps``: they have storage of their own."""

    def __init__(self, sampler, segments, block, of=None, reserve_bytes=0, early=None, early_keeps=False):
        self.sampler, self.segments, self.block, self.of, self.reserve_bytes = sampler, segments, block, of, reserve_bytes
        self.early, self.early_keeps = early, early_keeps
        self.lead = 1 if sampler._dwell_weighted else 0
        self.w_slot0 = 1 if self.lead else -1
        self.fn, self.src, self.head, self._owned = None, sampler._dev, None, []

    def __enter__(self):
        dev, lead = self.sampler._dev, self.lead
        try:
            if self.early is not None:
                dev.ring_alloc(1 + lead)               # (handles are created on a sampler that has its ring)
                self._open(1)
            self.block = block = self._choose_block()
            if self.early_keeps:
                dev.ring_alloc(block + lead)
            elif self.early is None or block + lead > dev.ring_slots or \
                    (self.fn is not None and block > self.fn.ring_slots):
                # a ring that grows is a new ring, and handles belong to the one they were created on: free them,
                # grow the ring by the budget that counted them, take them again (the functionals belong to the
                # sample ring in the same way, and the handles on them to the derived ring)
                self._close()
                dev.ring_alloc(block + lead)
                self._open(block)
        except BaseException:
            self._close()
            raise
        return self

    def __exit__(self, *exc):
        self._close()

    def _choose_block(self):
        s, n, block = self.sampler, self.segments[0], self.block
        if block is None:
            extra = s._extra_slot_bytes(self.of)
            reserve = self.reserve_bytes() if callable(self.reserve_bytes) else self.reserve_bytes
            block = s._dev.ring_budget_slots(n + self.lead, staging=False, extra_bytes=extra,
                                             reserve_bytes=reserve) - self.lead
        block = max(1, min(int(block), n))
        if s._comm is not None:
            # _run is collective for the jump samplers: every rank must walk the run in the same blocks, whatever its
            # own free memory or the caller's argument on that rank say
            block = int(s._comm.allreduce_ints([block], 'min')[0])
        return block

    def _open(self, n_slots):
        if self.of is not None:
            self.fn = self.src = self.sampler._open_functionals(self.of, n_slots)
        if self.early is not None:
            self.head = self.early(self)

    def _close(self):
        while self._owned:
            self._owned.pop().close()
        if self.fn is not None:
            self.fn.close()
        self.fn, self.src, self.head = None, self.sampler._dev, None

    def own(self, handle):
        self._owned.append(handle)
        return handle

    def release(self, handle):
        """``handle`` leaves the run open: its caller closes it"""
        self._owned.remove(handle)
        return handle

    def blocks(self):
        for seg, k in _ring_blocks(self.sampler, self.segments, self.block):
            if self.fn is not None:
                self.fn.evaluate(0, k, 0)
            yield seg, k

    def accumulate_about(self, handle, accumulate, shift, w_and_sum):
        """Every block into ``handle`` through ``accumulate(k)``, the sums about ``shift`` (rank 0's).  None: the first
        block's own mean, S / W of ``w_and_sum(handle.read())``, then the same block again about it.  Returns the shift."""
        if shift is not None:
            shift = self.sampler._from_rank0(shift)
            handle.set_shift(shift)
        for _, k in self.blocks():
            accumulate(k)
            if shift is None:
                W, S = w_and_sum(handle.read())
                shift = S / W
                handle.reset()
                handle.set_shift(shift)
                accumulate(k)
        return shift

    def first_block_sums(self, k):
        """One throw-away moment pass over the block in slots 0 .. k - 1 (the first: for a shift, a range, a quantum or
        a dt that the caller did not give): (W, S1, S2, None, n_states), summed over ranks."""
        est = self.own(self.src.estimator(False))
        est.accumulate(0, k, w_slot0=self.w_slot0)
        sums = self.sampler._reduce_sums(est.read())
        self.release(est).close()
        return sums

    def finish(self):
        self.sampler._publish()
        if self.lead:
            self.sampler._read_dwell()


class RecordedStatistics(object):
    """The statistics methods of ``HMCBase``.  They reach into the sampler through ``_dev``, ``_comm``, ``_run``,
    ``_publish``, ``_read_dwell``, ``_dwell_weighted``, ``distribution``, ``ndims`` and ``nbatch`` only."""

    _RecordedRun = RecordedRun                             # (the name the driver had as a nested class of HMCBase)

    def functionals(self, values, stats=(), params=(), names=None):
        """K functionals of the state for ``expectations / diagnostics / marginals (..., of=F)``:
            S[j] = sum_d stat_j(x_d, d; p),   g[k] = value_k(S; p)
        ``values``: 1 .. 16 C expressions of ``S[j]`` and ``p[m]``; ``stats``: 0 .. 8 C expressions of ``x`` (a coordinate,
        float64), ``d`` (its index) and ``p[m]``; ``params``: the float64 ``p``.  ``d == 3 ? x : 0.0`` picks a coordinate.
        Everything is float64 and nothing is fused, so + - * /, comparisons and ?: round as the same NumPy expression
        does.  The expressions are compiled here (no device needed): one that does not compile raises ValueError with the
        compiler's message.  Returns a ``Functionals``."""
        F = Functionals(values, stats, params, names)
        lib = _lib.load()
        rc = lib.mjhmc_functionals_check(int(self.ndims), engine.join_exprs(F.stats), engine.join_exprs(F.values),
                                         _lib.KERNEL_HEADERS.encode())
        if rc != 0:
            msg = lib.mjhmc_last_error()
            raise ValueError('functionals: %s' % (msg.decode() if msg else '?'))
        return F

    def projections(self, A, b=None, link=None, params=(), names=None):
        """K linear read-outs of the state for ``expectations / diagnostics / marginals / joint_marginals (..., of=P)``:
            u[k] = b[k] + sum_d A[k][d] x_d,   g[k] = link(u[k], k; p)
        ``A``: (K, ndims), or (ndims,) for one direction, 1 <= K <= 512; ``b``: a scalar or (K,), default 0; ``link``: None
        (g = u) or one C expression of ``u`` (float64), ``k`` (int) and ``p[m]``, e.g. ``'1.0 / (1.0 + exp(-u))'``;
        ``params``: the float64 ``p``.  The values are formed on the device by a small GEMM over the recorded states
        (csrc/projections.hpp): an accumulator starts at b[k] and adds the products in ascending d, nothing fused, so a
        value equals the NumPy loop ``u = b.copy(); for d: u = u + A[:, d, None] * X[d]`` bit for bit, whatever the state
        type and the blocks.  Shapes, finiteness and the range of K are checked and the link is compiled here (no device
        needed): ValueError, with the compiler's message for a link that does not compile.  Returns a ``Projections``;
        ``Projections.principal(expectations)`` builds one from a measured covariance."""
        P = Projections(A, b, link, params, names, ndims=self.ndims)
        lib = _lib.load()
        rc = lib.mjhmc_projections_check(P.n_values, None if P.link is None else P.link.encode(), _lib.KERNEL_HEADERS.encode())
        if rc != 0:
            msg = lib.mjhmc_last_error()
            raise ValueError('projections: %s' % (msg.decode() if msg else '?'))
        return P

    def energy_observables(self):
        """The energy observables [E, grad_sq, virial] for ``expectations / diagnostics / marginals / joint_marginals
        (..., of=EO)``: the potential energy of every recorded state, |dE/dX|^2 and x . dE/dX, evaluated on the device by
        the sampler's own energy kernels (one gradient per recorded state, against num_leapfrog_steps per iteration) --
        what ``functionals()`` cannot state for a coupled energy.  The run is that of ``of=None``, bit for bit, and these
        evaluations are NOT counted in ``distribution.E_count`` / ``dEdX_count``: those price the chain and feed
        ``ess_per_grad``; the observable is measurement, not sampling.  Returns an ``EnergyObservables``.  An energy given
        as opaque callables has no device evaluation: ValueError, before anything runs."""
        refuse_host_energy(self.distribution, 'energy_observables', 'E and dE/dX to record (sample(preserve_order=True) and '
                           'the callables give them on the host)')
        return EnergyObservables()

    def temperature(self, n_iter, split=True, block=None):
        """The virial thermometer: is this chain sampling exp(-E) at all?  Integration by parts gives, for every target
        density p = exp(-E) / Z with p(x) x -> 0 at infinity,

            E_p[x . dE/dX] = ndims

        so ``T = mean[virial] / ndims`` is 1 for chains that keep the law, above 1 for chains that run hot and below for
        cold ones.  Runs ``diagnostics(n_iter, split, block, of=self.energy_observables())`` -- the same run, counters and
        weights -- and returns a ``Temperature``: ``T``, its standard error ``stderr = sqrt(var_plus / ess) / ndims`` from
        the multi-chain ESS of the virial, ``z = (T - 1) / stderr``, ``mean_energy``, ``mean_grad_sq``, ``rhat_energy``
        and the ``diagnostics``.  ``T`` is the POOLED statement "all chains together keep the law" (the plain average of
        the chain means): it says nothing about a single chain, and chains that err in opposite directions can cancel --
        ``rhat_energy`` is the per-chain check.  The condition holds for the Gaussians, the funnels, the mixtures,
        ProductOfT and the linear models here.  It does NOT hold for SparseImageCode with the Cauchy prior at its
        lambda = 0.01: in the n_coeffs - img_size directions the dictionary does not see, p ~ (1 + a^2)^-lambda is not
        integrable (it would need 2 lambda > 1), each such coordinate contributes at most 2 lambda to the virial instead
        of 1, and the thermometer reads about img_size / n_coeffs (0.26 measured at 256 / 1024) on a correct chain: there
        T compares chains with each other (float32 against bfloat16 state), not with 1."""
        return Temperature(self.diagnostics(n_iter, split=split, block=block, of=self.energy_observables()), self.ndims)

    def stein_discrepancy(self, n_iter, every=1, particles=None, c=None, block=None):
        """Is the ensemble a sample of exp(-E)?  The kernel Stein discrepancy of the particles at every ``every``-th of
        ``n_iter`` recorded states, against the sampler's own target, on the device (csrc/stein.hpp): the supremum of the
        Stein identity over the unit ball of the IMQ kernel (c^2 + |x-y|^2)^(-1/2) (Gorham & Mackey 2017).  It needs the
        states and dE/dX at the states only -- no normaliser, no reference sample, no closed-form moments -- and with this
        kernel it vanishes in the limit for the target alone.  Returns a ``SteinDiscrepancy``: a burn-in curve
        (``ksd`` / ``u`` against ``iterations``) and a scalar (``mean_u``) that compares samplers on one target.

        The run is that of ``expectations(n_iter)``: the same iterations in blocks of ``block`` states, the same weights
        (holding times for the jump samplers, which run ``n_iter + 1`` iterations; one per state otherwise), the same
        counters, ``dwelling_times`` and final state, bit for bit.  The gradient evaluations of the pass are NOT counted in
        ``E_count`` / ``dEdX_count`` (measurement, not sampling).  The results do not depend on ``block``.

        ``particles``: the pass is quadratic, so it takes the first ``particles`` particles (default min(nbatch, 8192));
        particle columns are exchangeable, so a prefix is a fair subsample.  ``c``: the kernel scale, default sqrt(ndims)
        (c = 1 loses a scale error at ndims = 512; pass c = 1.0 for the literature's default).  ValueError, before anything
        runs: n_iter < 1, every < 1, particles outside [1, nbatch], c not finite or <= 0, an energy given as opaque
        callables (no device evaluation of dE/dX), a sharded sampler (pairs across ranks are not formed)."""
        n_iter, every = checked_n_iter(n_iter), int(every)
        if every < 1:
            raise ValueError('every must be >= 1, got %d' % every)
        particles = min(int(self.nbatch), 8192) if particles is None else int(particles)
        if particles < 1 or particles > int(self.nbatch):
            raise ValueError('particles must be in [1, nbatch = %d], got %d' % (int(self.nbatch), particles))
        c = float(np.sqrt(self.ndims)) if c is None else float(c)
        if not np.isfinite(c) or c <= 0:
            raise ValueError('the kernel scale c must be finite and > 0, got %r' % c)
        refuse_host_energy(self.distribution, 'stein_discrepancy', 'dE/dX to form the Stein kernel from')
        refuse_sharded(self._comm, 'stein_discrepancy', 'pairs of particles across ranks are not formed')
        # the handle's dE/dX matrix is at most two slots (float32 gradient of a bfloat16 state); the partials are small
        reserve = lambda: 2 * self._dev.ring_slot_bytes()
        its, rows = [], []
        with self._RecordedRun(self, [n_iter], block, reserve_bytes=reserve) as run:
            st = run.own(self._dev.stein(c))
            done = 0
            for _, k in run.blocks():
                for j in range(k):
                    if (done + j) % every == 0:
                        its.append(done + j)
                        rows.append(st.evaluate(j, 1 + j if run.lead else -1, particles))
                done += k
            run.finish()
        rows = np.asarray(rows, dtype=np.float64).reshape(-1, 4)
        return SteinDiscrepancy(its, rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3], particles, c)

    def _open_functionals(self, of, n_slots):
        """the device side of ``of`` on this sampler's ring (which must have its final size), with a derived ring"""
        if isinstance(of, EnergyObservables):
            fn = self._dev.energy_observables()
        elif isinstance(of, Projections):
            fn = self._dev.projections(of.A, of.b, of.link, of.params)
        else:
            fn = self._dev.functionals(of.values, of.stats, of.params)
        try:
            fn.ring_alloc(n_slots)
        except Exception:
            fn.close()
            raise
        return fn

    def _check_of(self, of):
        """what of ``of`` can be refused before the run starts"""
        if isinstance(of, Projections) and of.A.shape[1] != self.ndims:
            raise ValueError('the projections have %d columns, the sampler has ndims = %d' % (of.A.shape[1], self.ndims))

    def _extra_slot_bytes(self, of):
        return 0 if of is None else of.slot_bytes(self._dev.nparticles)

    def expectations(self, n_iter, cov=False, block=None, shift=None, of=None):
        """Mean, variance and (``cov=True``, ndims <= 512) covariance of ``n_iter`` consecutive states of every particle,
        accumulated on the device: the host receives O(D) or O(D^2) numbers whatever the length of the run
        (csrc/estimators.hip).  Returns an ``Expectations``.

        Discrete-time samplers run ``n_iter`` iterations and count every state once.  The jump samplers weight the
        state of ring slot s by the holding time the NEXT iteration draws for it (dwell slot s + 1), so they run
        ``n_iter + 1`` iterations: the last one supplies the last holding time and its state is not counted.  Counters,
        ``dwelling_times`` and the final state are what that many iterations of ``sample(resample=False)`` leave.

        The run goes through the ring in blocks of ``block`` states (default: what the device holds).  ``shift``: the
        vector the device sums are taken about (cancellation); None takes the first block's own mean, at the price of
        reading that block twice.  The returned moments are about the true mean whatever the shift.  Sharded samplers
        sum over ranks, use rank 0's shift and the smallest ``block`` of all ranks.

        ``of``: a ``Functionals`` (``functionals()``), ``Projections`` (``projections()``) or ``EnergyObservables`` (``energy_observables()``).  The run is exactly that of ``of=None``; every block is evaluated
        into a derived ring on the device (csrc/functionals.hip) and the moments are those of the K functional values:
        ``shift`` has K entries and the result K "dimensions".  With an ``EnergyObservables`` the moments are accumulated
        slot by slot, so that under a given ``shift`` the sums W, S1, S2 (and C) do not depend on ``block``."""
        n_iter = checked_n_iter(n_iter)
        shift = self._checked_shift(shift, of)
        self._check_of(of)
        with self._RecordedRun(self, [n_iter], block, of) as run:
            est = run.own(run.src.estimator(cov))
            def accumulate(k):
                if isinstance(of, EnergyObservables):
                    # slot by slot, as the block was evaluated: the moment pass adds a call's sum to its running totals, so
                    # one call per slot makes W, S1 and S2 independent of how the run is cut into blocks, bit for bit
                    for j in range(k):
                        est.accumulate(j, 1, w_slot0=1 + j if run.lead else -1)
                else:
                    est.accumulate(0, k, w_slot0=run.w_slot0)

            shift = run.accumulate_about(est, accumulate, shift, lambda sums: self._reduce_sums(sums)[:2])
            run.finish()
            W, S1, S2, C, n_states = self._reduce_sums(est.read())
        return Expectations(W, S1, S2, C, n_states, shift)

    def cv_expectations(self, n_iter, of=None, block=None, shift=None):
        """Variance-reduced expectations of ``n_iter`` consecutive states of every particle: the means of
        ``expectations(n_iter, of=of)`` with the gradient g = dE/dX of every recorded state as ndims control variates
        (csrc/crossmoments.hip).  Integration by parts gives E_p[g] = 0 for every target p = exp(-E) / Z that vanishes at
        infinity, so f - coef^T g has the expectation of f for any coef, and with coef = Cov(g, g)^-1 Cov(g, f) the variance
        of the residual of a linear regression of f on g (the first-order zero-variance control variates of Mira, Solgi and
        Imparato 2013).  For a Gaussian target the mean is exact at every state, equilibrated or not.  Returns a
        ``ControlVariateExpectations``: ``mean``, ``plain`` (the ``Expectations`` of the same run), ``variance_ratio``,
        ``coef``, ``grad_mean``, ``rank``, ``n_states`` and the raw sums.

        The run is that of ``expectations(n_iter, of=of)``: the same iterations in blocks of ``block`` states, the same
        weights (holding times for the jump samplers, which run ``n_iter + 1`` iterations; one per state otherwise), the
        same counters, ``dwelling_times`` and final state, bit for bit.  The pass costs one gradient per recorded state,
        against num_leapfrog_steps per iteration; these evaluations are NOT counted in ``E_count`` / ``dEdX_count``
        (measurement, not sampling).  Every slot is added to the device sums separately: under a given ``shift`` the sums
        do not depend on ``block``.  ``shift``: the vector the sums of f are taken about; None takes the first block's own
        mean, at the price of reading that block twice.

        ``of``: None (f is the state itself, K = ndims), or the K values of a ``Functionals``, ``Projections`` or
        ``EnergyObservables``.  Second moments of the coordinates come from ``projections(np.eye(ndims), link='u*u')``.

        Caveats.  E_p[g] = 0 needs p -> 0 at infinity: it fails in SparseImageCode's improper directions (the Cauchy prior
        at lambda = 0.01, the warning ``temperature()`` gives).  ``coef`` is estimated from the same states, which leaves a
        bias of order ndims / n_eff.  ``variance_ratio`` is the in-sample residual of the regression, not an ESS-aware
        promise of the error of ``mean``.

        ValueError, before anything runs: n_iter < 1; n_iter * nbatch <= 2 * ndims (the regression is not determined);
        ndims > 512 or K > 512; a wide linear model (named); an energy given as opaque callables; a grouped linear model
        (its sampler runs the multi-pass path, which has no single-launch dE/dX; named); a sharded sampler (the sums are
        additive over ranks, but that is out of scope here: it has not been proved on a multi-rank machine)."""
        n_iter = checked_n_iter(n_iter)
        K = int(self.ndims) if of is None else int(of.n_values)
        refuse_wide(self.distribution, 'cv_expectations')
        if int(self.ndims) > 512 or K > 512:
            raise ValueError('cv_expectations takes ndims <= 512 and K <= 512 values, got ndims = %d, K = %d' % (self.ndims, K))
        if n_iter * int(self.nbatch) <= 2 * int(self.ndims):
            raise ValueError('cv_expectations: n_iter * nbatch = %d states do not determine a regression on ndims = %d '
                             'control variates (more than 2 * ndims are needed)' % (n_iter * int(self.nbatch), self.ndims))
        shift = self._checked_shift(shift, of, 'shift must have %d entries')
        self._check_of(of)
        refuse_grouped(self.distribution, 'cv_expectations',
                       'its sampler runs the multi-pass path with either state dtype, which has no single-launch '
                       'evaluation of dE/dX to take the control variates from')
        refuse_host_energy(self.distribution, 'cv_expectations', 'dE/dX to take the control variates from')
        refuse_sharded(self._comm, 'cv_expectations', 'the sums are additive over ranks, but that is out of scope: it has not '
                       'been proved on a multi-rank machine')
        # the handle's dE/dX matrix is at most two slots (float32 gradient of a bfloat16 state); the partials of the
        # covariance and cross passes are at most ~2048 waves x 32 KiB each
        reserve = lambda: 2 * self._dev.ring_slot_bytes() + (160 << 20)
        with self._RecordedRun(self, [n_iter], block, of, reserve_bytes=reserve) as run:
            cm = run.own(run.src.cross_moments())
            shift = run.accumulate_about(cm, lambda k: cm.accumulate(0, k, w_slot0=run.w_slot0), shift,
                                         lambda sums: (sums[0], sums[3]))
            run.finish()
            sums = cm.read()
        return ControlVariateExpectations(*(sums + (shift,)))

    def pointwise(self, n_iter, values=None, log_mean_exp=None, block=None):
        """Statistics of the DATA ROWS of a linear model over ``n_iter`` consecutive states of every particle: for the
        experts j of the energy E = sum_j f(u_j, j), u = W x + b, and 1 .. 4 ``values`` h_m(u, j) -- float32 C expressions
        of the variables the energy expression sees (``u``, ``j``, ``p[k]``, ``q[m]``) -- the weighted mean and variance of
        every value at every expert and, where ``log_mean_exp`` (one flag per value) asks, the log of the weighted mean of
        exp(value), kept as an online log-sum-exp.  u is formed on the matrix cores by the force's own first GEMM and is
        never stored (csrc/dense_lin_pointwise.hpp): the host receives O(M K) numbers whatever the length of the run.
        Returns a ``PointwiseStatistics``.  ``values=None`` takes ``self.distribution.pointwise_values()``.

        The run is that of ``expectations(n_iter)``: the same iterations in blocks of ``block`` states, the same weights
        (holding times for the jump samplers, which run ``n_iter + 1`` iterations; one per state otherwise), the same
        counters, ``dwelling_times`` and final state, bit for bit.  Nothing is added to ``E_count`` / ``dEdX_count``
        (measurement, not sampling).  The results do not depend on ``block``, bit for bit.

        ValueError, before anything runs: n_iter < 1, no value or more than 4, an energy that is not a linear model, a
        grouped or a wide one (the pass takes at most 512 dims; named), an expression that does not compile (with the
        compiler's message), a sharded sampler (summing over ranks is out of scope here)."""
        values, flags = pointwise_request(self.distribution, n_iter, values, log_mean_exp)
        n_iter = int(n_iter)
        refuse_sharded(self._comm, 'pointwise', _SUMS_NOT_REDUCED)
        def reserve():
            # the handle's float32 rows are at most one slot; its partials are (strips x 4 M x K) doubles
            K = int(np.shape(self.distribution.device_energy()[1]['W'])[0])
            strips = (int(self.nbatch) + 1023) // 1024
            return self._dev.ring_slot_bytes() + 32 * len(values) * (strips + 2) * (K + 512)

        with self._RecordedRun(self, [n_iter], block, reserve_bytes=reserve) as run:
            pw = run.own(self._dev.pointwise(values, flags))
            for _, k in run.blocks():
                pw.accumulate(0, k, w_slot0=run.w_slot0)
            run.finish()
            sums = pw.read()
        return PointwiseStatistics(*(sums + (flags,)))

    def waic(self, n_iter, block=None):
        """WAIC of the model from ``pointwise(n_iter)`` with the distribution's own values: value 0 the pointwise
        log-likelihood without its constants (log-mean-exp on), value 1 the fitted mean
        (``distribution.pointwise_values()``), the constants from ``distribution.log_lik_constants()``, on the first
        ``n_data`` experts (the data rows; the prior's experts are left out).  Returns a ``Waic`` -- ``elpd_waic``,
        ``p_waic``, ``lppd``, ``se``, ``waic``, the per-row arrays, ``fitted`` and ``n_warn``.  Definitions: Gelman, Hwang and
        Vehtari (2014); the weighted population variance of the recorded states stands where they use S - 1.  The run is
        that of ``pointwise(n_iter)``.  ValueError for a distribution without those two methods."""
        d = self.distribution
        refuse_grouped(d, 'waic', _GROUPED_PER_EXPERT)
        refuse_wide(d, 'waic')
        if not (hasattr(d, 'pointwise_values') and hasattr(d, 'log_lik_constants')):
            raise ValueError('waic: %s has no pointwise_values() / log_lik_constants() (GeneralizedLinearModel has)'
                             % type(d).__name__)
        const = np.asarray(d.log_lik_constants(), dtype=np.float64)
        pw = self.pointwise(n_iter, block=block)
        n = const.shape[0]
        fitted = d.fitted_from_value(pw.mean[1, :n]) if hasattr(d, 'fitted_from_value') else None
        return Waic(pw, n, const, fitted)

    def group_pointwise(self, n_iter, values=None, log_mean_exp=None, per=None, block=None):
        """Statistics of the DATA ROWS of a grouped linear model (softmax regression: a row is a GROUP of C experts under a
        log-sum-exp) over ``n_iter`` consecutive states of every particle -- what ``pointwise()`` is to the experts of the
        other linear models.  The 1 .. 4 ``values`` are float32 C expressions at a grouped expert: they see what a
        ``pointwise`` value sees (``u``, ``j`` = g C + c, ``p[k]``, ``q[m]``) and ``lse`` (the group's log-sum-exp, formed as
        the energy forms it), ``sm`` (the member's softmax) and ``c`` (the member index).  ``per`` gives each value's kind:
        'group' (the default) -- the float32 sum of the expression over the group's members in ascending c, one number per
        row -- or 'member' -- one number per grouped expert.  The logits are formed on the matrix cores by the force's own
        first GEMM and never stored (csrc/dense_lin_group_pointwise.hpp).  ``values=None`` takes
        ``self.distribution.group_values()``.

        Returns one ``PointwiseStatistics`` per value, in a list: the arrays of a per-group value have shape (G,), those of
        a per-member value (G, C) -- row g the group, column c the member.  The plain experts behind the groups (a prior)
        are not reported on.

        The run is that of ``expectations(n_iter)``, exactly as for ``pointwise()``: the same iterations, weights,
        counters, ``dwelling_times`` and final state, bit for bit; nothing is added to ``E_count`` / ``dEdX_count``; the
        results do not depend on ``block``, bit for bit.

        ValueError, before anything runs: n_iter < 1, no value or more than 4, flags or kinds that do not pair with the
        values, an energy that is not a grouped linear model, an expression that does not compile (with the compiler's
        message), a sharded sampler (summing over ranks is out of scope here)."""
        values, flags, per = group_pointwise_request(self.distribution, n_iter, values, log_mean_exp, per)
        n_iter = int(n_iter)
        refuse_sharded(self._comm, 'group_pointwise', _SUMS_NOT_REDUCED)
        C, G = (int(v) for v in self.distribution.device_energy()[1]['groups'])

        def reserve():
            # the handle's float32 rows are at most one slot; its partials are (strips x 4 M x columns) doubles
            strips = (int(self.nbatch) + 1023) // 1024
            return self._dev.ring_slot_bytes() + 32 * len(values) * (strips + 2) * (G * C + 512)

        with self._RecordedRun(self, [n_iter], block, reserve_bytes=reserve) as run:
            pw = run.own(self._dev.group_pointwise(values, flags, per))
            for _, k in run.blocks():
                pw.accumulate(0, k, w_slot0=run.w_slot0)
            run.finish()
            W, S1, S2, mx, se, n_states = pw.read()
        out = []
        for m, kind in enumerate(per):
            shape, n = ((G, C), G * C) if kind == 'member' else ((G,), G)
            out.append(PointwiseStatistics(W, *([a[m, :n].reshape(shape).copy() for a in (S1, S2, mx, se)] + [n_states, [flags[m]]])))
        return out

    def group_waic(self, n_iter, block=None):
        """WAIC of a grouped model from ``group_pointwise(n_iter)`` with the distribution's own values
        (``distribution.group_values()``): value 0 the log-likelihood of every data row (per group, log-mean-exp on), value 1
        the fitted class probabilities (per member); the constants from ``distribution.log_lik_constants()``.  Returns a
        ``Waic`` with ``n_data`` = G rows and ``fitted`` the (G, C) posterior-mean class probabilities; its ``pointwise`` is
        value 0's statistics with the arrays as (1, G).  Definitions as for ``waic()``; the run is that of
        ``group_pointwise(n_iter)``.  ValueError for a distribution without those two methods."""
        d = self.distribution
        if not (hasattr(d, 'group_values') and hasattr(d, 'log_lik_constants')):
            raise ValueError('group_waic: %s has no group_values() / log_lik_constants() (MultinomialLogisticRegression has)'
                             % type(d).__name__)
        const = np.asarray(d.log_lik_constants(), dtype=np.float64)
        ll, fit = self.group_pointwise(n_iter, block=block)[:2]
        rows = PointwiseStatistics(ll.W, ll.S1[None, :], ll.S2[None, :], ll.lme_max[None, :], ll.lme_sum[None, :], ll.n_states,
                                   ll.flags)
        return Waic(rows, const.shape[0], const, fit.mean)

    def influence(self, n_iter, value=None, experts=None, block=None, shift=None):
        """How the DATA ROWS of a linear model move its coefficients, over ``n_iter`` consecutive states of every particle:
        the (ndims, j1 - j0) matrix Cov(x_d, t_j) of the state with ONE value t_j = h(u_j, j) per expert -- a float32 C
        expression of the variables a ``pointwise`` value sees; ``value=None`` takes ``distribution.influence_value()``, the
        pointwise log-likelihood.  To first order -Cov(x, l_j) is what deleting row j does to the posterior mean, and
        sum_j Cov(x, l_j) Cov(x, l_j)^T the infinitesimal-jackknife covariance of that mean.  u is formed on the matrix
        cores panel of experts by panel; the values of one panel are stored, the N x K matrix never is
        (csrc/dense_lin_values.hpp, csrc/influence.hip).  Returns an ``Influence``.  ``experts``: (j0, j1), None for all K.

        The run is that of ``expectations(n_iter)``: the same iterations in blocks of ``block`` states, the same weights
        (holding times for the jump samplers, which run ``n_iter + 1`` iterations; one per state otherwise), the same
        counters, ``dwelling_times`` and final state, bit for bit.  Nothing is added to ``E_count`` / ``dEdX_count``: no
        gradient is evaluated.  Under a given ``shift`` the sums do not depend on ``block``, bit for bit.  ``shift``:
        (cx, ct), the ndims and j1 - j0 numbers the sums of x and of t are taken about; None takes the first block's own
        means (an estimator for x, the ``pointwise`` pass for t), at the price of reading that block twice.

        ValueError, before anything runs: n_iter < 1, an energy that is not a linear model (named), a distribution without
        ``influence_value()`` when ``value=None``, experts that are not a range inside the model, a sharded sampler, an
        expression that does not compile (with the compiler's message)."""
        value, (j0, j1) = influence_request(self.distribution, n_iter, value, experts, sharded=self._comm is not None)
        n_iter = int(n_iter)
        D, J = int(self.ndims), j1 - j0
        if shift is not None:
            cx = np.ascontiguousarray(np.asarray(shift[0], dtype=np.float64).reshape(-1))
            ct = np.ascontiguousarray(np.asarray(shift[1], dtype=np.float64).reshape(-1))
            if cx.shape != (D,) or ct.shape != (J,):
                raise ValueError('shift must be (cx with ndims = %d entries, ct with %d entries)' % (D, J))
            shift = (cx, ct)
        def reserve():
            # the handle's panel, float32 rows and widened panel are at most two slots, the first block's pointwise handle
            # half a slot and its partials; the totals are D x J doubles, the cross pass's partials at most ~2048 waves x 32 KiB
            K = int(np.shape(self.distribution.device_energy()[1]['W'])[0])
            strips = (int(self.nbatch) + 1023) // 1024
            return (3 * self._dev.ring_slot_bytes() + (96 << 20) + 8 * D * J
                    + 16 * 1025 * (J // 128 + 2) + 32 * (strips + 2) * (K + 512))

        with self._RecordedRun(self, [n_iter], block, reserve_bytes=reserve) as run:
            inf = run.own(self._dev.influence(value, (j0, j1)))
            if shift is not None:
                inf.set_shift(*shift)
            for _, k in run.blocks():
                if shift is None:                          # the first block's own means; neither handle touches the sampler
                    W, S1 = run.first_block_sums(k)[:2]
                    pw = run.own(self._dev.pointwise([value], [False]))
                    pw.accumulate(0, k, w_slot0=run.w_slot0)
                    Wt, T1 = pw.read()[:2]
                    run.release(pw).close()
                    shift = (S1 / W, np.ascontiguousarray(T1[0, j0:j1] / Wt))
                    inf.set_shift(*shift)
                inf.accumulate(0, k, w_slot0=run.w_slot0)
            run.finish()
            sums = inf.read()
            Cxt = inf.read_cross()
        W, Sx, S2x, St, S2t, n_states = sums
        return Influence(W, Sx, S2x, St, S2t, Cxt, n_states, (j0, j1), shift[0], shift[1],
                         n_data=getattr(self.distribution, 'n_data', None))

    def _checked_shift(self, shift, of=None, text=None):
        """A caller's ``shift`` as the float64 vector the device takes, checked before the run: one entry per dimension,
        or per value of ``of`` (``text``: the refusal, where a method words its own).  None stays None."""
        if shift is None:
            return None
        name, n = ('ndims', self.ndims) if of is None else ('n_values', of.n_values)
        if np.size(shift) != n:
            raise ValueError((text or 'shift must have %s = %%d entries' % name) % n)
        return np.ascontiguousarray(np.asarray(shift, dtype=np.float64).reshape(-1))

    def _from_rank0(self, v):
        """rank 0's ``v`` on every rank of a sharded sampler"""
        return v if self._comm is None else self._comm.bcast(v.copy(), 0)

    def diagnostics(self, n_iter, split=True, block=None, shift=None, of=None):
        """R-hat and the multi-chain effective sample size of ``n_iter`` consecutive states of every particle, every
        particle being one chain: per-chain sums kept on the device (csrc/chainstats.hip), O(ndims) numbers to the host
        whatever the length of the run and the number of chains.  Returns a ``Diagnostics``.

        ``split=True`` (even ``n_iter`` >= 4) treats the two halves of every chain as two chains of ``n_iter / 2`` states
        -- a chain that drifts disagrees with itself; ``split=False`` (``n_iter`` >= 2) takes the chains whole.  The run
        itself is that of ``expectations(n_iter)``: the same iterations, the same weights (holding times for the jump
        samplers, which run ``n_iter + 1`` iterations; one per state otherwise), the same counters, ``dwelling_times`` and
        final state, in blocks of ``block`` states that never straddle the half boundary.  ``shift``: the vector the
        device sums are taken about; None takes the pooled mean of the first block (one extra moment pass over it, before
        the chain sums start).  Sharded samplers sum over ranks, use rank 0's shift and the smallest ``block`` of all
        ranks.  The per-chain sums take device memory (parts x (2 x row pitch + 1) x padded particles x 8 bytes): they
        are created before the block size is taken from what the device has left.

        ``of``: a ``Functionals`` (``functionals()``), ``Projections`` (``projections()``) or ``EnergyObservables`` (``energy_observables()``): the same run, the diagnostics of the K functional values (every
        block is evaluated into a derived ring first; ``shift`` has K entries)."""
        n_iter = int(n_iter)
        if split and (n_iter < 4 or n_iter % 2):
            raise ValueError('split=True needs an even n_iter >= 4, got %d' % n_iter)
        if not split:
            checked_n_iter(n_iter, least=2)
        shift = self._checked_shift(shift, of)
        self._check_of(of)
        segments = [n_iter // 2, n_iter // 2] if split else [n_iter]
        grad0 = self.distribution.dEdX_count
        # (the per-chain sums have the ring's row layout and take memory: they exist before the budget is taken)
        with self._RecordedRun(self, segments, block, of,
                               early=lambda run: run.own(run.src.chain_stats(len(segments)))) as run:
            cs = run.head
            if shift is not None:
                shift = self._from_rank0(shift)
                cs.set_shift(shift)
            for part, k in run.blocks():
                if shift is None:
                    W, S1 = run.first_block_sums(k)[:2]
                    shift = S1 / W
                    cs.set_shift(shift)
                cs.accumulate(0, k, w_slot0=run.w_slot0, part=part)
            run.finish()
            parts = [cs.read(h) for h in range(len(segments))]
        if self._comm is not None:
            from ..parallel import reduce_chain_sums
            parts = reduce_chain_sums(self._comm, parts)
        return Diagnostics(parts, shift, self.distribution.dEdX_count - grad0)

    def marginals(self, n_iter, bins=256, range=None, block=None, span=8.0, of=None):
        """Weighted histograms of every dimension over ``n_iter`` consecutive states of every particle, accumulated on
        the device (csrc/histograms.hip): the host receives 2 x ndims x (bins + 2) integers whatever the length of the
        run.  Returns a ``Marginals`` (quantiles, median, credible intervals, CDF).

        The run itself is that of ``expectations(n_iter)``: the same iterations, the same weights (holding times for the
        jump samplers, which run ``n_iter + 1`` iterations; one per state otherwise), the same counters,
        ``dwelling_times`` and final state, in blocks of ``block`` states.  ``range``: ``(lo, hi)``, scalars or
        ndims-vectors; None takes mean -/+ ``span`` standard deviations from one moment pass over the first block.  The
        jump samplers count weights in units of q = 2^(floor(log2(mean weight of the first block)) - 24); the others in
        units of 1.  Sharded samplers use rank 0's range and quantum and the smallest ``block`` of all ranks, and add
        their integer tables over ranks.

        ``of``: a ``Functionals`` (``functionals()``), ``Projections`` (``projections()``) or ``EnergyObservables`` (``energy_observables()``): the same run, one histogram per functional value (every block is
        evaluated into a derived ring first; ``range`` entries are scalars or K-vectors, and the range=None moment pass,
        ``span`` and the quantum rule apply to the values)."""
        n_iter, bins = checked_n_iter(n_iter), int(bins)
        if not 1 <= bins <= 1024:
            raise ValueError('bins must be in [1, 1024], got %d' % bins)
        lo, hi, q, sums = self._histograms(n_iter, range, block, span, of,
                                           lambda src, lo, hi, q: src.histogram(bins, lo, hi, q))
        return Marginals(lo, hi, bins, q, *sums)

    def _histograms(self, n_iter, range, block, span, of, create):
        """The run of marginals() and joint_marginals(): the range check, the first block's range and quantum, rank 0's
        [lo | hi | q] for all ranks, the handle from ``create(src, lo, hi, q)``, the accumulation, and the tables added over
        ranks.  Returns (lo, hi, q, (counts, units, W_units, n_states)), lo and hi per dimension."""
        K = self.ndims if of is None else of.n_values
        if range is not None:
            if len(range) != 2:
                raise ValueError('range must be (lo, hi)')
            lo, hi = [np.array(np.broadcast_to(np.asarray(v, dtype=np.float64), (K,))) if np.size(v) in (1, K)
                      else None for v in range]
            if lo is None or hi is None:
                raise ValueError('lo and hi must be scalars or have %s = %d entries' % ('ndims' if of is None else 'n_values', K))
            if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi)) and np.all(lo < hi)):
                raise ValueError('range needs finite lo < hi in every dimension')
        elif not span > 0:
            raise ValueError('span must be positive')
        self._check_of(of)
        hist, q = None, 1.0
        with self._RecordedRun(self, [n_iter], block, of) as run:
            for _, k in run.blocks():
                if hist is None:
                    if range is None or run.lead:
                        W, S1, S2, _, n_first = run.first_block_sums(k)
                        if run.lead:
                            q = dwell_quantum(W, n_first)
                        if range is None:
                            mean = S1 / W
                            sd = np.sqrt(np.maximum(S2 / W - mean * mean, 0.0))
                            sd = np.where(sd > 0, sd, 1.0)             # (a constant coordinate still needs lo < hi)
                            lo, hi = mean - span * sd, mean + span * sd
                    if self._comm is not None:
                        packed = self._comm.bcast(np.concatenate([lo, hi, [q]]), 0)
                        lo, hi, q = packed[:K].copy(), packed[K:2 * K].copy(), float(packed[-1])
                    hist = run.own(create(run.src, lo, hi, q))
                hist.accumulate(0, k, w_slot0=run.w_slot0)
            run.finish()
            sums = hist.read()
        if self._comm is not None:
            from ..parallel import reduce_histogram
            sums = reduce_histogram(self._comm, *sums)
        return lo, hi, q, sums

    def joint_marginals(self, n_iter, pairs, bins=64, range=None, block=None, span=8.0, of=None):
        """Weighted joint histograms of ``pairs`` [(i, j), ...] of dimensions over ``n_iter`` consecutive states of every
        particle, accumulated on the device (csrc/pairhist.hip): the host receives 2 x P x (bins + 2)^2 integers whatever
        the length of the run.  Returns a ``JointMarginals`` (density, marginals of either axis, highest-density regions).
        1 <= P <= 64 pairs, 1 <= ``bins`` <= 128 per axis; i == j, repeated pairs and both orders of a pair are allowed.

        The run itself is that of ``marginals(n_iter)``: the same iterations, weights, blocks, quantum rule and -- for
        ``range=None`` -- the same moment pass over the first block (mean -/+ ``span`` standard deviations), the same
        counters, ``dwelling_times`` and final state.  ``range``: ``(lo, hi)`` per DIMENSION, scalars or ndims-vectors: a
        dimension has one range in every pair it appears in.  Sharded samplers use rank 0's ranges and quantum and the
        smallest ``block`` of all ranks, and add their integer tables over ranks.

        ``of``: a ``Functionals`` (``functionals()``), ``Projections`` (``projections()``) or ``EnergyObservables`` (``energy_observables()``): the same run, ``pairs`` index the K functional values (every block
        is evaluated into a derived ring first; ``range`` entries are scalars or K-vectors)."""
        n_iter, bins = checked_n_iter(n_iter), int(bins)
        K = self.ndims if of is None else of.n_values
        if not 1 <= bins <= 128:
            raise ValueError('bins must be in [1, 128], got %d' % bins)
        pairs = np.asarray(pairs)
        if pairs.ndim != 2 or pairs.shape[1] != 2 or not 1 <= pairs.shape[0] <= 64 or pairs.dtype.kind not in 'iu':
            raise ValueError('pairs must be 1 .. 64 pairs (i, j) of integers, got an array of shape %r' % (pairs.shape,))
        pairs = pairs.astype(np.int64)
        if pairs.min() < 0 or pairs.max() >= K:
            raise ValueError('pairs must index [0, %s = %d)' % ('ndims' if of is None else 'n_values', K))
        lo, hi, q, sums = self._histograms(n_iter, range, block, span, of,
                                           lambda src, lo, hi, q: src.pair_histogram(pairs, bins, lo[pairs], hi[pairs], q))
        return JointMarginals(pairs, lo[pairs], hi[pairs], bins, q, *sums)

    def occupancy(self, n_iter, centres, radius=None, of=None, block=None):
        """Cell occupancy and transition counts of ``n_iter`` consecutive states of every particle, every particle being
        one chain, accumulated on the device (csrc/occupancy.hip): how much time the chains spend in each region, how often
        they cross, how many never did, and the relaxation time the crossings imply.  The host receives (M + 1)^2 integers
        whatever the length of the run.  Returns an ``Occupancy``.

        The cells are the Voronoi cells of ``centres`` (M, ndims), 1 <= M <= 64: a state belongs to the nearest centre (the
        lowest index at equal distances).  ``radius``, a scalar or an M-vector, cuts every cell to the ball around its
        centre (core sets).  One more cell, index M, is "outside": every state that belongs to no centre, a state that is
        not finite included.

        The run itself is that of ``expectations(n_iter)``: the same iterations, the same weights (holding times for the
        jump samplers, which run ``n_iter + 1`` iterations; one per state otherwise), the same counters,
        ``dwelling_times`` and final state, bit for bit, in blocks of ``block`` states; nothing is added to ``E_count`` /
        ``dEdX_count``.  Every chain carries its last label from one block to the next, so the tables do not depend on
        ``block``, bit for bit.  The jump samplers count weights in units of q = 2^(floor(log2(mean weight of the first
        block)) - 24); the others in units of 1.

        ``of``: a ``Functionals`` (``functionals()``), ``Projections`` (``projections()``) or ``EnergyObservables``
        (``energy_observables()``): the same run, the cells live in the space of the K functional values (``centres`` is
        (M, K); every block is evaluated into a derived ring first).

        ValueError, before anything runs: n_iter < 2, centres that are not (M, K) with 1 <= M <= 64 or not finite, a radius
        that is negative, NaN or of another size, a sharded sampler (the tables are additive over ranks, but summing them is
        out of scope here)."""
        n_iter = int(n_iter)
        K = self.ndims if of is None else of.n_values
        refuse_sharded(self._comm, 'occupancy', 'the tables are additive over ranks, but summing them is out of scope here')
        if n_iter < 2:
            raise ValueError('n_iter must be >= 2 (a transition takes two states), got %d' % n_iter)
        centres = np.ascontiguousarray(np.asarray(centres, dtype=np.float64))
        if centres.ndim != 2 or centres.shape[1] != K or not 1 <= centres.shape[0] <= 64:
            raise ValueError('centres must be (M, %s = %d) with 1 <= M <= 64, got an array of shape %r'
                             % ('ndims' if of is None else 'n_values', K, centres.shape))
        if not np.all(np.isfinite(centres)):
            raise ValueError('centres must be finite')
        M, r2 = centres.shape[0], None
        if radius is not None:
            radius = np.asarray(radius, dtype=np.float64)
            if radius.size not in (1, M):
                raise ValueError('radius must be a scalar or have M = %d entries' % M)
            radius = np.array(np.broadcast_to(radius.reshape(-1), (M,)))
            if not np.all(radius >= 0):                   # (NaN fails it too)
                raise ValueError('radius must not be negative or NaN')
            r2 = radius * radius
        self._check_of(of)
        grad0 = self.distribution.dEdX_count
        occ, q, done = None, 1.0, 0
        with self._RecordedRun(self, [n_iter], block, of) as run:
            for _, k in run.blocks():
                if occ is None:
                    if run.lead:
                        W, _, _, _, n_first = run.first_block_sums(k)
                        q = dwell_quantum(W, n_first)
                    occ = run.own(run.src.occupancy(centres, r2, q))
                occ.accumulate(0, k, w_slot0=run.w_slot0, linked=done > 0)
                done += k
            run.finish()
            tables = occ.read()
        return Occupancy(tables, q, centres, tables['n_states'], self.distribution.dEdX_count - grad0)

    def paths(self, n_iter, n_grid=None, dt=None, block=None):
        """A fair sample of every chain with its time order kept: the process "chain p sits in state k for its holding
        time" sampled at t_j = j ``dt``, j < ``n_grid``, on the device (csrc/timegrid.hip).  Returns a ``Paths`` (``read``,
        ``autocor``, ``close``); the grid stays on the device.  The weighted estimators make pooled statistics fair and
        lose the order; ``sample(resample=False)`` keeps the order and counts every state once whatever its holding time.

        The run itself is that of ``expectations(n_iter)``: the same iterations, the same holding times (the jump
        samplers run ``n_iter + 1`` iterations; a discrete-time sampler's states hold for one unit each), the same
        counters, ``dwelling_times`` and final state, in blocks of ``block`` states.  ``dt=None`` takes the mean holding
        time of the first block (one moment pass over it; 1 for a discrete-time sampler, whose grid is then its ring);
        ``n_grid=None`` takes ``n_iter``.  With ``dt`` the mean holding time the chains reach grid point ``n_iter`` on
        average, so about half of them stop short of it: ``covered`` says how many grid points all of them reached.
        The grid takes ``n_grid`` ring slots of device memory, counted before the block size is taken from what the
        device has left.  Sharded samplers use rank 0's ``dt`` and the smallest ``block`` of all ranks; ``covered`` is the
        minimum over ranks."""
        n_iter = checked_n_iter(n_iter)
        n_grid = n_iter if n_grid is None else int(n_grid)
        if n_grid < 1:
            raise ValueError('n_grid must be >= 1, got %d' % n_grid)
        if dt is not None and not (np.isfinite(dt) and dt > 0):
            raise ValueError('dt must be finite and positive, got %r' % (dt,))
        comm = self._comm
        if dt is None and not self._dwell_weighted:
            dt = 1.0
        if dt is not None and comm is not None:
            dt = float(comm.bcast(np.array([dt], dtype=np.float64), 0)[0])
        grad0 = self.distribution.dEdX_count
        # a grid whose dt is known exists before the budget is taken (its own storage: the ring may still grow); one that
        # waits for the first block's dt is spoken for
        dt0 = dt
        early = lambda run: None if dt0 is None else run.own(self._dev.time_grid(n_grid, dt0))
        reserve = lambda: n_grid * self._dev.ring_slot_bytes() if dt0 is None else 0
        with self._RecordedRun(self, [n_iter], block, reserve_bytes=reserve, early=early, early_keeps=True) as run:
            tg = run.head
            for _, k in run.blocks():
                if tg is None:                             # dt = W / (N k), the mean holding time of the first block
                    W, _, _, _, n_first = run.first_block_sums(k)
                    dt = float(W) / n_first
                    if comm is not None:
                        dt = float(comm.bcast(np.array([dt], dtype=np.float64), 0)[0])
                    tg = run.own(self._dev.time_grid(n_grid, dt))
                tg.accumulate(0, k, w_slot0=run.w_slot0)
            run.finish()
            covered = tg.progress()[0]
            T = tg.read_clocks()[0]
            sum_T, n_chains = float(np.sum(T)), int(T.size)
            if comm is not None:
                covered = int(comm.allreduce_ints([covered], 'min')[0])
                n_chains = int(comm.allreduce_ints([n_chains], 'sum')[0])
                sum_T = float(comm.allreduce_f64(np.array([sum_T]))[0])
            run.release(tg)                                # the caller's from here: Paths.close() frees it
        grad = self.distribution.dEdX_count - grad0
        return Paths(tg, dt, n_grid, covered, sum_T / n_chains, grad / float(n_chains), n_chains, comm)

    def _reduce_sums(self, sums):
        if self._comm is None:
            return sums
        from ..parallel import reduce_moment_sums
        return reduce_moment_sums(self._comm, sums)
