"""Sampler classes of the drop-in (mirrors mjhmc/samplers/markov_jump_hmc.py).

Same constructor keywords, methods and attributes as the reference; the per-iteration work
(``state.copy().L()/FLF()/R()``, ``transition_rates``, ``draw_from``, ``min_idx``,
``state.update`` -- markov_jump_hmc.py:355-415) is ONE fused HIP kernel launch per iteration on
the MI355X.  Extra keyword-only arguments: ``seed`` (counter-RNG seed; default drawn from
``np.random`` so ``np.random.seed`` still makes runs reproducible), ``dtype``, ``device``.
"""
from __future__ import print_function

import numpy as np

from .. import _lib
from .. import engine
from ..misc.distributions import Distribution
from .hmc_state import DeviceHMCState, HMCState

MAX_RETRY_DEPTH = 60


class Expectations(object):
    """What ``expectations()`` returns: ``mean`` (D,), ``var`` (D,) and ``cov`` (D, D) or None -- weighted moments about
    the true mean, normalised by ``total_weight`` (no n - 1 correction) -- the number of (slot, particle) states
    ``n_states``, and the raw device sums ``W, S1, S2, C`` about ``shift`` they were computed from
    (include/mjhmc_hip.h: mjhmc_estimator_read)."""

    def __init__(self, W, S1, S2, C, n_states, shift):
        self.W, self.S1, self.S2, self.C, self.shift = W, S1, S2, C, shift
        self.total_weight, self.n_states = W, n_states
        m1 = S1 / W
        self.mean = shift + m1
        self.var = S2 / W - m1 * m1
        self.cov = None if C is None else C / W - np.outer(m1, m1)


class ControlVariateExpectations(object):
    """What ``cv_expectations()`` returns: expectations of the K values f with the gradient g = dE/dX as ndims control
    variates of known mean zero.  From the device sums (include/mjhmc_hip.h: mjhmc_crossmoments_read) -- ``W``, ``Sg``,
    ``S2g``, ``Cgg`` of g about 0 and ``Sb``, ``S2b``, ``Cgb`` of f about ``shift`` --

      grad_mean = Sg / W                               ~ 0 on a correct chain: a per-dimension Stein check in its own right
      m = Sb / W
      cov_gg = Cgg / W - grad_mean grad_mean^T         cov_gf = Cgb / W - grad_mean m^T
      coef = solve(cov_gg, cov_gf)                     (ndims, K): Cholesky; when cov_gg is not positive definite, the
                                                       minimum-norm least-squares solution, and ``rank`` < ndims says so
      mean = shift + m - coef^T grad_mean              the control-variate estimate of E[f]
      plain                                            the ``Expectations`` of f from the same run (mean, var)
      variance_ratio = 1 - diag(cov_gf^T coef) / plain.var
                                                       the in-sample residual of the regression of f on g, in [0, 1]

    plus ``rank``, ``n_states`` and ``total_weight``."""

    def __init__(self, W, Sg, S2g, Sb, S2b, Cgg, Cgb, n_states, shift):
        self.W, self.Sg, self.S2g, self.Sb, self.S2b, self.Cgg, self.Cgb, self.shift = W, Sg, S2g, Sb, S2b, Cgg, Cgb, shift
        self.total_weight, self.n_states = W, n_states
        D = Sg.shape[0]
        self.grad_mean = Sg / W
        m = Sb / W
        self.cov_gg = Cgg / W - np.outer(self.grad_mean, self.grad_mean)
        self.cov_gf = Cgb / W - np.outer(self.grad_mean, m)
        try:
            L = np.linalg.cholesky(self.cov_gg)
            self.coef = np.linalg.solve(L.T, np.linalg.solve(L, self.cov_gf))
            self.rank = D
        except np.linalg.LinAlgError:
            self.coef, _, rank, _ = np.linalg.lstsq(self.cov_gg, self.cov_gf, rcond=None)
            self.rank = int(rank)
        self.plain = Expectations(W, Sb, S2b, None, n_states, shift)
        self.mean = shift + m - self.coef.T.dot(self.grad_mean)
        self.variance_ratio = 1.0 - np.sum(self.cov_gf * self.coef, axis=0) / self.plain.var


class Diagnostics(object):
    """What ``diagnostics()`` returns: do the chains agree with each other, and how many independent draws are they worth.

    Built from the per-part sums of ``DeviceChainStats.read()`` -- ``parts`` = [(n_chains, n_states_per_chain, Sw, Sm, Sq,
    Sv), ...], already summed over ranks, all about ``shift``.  With ``M`` = chains x parts (``n_chains``), ``n`` = states
    per chain and part (``n_states``), m = a chain's (weighted) mean and v its variance normalised by its weight, per
    dimension:

      chain_mean_avg = sum m / M                       between = (sum m^2 - M chain_mean_avg^2) / (M - 1)
      within = sum v / M                               var_plus = within + between
      rhat = sqrt((n - 1) / n * var_plus / within)     the potential scale reduction: the textbook
                                                       sqrt(((n - 1) / n W + B / n) / W) with W = n / (n - 1) within and
                                                       B / n = between, so one expression serves weighted chains too
      ess_per_chain = var_plus / between               the variance of the chain means across chains IS var / ESS
      ess = M * ess_per_chain                          NOT capped at M * n: antithetic chains may exceed it
      mean = shift + chain_mean_avg

    and the scalars ``total_weight`` (sum of all weights), ``grad_evals`` (the increase of ``distribution.dEdX_count`` over
    the call), ``ess_per_grad = ess / grad_evals``, plus the raw sums ``Sw, Sm, Sq, Sv`` (added over parts) and ``parts``.
    Every chain counts equally whatever its total holding time: chain_mean_avg is the plain average of the chain means,
    not the pooled time average of ``expectations()``.  With ``M`` = 10^5 chains the relative standard error of
    ``between``, and so of the ESS, is sqrt(2 / (M - 1)) = 0.45 %."""

    def __init__(self, parts, shift, grad_evals=0):
        self.parts = parts
        self.shift = shift
        self.n_chains = M = int(sum(p[0] for p in parts))
        self.n_states = n = int(parts[0][1])
        self.Sw = self.total_weight = float(sum(p[2] for p in parts))
        self.Sm = sum(p[3] for p in parts)
        self.Sq = sum(p[4] for p in parts)
        self.Sv = sum(p[5] for p in parts)
        self.chain_mean_avg = self.Sm / M
        self.between = (self.Sq - M * self.chain_mean_avg * self.chain_mean_avg) / (M - 1)
        self.within = self.Sv / M
        self.var_plus = self.within + self.between
        self.rhat = np.sqrt((n - 1.0) / n * self.var_plus / self.within)
        self.ess_per_chain = self.var_plus / self.between
        self.ess = M * self.ess_per_chain
        self.mean = shift + self.chain_mean_avg
        self.grad_evals = int(grad_evals)
        self.ess_per_grad = self.ess / self.grad_evals if self.grad_evals else np.full_like(self.ess, np.nan)


class Marginals(object):
    """What ``marginals()`` returns: one weighted histogram per dimension, and the quantiles read off it.  Pure NumPy.

    Built from the integer tables of ``DeviceHistogram.read()`` (already summed over ranks): ``counts`` and ``units``
    (ndims, bins + 2) uint64 -- column 0 holds what fell below ``lo`` (and NaN), column bins + 1 what fell at or above
    ``hi``, columns 1 .. bins the bins between, all of one width per dimension -- the total ``W_units`` and the number of
    states ``n_states``.  ``quantum`` q is the weight of one unit:

      mass = q * units                                 |mass - the bin's sum of weights| <= 0.5 q counts
      total_weight = q * W_units                       every row of units adds up to W_units, exactly
      edges (ndims, bins + 1)                          edges[d][j] = lo_d + j (hi_d - lo_d) / bins
      density (ndims, bins)                            mass of the inner bins / (total_weight * bin width)
      out_of_range (ndims,)                            the share of the weight in the two outer bins

    ``cdf(x)`` is the piecewise-linear distribution function through the bin edges: exact (as a ratio of the integer sums)
    at an edge, linear inside a bin, NaN outside [lo, hi].  ``quantile(p)`` is its inverse and raises ValueError when the
    answer lies in an outer bin, where the histogram has no resolution; ``median`` and the equal-tailed
    ``interval(level)`` are quantiles.  The device assigns bins by (x - lo) * (bins / (hi - lo)) in float64, so a state
    within a rounding error of an edge may sit on either side of it."""

    def __init__(self, lo, hi, bins, quantum, counts, units, W_units, n_states):
        self.lo = np.asarray(lo, dtype=np.float64).reshape(-1)
        self.hi = np.asarray(hi, dtype=np.float64).reshape(-1)
        self.bins, self.quantum = int(bins), float(quantum)
        self.ndims = self.lo.size
        self.counts = np.asarray(counts, dtype=np.uint64).reshape(self.ndims, self.bins + 2)
        self.units = np.asarray(units, dtype=np.uint64).reshape(self.ndims, self.bins + 2)
        self.W_units, self.n_states = int(W_units), int(n_states)
        self.mass = self.quantum * self.units.astype(np.float64)
        self.total_weight = self.quantum * float(self.W_units)
        self.width = (self.hi - self.lo) / self.bins
        self.edges = self.lo[:, None] + np.arange(self.bins + 1)[None, :] * self.width[:, None]
        self.edges[:, -1] = self.hi
        W = float(self.W_units) if self.W_units else np.nan
        self.density = self.units[:, 1:-1].astype(np.float64) / (W * self.width[:, None])
        self.out_of_range = (self.units[:, 0].astype(np.float64) + self.units[:, -1].astype(np.float64)) / W
        # the distribution function at the edges: units below the edge (the underflow bin included) / all units
        self._F = np.cumsum(self.units[:, :-1], axis=1, dtype=np.uint64).astype(np.float64) / W

    def _per_dim(self, v):
        """scalar, (K,), (ndims, K) -> (ndims, K) and the shape to return"""
        v = np.asarray(v, dtype=np.float64)
        if v.ndim == 0:
            return np.broadcast_to(v, (self.ndims, 1)), (self.ndims,)
        if v.ndim == 1:
            return np.broadcast_to(v[None, :], (self.ndims, v.size)), (self.ndims, v.size)
        if v.ndim == 2 and v.shape[0] == self.ndims:
            return v, v.shape
        raise ValueError('expected a scalar, a vector (applied to every dimension) or an (ndims, K) array, got shape %r' % (v.shape,))

    def cdf(self, x):
        """x: a scalar or a (K,) vector, taken for every dimension, or (ndims, K).  Returns (ndims,), (ndims, K)."""
        X, shape = self._per_dim(x)
        out = np.full(X.shape, np.nan)
        for d in range(self.ndims):
            e, F, xd = self.edges[d], self._F[d], X[d]
            ok = (xd >= e[0]) & (xd <= e[-1])
            j = np.clip(np.searchsorted(e, xd[ok], side='right') - 1, 0, self.bins - 1)
            frac = (xd[ok] - e[j]) / (e[j + 1] - e[j])
            out[d, ok] = np.where(frac >= 1.0, F[j + 1], F[j] + frac * (F[j + 1] - F[j]))
        return out.reshape(shape)

    def quantile(self, p):
        """p in [0, 1]: a scalar or a (K,) vector, taken for every dimension, or (ndims, K).  The smallest x with
        cdf(x) = p.  ValueError when it lies below ``lo`` or above ``hi`` in some dimension."""
        P, shape = self._per_dim(p)
        if np.any(~((P >= 0.0) & (P <= 1.0))):
            raise ValueError('p must be in [0, 1]')
        out = np.empty(P.shape)
        for d in range(self.ndims):
            e, F, pd = self.edges[d], self._F[d], P[d]
            if np.any(pd < F[0]) or np.any(pd > F[-1]):
                raise ValueError('dimension %d: the quantile lies in an outer bin (%.3g of the weight below lo = %g, %.3g at '
                                 'or above hi = %g): widen the range' % (d, F[0], e[0], 1.0 - F[-1], e[-1]))
            i = np.searchsorted(F, pd, side='left')          # F[i - 1] < p <= F[i]
            j = np.maximum(i, 1) - 1
            rise = F[j + 1] - F[j]
            frac = np.where(i == 0, 0.0, (pd - F[j]) / np.where(rise > 0, rise, 1.0))
            out[d] = np.where(frac >= 1.0, e[j + 1], e[j] + frac * (e[j + 1] - e[j]))
        return out.reshape(shape)

    @property
    def median(self):
        return self.quantile(0.5)

    def interval(self, level=0.95):
        """the equal-tailed interval that holds ``level`` of the weight: (lower (ndims,), upper (ndims,))"""
        if not 0.0 < level < 1.0:
            raise ValueError('level must be in (0, 1)')
        tail = 0.5 * (1.0 - level)
        return self.quantile(tail), self.quantile(1.0 - tail)


class JointMarginals(object):
    """What ``joint_marginals()`` returns: one weighted two-dimensional histogram per pair of dimensions.  Pure NumPy.

    Built from the integer tables of ``DevicePairHistogram.read()`` (already summed over ranks): ``counts`` and ``units``
    (P, bins + 2, bins + 2) uint64, indexed [pair][bin of the pair's SECOND dimension][bin of its FIRST dimension] -- per
    axis bin 0 holds what fell below ``lo`` (and NaN), bin bins + 1 what fell at or above ``hi``, bins 1 .. bins the bins
    between -- the total ``W_units`` and the number of states ``n_states``.  ``pairs`` (P, 2) are the dimensions (i, j),
    ``lo`` and ``hi`` (P, 2) the range per pair and axis (column 0: i), ``quantum`` q the weight of one unit:

      mass = q * units                                 |mass - the cell's sum of weights| <= 0.5 q counts
      total_weight = q * W_units                       every pair's table adds up to W_units, exactly
      edges_x, edges_y (P, bins + 1)                   the bin edges of the i axis and of the j axis
      density (P, bins, bins)                          mass of the inner cells / (total_weight * cell area), [pair][j bin][i bin]:
                                                       its sum times the cell area is 1 - out_of_range
      out_of_range (P,)                                the share of the weight in any outer cell

    ``marginal(p, axis)`` is the ``Marginals`` of one axis of pair p (0: i, 1: j), from the tables summed over the other
    axis: the integers ``marginals()`` counts for that dimension on the same run and range.  ``hdr(level)`` is the
    highest-density region."""

    def __init__(self, pairs, lo, hi, bins, quantum, counts, units, W_units, n_states):
        self.pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
        self.n_pairs = P = self.pairs.shape[0]
        self.lo = np.array(np.broadcast_to(np.asarray(lo, dtype=np.float64), (P, 2)))
        self.hi = np.array(np.broadcast_to(np.asarray(hi, dtype=np.float64), (P, 2)))
        self.bins, self.quantum = int(bins), float(quantum)
        B = self.bins
        self.counts = np.asarray(counts, dtype=np.uint64).reshape(P, B + 2, B + 2)
        self.units = np.asarray(units, dtype=np.uint64).reshape(P, B + 2, B + 2)
        self.W_units, self.n_states = int(W_units), int(n_states)
        self.mass = self.quantum * self.units.astype(np.float64)
        self.total_weight = self.quantum * float(self.W_units)
        self.width = (self.hi - self.lo) / B                                  # (P, 2)
        steps = np.arange(B + 1)[None, :]
        self.edges_x = self.lo[:, :1] + steps * self.width[:, :1]
        self.edges_y = self.lo[:, 1:] + steps * self.width[:, 1:]
        self.edges_x[:, -1], self.edges_y[:, -1] = self.hi[:, 0], self.hi[:, 1]
        W = float(self.W_units) if self.W_units else np.nan
        inner = self.units[:, 1:-1, 1:-1]
        self.cell_area = self.width[:, 0] * self.width[:, 1]
        self.density = inner.astype(np.float64) / (W * self.cell_area[:, None, None])
        self._inner_units = inner.reshape(P, -1).sum(axis=1, dtype=np.uint64)
        outer = self.units.reshape(P, -1).sum(axis=1, dtype=np.uint64) - self._inner_units
        self.out_of_range = outer.astype(np.float64) / W

    def marginal(self, p, axis):
        """the ``Marginals`` (one dimension) of pair ``p``'s axis 0 (its first dimension) or 1 (its second)"""
        p, axis = int(p), int(axis)
        if not 0 <= p < self.n_pairs or axis not in (0, 1):
            raise ValueError('p must be in [0, %d) and axis 0 or 1' % self.n_pairs)
        over = 0 if axis == 0 else 1                       # tables are [j bin][i bin]: the i axis remains after summing over j
        return Marginals([self.lo[p, axis]], [self.hi[p, axis]], self.bins, self.quantum,
                         self.counts[p].sum(axis=over, dtype=np.uint64)[None, :], self.units[p].sum(axis=over, dtype=np.uint64)[None, :],
                         self.W_units, self.n_states)

    def hdr(self, level=0.9):
        """The highest-density region: per pair the smallest set of inner cells, taken in order of falling density, that
        holds at least ``level`` of the total weight.  Returns ``(threshold (P,), mask (P, bins, bins) bool)``: the density
        of the last cell taken, and the cells, indexed as ``density``.  Cells of equal density are taken in order of their
        (flattened) index.  ValueError when ``out_of_range[p] > 1 - level``: the inner cells do not hold that much."""
        from fractions import Fraction
        if not 0.0 < level <= 1.0:
            raise ValueError('level must be in (0, 1]')
        if not self.W_units:
            raise ValueError('the tables hold no weight')
        need = Fraction(level) * self.W_units
        need = int(need) + (1 if need != int(need) else 0)                 # units the region must hold: ceil(level * W_units)
        B = self.bins
        threshold, mask = np.empty(self.n_pairs), np.zeros((self.n_pairs, B * B), dtype=bool)
        for p in range(self.n_pairs):
            if int(self._inner_units[p]) < need:
                raise ValueError('pair %d (%d, %d): %.3g of the weight lies outside the range, more than 1 - level = %.3g: '
                                 'widen the range' % (p, self.pairs[p, 0], self.pairs[p, 1], self.out_of_range[p], 1.0 - level))
            u = self.units[p, 1:-1, 1:-1].reshape(-1)
            order = np.argsort(u.max() - u, kind='stable')                 # falling units (exact in uint64), ties by cell index
            cum = np.cumsum(u[order], dtype=np.uint64)
            k = int(np.searchsorted(cum, np.uint64(need), side='left'))
            mask[p, order[:k + 1]] = True
            threshold[p] = self.density[p].reshape(-1)[order[k]]
        return threshold, mask.reshape(self.n_pairs, B, B)


class Occupancy(object):
    """What ``occupancy()`` returns: how the chains spend their time in, and move between, the cells of ``centres`` -- cell
    m < M the Voronoi cell of centre m (cut to its ball where a radius was given), cell M "outside".

    Built from the integer tables of ``DeviceOccupancy.read()`` (``tables``: count, mass, from_count, from_mass (M + 1,),
    trans (M + 1, M + 1), W_units, chains_by_switches (17,), chains_by_cells (M + 1,)), the quantum ``q`` of the masses, the
    ``centres``, ``n_states`` and ``grad_evals`` (the increase of ``distribution.dEdX_count`` over the call).  Everything
    below is float64 NumPy on (M + 1)^2 numbers:

      weight               mass / W_units: the (dwell-weighted) share of the time spent in each cell
      transition_matrix()  trans row-normalised; a cell with no departure keeps the identity row
      rate_matrix()        Q[a][b] = trans[a][b] / (q from_mass[a]) off the diagonal, Q[a][a] = -sum of its row: the
                           maximum-likelihood generator of the cell process in process time (a row without departures is
                           zero); for the discrete-time samplers (unit weights) it is transition_matrix() - I
      stationary()         the left null vector of Q on the cells that were visited (0 elsewhere), summing to 1
      spectral_gap()       1 - |lambda_2| of the transition matrix on the visited cells (the reference's sg(); NaN with
                           fewer than two visited cells)
      relaxation_time()    -1 / Re lambda_2(Q) on the visited cells, in process time (inf when a second eigenvalue is 0)
      relaxation_grads()   the same in gradient evaluations: relaxation_time() * grad_evals / (q W_units)
      mean_residence       q from_mass[a] / (departures from a to another cell): the mean time of a stay (inf: none left)
      crossings            transitions between different cells (the outside cell is a cell); crossings_per_grad
      chains_by_switches   chains with 0 .. 15 and with >= 16 switches;  never_left: the fraction with none
      chains_by_cells      chains that saw exactly c distinct cells < M"""

    def __init__(self, tables, q, centres, n_states, grad_evals=0):
        self.tables = tables
        self.quantum = q = float(q)
        self.centres = np.asarray(centres, dtype=np.float64)
        self.n_cells = self.centres.shape[0] + 1
        self.n_states, self.grad_evals = int(n_states), int(grad_evals)
        self.counts = np.asarray(tables['count'], dtype=np.uint64)
        self.units = np.asarray(tables['mass'], dtype=np.uint64)
        self.trans = np.asarray(tables['trans'], dtype=np.uint64)
        self.from_counts = np.asarray(tables['from_count'], dtype=np.uint64)
        self.from_units = np.asarray(tables['from_mass'], dtype=np.uint64)
        self.W_units = int(tables['W_units'])
        self.total_weight = q * self.W_units
        self.chains_by_switches = np.asarray(tables['chains_by_switches'], dtype=np.uint64)
        self.chains_by_cells = np.asarray(tables['chains_by_cells'], dtype=np.uint64)
        self.n_chains = int(self.chains_by_switches.sum())
        self.weight = self.units.astype(np.float64) / self.W_units if self.W_units else np.full(self.n_cells, np.nan)
        self.visited = self.counts > 0
        T = self.trans.astype(np.float64)
        self.crossings = int(self.trans.sum() - np.trace(self.trans))
        self.crossings_per_grad = self.crossings / float(self.grad_evals) if self.grad_evals else np.nan
        self.never_left = float(self.chains_by_switches[0]) / self.n_chains if self.n_chains else np.nan
        exits = T.sum(axis=1) - np.diag(T)
        with np.errstate(divide='ignore', invalid='ignore'):
            self.mean_residence = np.where(exits > 0, q * self.from_units.astype(np.float64) / exits, np.inf)

    def transition_matrix(self):
        T = self.trans.astype(np.float64)
        n = self.from_counts.astype(np.float64)
        P = np.eye(self.n_cells)
        rows = n > 0
        P[rows] = T[rows] / n[rows, None]
        return P

    def rate_matrix(self):
        T = self.trans.astype(np.float64)
        t = self.quantum * self.from_units.astype(np.float64)
        Q = np.zeros((self.n_cells, self.n_cells))
        rows = t > 0
        Q[rows] = T[rows] / t[rows, None]
        np.fill_diagonal(Q, 0.0)
        np.fill_diagonal(Q, -Q.sum(axis=1))
        return Q

    def _on_visited(self, A):
        v = np.flatnonzero(self.visited)
        return A[np.ix_(v, v)], v

    def stationary(self):
        Q, v = self._on_visited(self.rate_matrix())
        pi = np.zeros(self.n_cells)
        if v.size:
            # pi Q = 0 with sum pi = 1, in the least-squares sense (one solution when the visited cells communicate)
            A = np.vstack([Q.T, np.ones((1, v.size))])
            rhs = np.zeros(v.size + 1)
            rhs[-1] = 1.0
            pi[v] = np.linalg.lstsq(A, rhs, rcond=None)[0]
        return pi

    def spectral_gap(self):
        P, v = self._on_visited(self.transition_matrix())
        if v.size < 2:
            return np.nan
        lam = np.sort(np.abs(np.linalg.eigvals(P)))[::-1]
        return float(1.0 - lam[1])

    def relaxation_time(self):
        Q, v = self._on_visited(self.rate_matrix())
        if v.size < 2:
            return np.nan
        re = np.sort(np.linalg.eigvals(Q).real)[::-1]      # 0 first, then the slowest decay
        return float(-1.0 / re[1]) if re[1] < 0 else np.inf

    def relaxation_grads(self):
        if not (self.grad_evals and self.W_units):
            return np.nan
        return self.relaxation_time() * self.grad_evals / self.total_weight


class AutocorrelationTimes(object):
    """What ``Paths.iat()`` returns, per dimension: ``rho`` (max_lag + 1, ndims), ``tau`` (grid steps), ``tau_time``
    (process time), ``tau_grad_evals`` (gradient evaluations per chain), ``window`` (lags that entered tau), ``converged``;
    ``n`` grid points and ``max_lag`` as used."""

    def __init__(self, rho, tau, tau_time, tau_grad_evals, window, converged, n, max_lag):
        self.rho, self.tau, self.tau_time, self.tau_grad_evals = rho, tau, tau_time, tau_grad_evals
        self.window, self.converged, self.n, self.max_lag = window, converged, int(n), int(max_lag)


class EffectiveSamples(object):
    """What ``Paths.ess()`` returns, per dimension: ``ess`` = n_chains n / tau, ``ess_per_grad`` = ess over the run's
    gradient evaluations (all chains), and the ``tau``, ``window`` and ``converged`` they come from."""

    def __init__(self, ess, ess_per_grad, tau, window, converged):
        self.ess, self.ess_per_grad, self.tau, self.window, self.converged = ess, ess_per_grad, tau, window, converged


class Paths(object):
    """What ``paths()`` returns: the jump process of every chain sampled on the uniform time grid t_j = j ``dt``,
    j < ``n_grid`` -- a fair sample with its time order kept.  The grid stays on the device (csrc/timegrid.hip) until
    ``close()``.

      dt, n_grid            the grid
      covered               the grid points every chain has reached (the minimum over chains and ranks): the usable length
      mean_time             the mean over chains of the time a chain's recorded states span (the sum of their holding times)
      grad_evals_per_time   gradient evaluations per chain / mean_time: what one unit of process time costs
      n_chains              chains (all ranks)

    ``read(n)`` downloads the first ``n`` (default ``covered``) grid points as (ndims, nbatch, n) float64 -- the columns of
    this rank in a sharded run.  ``autocor(n, linear)`` is the autocorrelation along the grid, taken on the device:
    ``linear=False`` is ``fft_autocor`` of that array (circular, 1 at lag 0), ``linear=True`` the lag-product means
    np.mean(x[:, :, :-k] * x[:, :, k:]) divided by the one of lag 0; lag k is process time k ``dt``.  Both refuse
    ``n > covered``: a grid point some chain has not reached is no sample.

    Per dimension, also on the device (csrc/lagcov.hip) and over all ranks: ``lag_cov(max_lag, n, center)`` are the linear
    lag sums of the (centred) series, ``iat(max_lag, n)`` the autocorrelation, the integrated autocorrelation time and its
    truncation window (``misc.autocor.integrated_autocorrelation_time``), ``ess(max_lag, n)`` the effective sample size
    ``n_chains n / tau`` and what one effective sample costs in gradient evaluations."""

    def __init__(self, grid, dt, n_grid, covered, mean_time, grad_evals_per_chain, n_chains, comm=None):
        self._grid, self._comm = grid, comm
        self.dt, self.n_grid, self.covered = float(dt), int(n_grid), int(covered)
        self.mean_time = float(mean_time)
        self.n_chains = int(n_chains)
        self.grad_evals_per_chain = float(grad_evals_per_chain)
        self.grad_evals_per_time = self.grad_evals_per_chain / self.mean_time if self.mean_time > 0 else float('nan')

    def _length(self, n):
        n = self.covered if n is None else int(n)
        if n < 1 or n > self.covered:
            raise ValueError('n must be in [1, covered = %d], got %d: grid points beyond `covered` are not reached by every '
                             'chain (a longer run, a larger dt or a smaller n_grid covers more)' % (self.covered, n))
        if self._grid is None:
            raise ValueError('this Paths was closed')
        return n

    def read(self, n=None):
        n = self._length(n)
        return self._grid.read(0, n, stacked=True)

    def autocor(self, n=None, linear=False):
        n = self._length(n)
        sums = self._grid.autocor(0, n, linear=linear)
        if self._comm is not None:
            sums = self._comm.allreduce_f64(sums)         # column shards add their lag sums
        if linear:
            sums = sums / (n - np.arange(n, dtype=np.float64))
        return sums / sums[0]

    def lag_cov(self, max_lag, n=None, center=True):
        """``(A, S, shift)``: ``A[k, d] = sum over chains and t < n - k of u_t u_{t+k}``, k = 0 .. ``max_lag`` <= min(n - 1,
        256), and ``S[d] = sum u_t`` with u = x - shift[d], over the first ``n`` (default ``covered``) grid points of every
        chain of every rank.  ``center=True`` takes shift = the mean over chains and grid points, from a first device pass
        with ``max_lag`` 0 (its S, added over the ranks, over ``n_chains n``); ``center=False`` takes zeros.  A refused
        ``max_lag`` raises ValueError with the library's message."""
        n = self._length(n)
        shift = np.zeros(self._grid.ndims)
        if center:
            S = self._grid.lag_cov(0, n, 0)[1]
            if self._comm is not None:
                S = self._comm.allreduce_f64(S)
            shift = S / (float(self.n_chains) * n)
        A, S = self._grid.lag_cov(0, n, max_lag, shift if center else None)
        if self._comm is not None:                        # column shards add their lag sums
            A = self._comm.allreduce_f64(A.ravel()).reshape(A.shape)
            S = self._comm.allreduce_f64(S)
        return A, S, shift

    def iat(self, max_lag=None, n=None):
        """Per dimension: the autocorrelation ``rho`` (max_lag + 1, ndims) of the centred series, the integrated
        autocorrelation time ``tau`` in grid steps, ``tau_time = tau dt`` in process time, ``tau_grad_evals = tau dt
        grad_evals_per_time`` in gradient evaluations per chain, the truncation ``window`` and ``converged`` (False: the
        window ended before the pair sums turned non-positive -- take a larger ``max_lag`` or a longer run); see
        ``misc.autocor.integrated_autocorrelation_time``.  ``max_lag=None`` takes min(n - 1, 256)."""
        from ..misc.autocor import integrated_autocorrelation_time
        n = self._length(n)
        max_lag = min(n - 1, 256) if max_lag is None else int(max_lag)
        A, _, _ = self.lag_cov(max_lag, n, center=True)
        rho, tau, window, converged = integrated_autocorrelation_time(A, n, self.n_chains)
        return AutocorrelationTimes(rho, tau, tau * self.dt, tau * self.dt * self.grad_evals_per_time, window, converged, n,
                                    max_lag)

    def ess(self, max_lag=None, n=None):
        """Per dimension: ``ess = n_chains n / tau`` and ``ess_per_grad = ess / (n_chains grad_evals_per_chain)``, effective
        samples per gradient evaluation of the run; ``tau``, ``window`` and ``converged`` of ``iat`` ride along."""
        t = self.iat(max_lag, n)
        ess = float(self.n_chains) * t.n / t.tau
        return EffectiveSamples(ess, ess / (self.n_chains * self.grad_evals_per_chain), t.tau, t.window, t.converged)

    def close(self):
        if self._grid is not None:
            self._grid.close()
            self._grid = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Functionals(object):
    """What ``HMCBase.functionals()`` returns: the description of K functionals of the state,
        S[j] = sum_d stat_j(x_d, d; p),   g[k] = value_k(S; p)
    -- ``values`` (K C expressions of ``S[j]`` and ``p[m]``), ``stats`` (J <= 8 C expressions of ``x``, ``d`` and ``p[m]``),
    ``params`` (float64), ``names`` (K strings) and ``n_values`` = K -- checked to compile, bound to no device.  Pass it
    as ``of=`` to ``expectations()``, ``diagnostics()``, ``marginals()`` or ``joint_marginals()``: their results then have K "dimensions"."""

    def __init__(self, values, stats=(), params=(), names=None):
        self.values = [values] if isinstance(values, str) else [str(v) for v in values]
        self.stats = [stats] if isinstance(stats, str) else [str(t) for t in stats]
        self.params = np.ascontiguousarray(np.atleast_1d(np.asarray(params, dtype=np.float64)).ravel())
        self.n_values = len(self.values)
        self.names = ['g%d' % k for k in range(self.n_values)] if names is None else [str(n) for n in names]
        if len(self.names) != self.n_values:
            raise ValueError('names must have one entry per value (%d), got %d' % (self.n_values, len(self.names)))

    def slot_bytes(self, nparticles):
        """bytes of one slot of the derived ring: rows padded to 64, values to an even count, float64"""
        return (int(nparticles) + 63) // 64 * 64 * ((self.n_values + 1) // 2 * 2) * 8


class EnergyObservables(object):
    """What ``HMCBase.energy_observables()`` returns: the description of the K = 3 energy observables of a recorded state,
        E = the potential energy,   grad_sq = sum_d (dE/dx_d)^2,   virial = sum_d x_d dE/dx_d
    -- as the sampler's own device evaluation of the stored state gives them (csrc/energy_observables.hpp).  It stands
    where a ``Functionals`` stands: pass it as ``of=`` to ``expectations()``, ``diagnostics()``, ``marginals()`` or
    ``joint_marginals()``, whose results then have these 3 "dimensions" (``names``)."""

    n_values = 3
    names = ['E', 'grad_sq', 'virial']

    def slot_bytes(self, nparticles):
        """bytes of one slot of the derived ring: rows padded to 64, [E, grad_sq, virial, 0.0] float64"""
        return (int(nparticles) + 63) // 64 * 64 * 4 * 8


class Projections(object):
    """What ``HMCBase.projections()`` returns: the description of K linear read-outs of the state,
        u[k] = b[k] + sum_d A[k][d] x_d,   g[k] = link(u[k], k; p)
    -- ``A`` (K, ndims) float64, ``b`` (K,) float64, ``link`` (one C expression of ``u``, ``k`` and ``p[m]``, or None for
    g = u), ``params`` (float64), ``names`` (K strings, default 'u0', 'u1', ...) and ``n_values`` = K <= 512 -- checked
    for shape and finiteness, bound to no device.  It stands where a ``Functionals`` stands: pass it as ``of=`` to
    ``expectations()``, ``diagnostics()``, ``marginals()`` or ``joint_marginals()``, whose results then have K
    "dimensions".  ``Projections.principal`` builds the principal axes of a measured covariance."""

    MAX_VALUES = 512

    def __init__(self, A, b=None, link=None, params=(), names=None, ndims=None):
        A = np.asarray(A, dtype=np.float64)
        if A.ndim == 1:
            A = A.reshape(1, -1)
        if A.ndim != 2 or A.shape[1] < 1:
            raise ValueError('A must be (K, ndims) or (ndims,), got an array of shape %r' % (A.shape,))
        if ndims is not None and A.shape[1] != int(ndims):
            raise ValueError('A must have ndims = %d columns, got %d' % (int(ndims), A.shape[1]))
        K = A.shape[0]
        if not 1 <= K <= self.MAX_VALUES:
            raise ValueError('the number of values K must be in [1, %d], got %d' % (self.MAX_VALUES, K))
        if b is None:
            b = np.zeros(K)
        else:
            b = np.asarray(b, dtype=np.float64)
            if b.size not in (1, K) or b.ndim > 1:
                raise ValueError('b must be a scalar or have K = %d entries, got shape %r' % (K, b.shape))
            b = np.broadcast_to(b.reshape(-1), (K,))
        params = np.atleast_1d(np.asarray(params, dtype=np.float64)).ravel()
        for what, v in (('A', A), ('b', b), ('params', params)):
            if not np.all(np.isfinite(v)):
                raise ValueError('%s must be finite' % what)
        if link is not None and (not isinstance(link, str) or not link.strip() or ';' in link):
            raise ValueError('link must be one C expression of u, k and p[m] (a non-empty string without semicolons), got %r' % (link,))
        self.A, self.b, self.params = np.ascontiguousarray(A), np.ascontiguousarray(b), np.ascontiguousarray(params)
        self.link = link
        self.n_values = K
        self.names = ['u%d' % k for k in range(K)] if names is None else [str(n) for n in names]
        if len(self.names) != K:
            raise ValueError('names must have one entry per value (%d), got %d' % (K, len(self.names)))

    def slot_bytes(self, nparticles):
        """bytes of one slot of the derived ring: rows padded to 64, values to an even count, float64"""
        return (int(nparticles) + 63) // 64 * 64 * ((self.n_values + 1) // 2 * 2) * 8

    @classmethod
    def principal(cls, expectations, k=None, whiten=False, names=None):
        """The principal axes of a measured covariance as projections: from an ``Expectations`` with a ``cov``
        (``expectations(n, cov=True)``), row i of ``A`` is the eigenvector of ``cov`` with the i-th largest eigenvalue
        (``numpy.linalg.eigh``), its sign fixed so that its largest-magnitude entry is positive, and ``b = -A mean``: the
        values are the centred coordinates of the state along the widest axes.  ``k``: keep the first k axes (default
        all).  ``whiten``: divide row i by sqrt(eigenvalue_i), so that the values have unit variance under the measured
        covariance.  ValueError: ``cov`` is None; ``whiten`` with an eigenvalue <= 0; k outside [1, ndims]."""
        cov = getattr(expectations, 'cov', None)
        if cov is None:
            raise ValueError('principal axes need a covariance: take the Expectations with cov=True')
        cov = np.asarray(cov, dtype=np.float64)
        mean = np.asarray(expectations.mean, dtype=np.float64).reshape(-1)
        D = mean.size
        if cov.shape != (D, D):
            raise ValueError('cov must be (%d, %d), got %r' % (D, D, cov.shape))
        k = D if k is None else int(k)
        if not 1 <= k <= D:
            raise ValueError('k must be in [1, ndims = %d], got %d' % (D, k))
        lam, vec = np.linalg.eigh(0.5 * (cov + cov.T))
        order = np.argsort(lam)[::-1][:k]
        lam, A = lam[order], vec[:, order].T.copy()
        big = np.argmax(np.abs(A), axis=1)
        A *= np.where(A[np.arange(k), big] < 0, -1.0, 1.0)[:, None]
        if whiten:
            if np.any(lam <= 0):
                raise ValueError('whiten needs positive eigenvalues, the smallest kept is %g' % lam.min())
            A /= np.sqrt(lam)[:, None]
        return cls(A, -A.dot(mean), names=names)


class Temperature(object):
    """What ``HMCBase.temperature()`` returns: the virial thermometer of a run, from the ``Diagnostics`` of its energy
    observables (value 0 ``E``, 1 ``grad_sq``, 2 ``virial``):

      T = mean[virial] / ndims                              1 for chains that keep exp(-E)
      stderr = sqrt(var_plus[virial] / ess[virial]) / ndims    the standard error of T (multi-chain ESS)
      z = (T - 1) / stderr

    and ``mean_energy``, ``mean_grad_sq``, ``rhat_energy`` (the R-hat of E: the ``lp__`` check), ``ndims`` and the
    ``diagnostics`` object itself."""

    def __init__(self, diagnostics, ndims):
        self.diagnostics = d = diagnostics
        self.ndims = ndims = int(ndims)
        self.T = d.mean[2] / ndims
        self.stderr = np.sqrt(d.var_plus[2] / d.ess[2]) / ndims
        self.z = (self.T - 1) / self.stderr
        self.mean_energy = d.mean[0]
        self.mean_grad_sq = d.mean[1]
        self.rhat_energy = d.rhat[0]


class SteinDiscrepancy(object):
    """What ``HMCBase.stein_discrepancy()`` returns: the kernel Stein discrepancy of the ensemble against exp(-E) at every
    evaluated recorded state, from the four device sums of each (include/mjhmc_hip.h: mjhmc_stein_evaluate).  Arrays of
    one entry per evaluated state:

      ``iterations``  index of the recorded state within the run (0, every, 2 every, ...)
      ``W, W2, S, Sd``  sum w, sum w^2, sum_ij w_i w_j k_p(x_i, x_j) and its diagonal sum_i w_i^2 k_p(x_i, x_i)
      ``v = S / W^2``   the V-statistic (>= 0 up to rounding);  ``ksd = sqrt(max(v, 0))``
      ``u = (S - Sd) / (W^2 - W2)``  the U-statistic: unbiased, mean zero under the target; NaN where W^2 == W2 (one particle)

    and ``n_particles``, ``c`` (the IMQ scale) and ``mean_u`` (the mean of ``u`` over the evaluated states, NaN-aware)."""

    def __init__(self, iterations, W, W2, S, Sd, n_particles, c):
        self.iterations = np.asarray(iterations, dtype=np.int64).reshape(-1)
        self.W, self.W2, self.S, self.Sd = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (W, W2, S, Sd))
        self.n_particles, self.c = int(n_particles), float(c)
        WW = self.W * self.W
        self.v = self.S / WW
        self.ksd = np.sqrt(np.maximum(self.v, 0.0))
        den = WW - self.W2
        ok = den != 0
        self.u = np.full(self.W.shape, np.nan)
        self.u[ok] = (self.S[ok] - self.Sd[ok]) / den[ok]

    @property
    def mean_u(self):
        ok = ~np.isnan(self.u)
        return float(np.mean(self.u[ok])) if ok.any() else float('nan')


def merge_log_sum_exp(mx1, se1, mx2, se2):
    """Two (max, sum of w exp(t - max)) pairs as one: mx = max(mx1, mx2), se = se1 exp(mx1 - mx) + se2 exp(mx2 - mx); an
    empty pair is (-inf, 0) and two empty pairs stay empty (no -inf - (-inf) is formed).  Arrays broadcast."""
    mx1, se1, mx2, se2 = np.broadcast_arrays(*(np.asarray(a, dtype=np.float64) for a in (mx1, se1, mx2, se2)))
    mx = np.maximum(mx1, mx2)
    base = np.where(np.isneginf(mx), 0.0, mx)               # (an empty pair has se = 0: its factor does not matter)
    with np.errstate(under='ignore'):
        se = se1 * np.exp(np.where(np.isneginf(mx1), -np.inf, mx1 - base)) + \
            se2 * np.exp(np.where(np.isneginf(mx2), -np.inf, mx2 - base))
    return mx, se


class PointwiseStatistics(object):
    """What ``pointwise()`` returns: statistics of M values h_m(u_j, j) per expert j of a linear-model energy over the
    recorded ensemble, from the device sums (include/mjhmc_hip.h: mjhmc_pointwise_read) ``W`` = sum w, ``S1`` = sum w t,
    ``S2`` = sum w t^2 and the pairs ``lme_max`` = max t, ``lme_sum`` = sum w exp(t - lme_max), each (M, K):

      ``mean = S1 / W``
      ``var = max(S2 / W - mean^2, 0)``                     the weighted POPULATION variance (no n - 1 correction)
      ``log_mean_exp = log(lme_sum / W) + lme_max``         log of the weighted mean of exp(t), finite where exp(t)
                                                            underflows; NaN in the rows that did not ask for it, -inf
                                                            for an expert that has seen no weight

    plus ``n_states``, the number of (slot, particle) states, ``total_weight`` = W and ``flags`` (which rows asked).
    ``group_pointwise()`` returns one of these per value, with the arrays of that value alone: (G,) per group, (G, C) per
    member."""

    def __init__(self, W, S1, S2, lme_max, lme_sum, n_states, log_mean_exp):
        self.W, self.S1, self.S2, self.lme_max, self.lme_sum = float(W), S1, S2, lme_max, lme_sum
        self.total_weight, self.n_states = self.W, int(n_states)
        self.flags = np.array([bool(f) for f in log_mean_exp], dtype=bool).reshape(-1)
        with np.errstate(divide='ignore', invalid='ignore'):
            self.mean = S1 / self.W
            self.var = np.maximum(S2 / self.W - self.mean * self.mean, 0.0)
            self.log_mean_exp = np.where(np.isneginf(lme_max), -np.inf, np.log(lme_sum / self.W) + lme_max)
        if self.flags.size == 1:            # (one value, and the arrays may be its own: group_pointwise()'s (G,) and (G, C))
            if not self.flags[0]:
                self.log_mean_exp[...] = np.nan
        else:
            self.log_mean_exp[~self.flags] = np.nan


class Waic(object):
    """What ``waic()`` returns: the widely applicable information criterion of a model with pointwise log-likelihoods
    l_i = log p(y_i | x), from a ``PointwiseStatistics`` whose value 0 is l_i without its constants (log-mean-exp on) and
    whose value 1 is the fitted mean, on the first ``n_data`` experts (Gelman, Hwang and Vehtari 2014, sections 3.4-3.5):

      ``lppd_i = log_mean_exp[0][i] + const_i``             log pointwise predictive density
      ``p_waic_i = var[0][i]``                              effective number of parameters (their p_WAIC2) -- the weighted
                                                            POPULATION variance over the S recorded states stands where
                                                            they use the sample variance with S - 1
      ``elpd_i = lppd_i - p_waic_i``
      ``lppd``, ``p_waic``, ``elpd_waic``                   the sums over the rows;  ``waic = -2 elpd_waic``
      ``se = sqrt(n_data * var_i(elpd_i))``                 standard error of elpd_waic over the rows
      ``fitted``                                            posterior-predictive mean of every row (value 1)
      ``n_warn``                                            rows with p_waic_i > 0.4: where WAIC is unreliable (Vehtari,
                                                            Gelman and Gabry 2017)

    and ``pointwise``, the statistics of all experts."""

    def __init__(self, pointwise, n_data, constants, fitted=None):
        n = int(n_data)
        constants = np.broadcast_to(np.asarray(constants, dtype=np.float64), (n,))
        self.pointwise, self.n_data = pointwise, n
        self.lppd_i = pointwise.log_mean_exp[0, :n] + constants
        self.p_waic_i = pointwise.var[0, :n].copy()
        self.elpd_i = self.lppd_i - self.p_waic_i
        self.lppd, self.p_waic, self.elpd_waic = float(self.lppd_i.sum()), float(self.p_waic_i.sum()), float(self.elpd_i.sum())
        self.se = float(np.sqrt(n * np.var(self.elpd_i)))
        self.waic = -2.0 * self.elpd_waic
        self.fitted = pointwise.mean[1, :n].copy() if fitted is None else np.asarray(fitted, dtype=np.float64)
        self.n_warn = int(np.sum(self.p_waic_i > 0.4))


def refuse_grouped(distribution, what, why):
    """ValueError when the distribution's energy is a grouped linear model (device_linear_grouped,
    MultinomialLogisticRegression): the passes that cannot run on one name it."""
    kind, params = distribution.device_energy()
    if kind == _lib.E_LINEAR_EXPR and params.get('groups'):
        raise ValueError('%s: the energy of %s is a grouped linear model (device_linear_grouped, '
                         'MultinomialLogisticRegression: groups of %d experts under a log-sum-exp) -- %s'
                         % (what, type(distribution).__name__, params['groups'][0], why))


def refuse_wide(distribution, what):
    """ValueError when the distribution's energy is a wide linear model (device_linear_wide,
    GeneralizedLinearModel(wide=True)): the passes that take at most 512 dims name it."""
    kind, params = distribution.device_energy()
    if kind == _lib.E_LINEAR_EXPR and params.get('wide'):
        raise ValueError('%s: the energy of %s is a wide linear model (device_linear_wide, '
                         'GeneralizedLinearModel(wide=True): W is %d x %d) -- this pass takes models of at most 512 dims, '
                         'stored in one chunk of dims per block of experts'
                         % ((what, type(distribution).__name__) + tuple(np.shape(params['W']))))


_GROUPED_PER_EXPERT = ('the per-expert passes report in the caller\'s order on terms that each see one u_j; a grouped model '
                       'stores its experts in a permuted order and couples the members of a group (its per-row pass is '
                       'group_pointwise() / group_waic())')


def pointwise_request(distribution, n_iter, values=None, log_mean_exp=None, compile_check=True):
    """The checks ``pointwise()`` makes before anything runs, none of which needs a device: returns
    (values, flags) or raises ValueError -- n_iter < 1, no value or more than 4, an energy that is not a linear model, an
    expression that does not compile (with the compiler's message, mjhmc_pointwise_check)."""
    n_iter = int(n_iter)
    if n_iter < 1:
        raise ValueError('n_iter must be >= 1, got %d' % n_iter)
    kind, params = distribution.device_energy()
    if kind != _lib.E_LINEAR_EXPR:
        names = dict((getattr(_lib, n), n[2:]) for n in dir(_lib) if n.startswith('E_') and isinstance(getattr(_lib, n), int))
        raise ValueError('pointwise: the per-expert statistics are those of a linear-model energy (LINEAR_EXPR: '
                         'device_linear, device_linear_tall, GeneralizedLinearModel); the energy of %s is %s'
                         % (type(distribution).__name__, names.get(kind, kind)))
    refuse_grouped(distribution, 'pointwise', _GROUPED_PER_EXPERT)
    refuse_wide(distribution, 'pointwise')
    if values is None:
        if not hasattr(distribution, 'pointwise_values'):
            raise ValueError('pointwise: %s has no pointwise_values(); pass values=' % type(distribution).__name__)
        if log_mean_exp is not None:
            raise ValueError('log_mean_exp belongs to values=: the distribution\'s own values carry their flags')
        values, log_mean_exp = distribution.pointwise_values()
    values = [values] if isinstance(values, str) else [str(v) for v in values]
    engine.pointwise_args(values, log_mean_exp)
    flags = [False] * len(values) if log_mean_exp is None else [bool(f) for f in np.atleast_1d(log_mean_exp)]
    if compile_check:
        K, D = np.shape(params['W'])
        engine.pointwise_check(D, K, values)
    return values, flags


def group_pointwise_request(distribution, n_iter, values=None, log_mean_exp=None, per=None, compile_check=True):
    """The checks ``group_pointwise()`` makes before anything runs, none of which needs a device: returns
    (values, flags, per) or raises ValueError -- n_iter < 1, no value or more than 4, flags or ``per`` that do not pair with
    the values, a kind other than 'group' / 'member', an energy that is not a linear model or is one without groups, an
    expression that does not compile (with the compiler's message, mjhmc_pointwise_grouped_check)."""
    n_iter = int(n_iter)
    if n_iter < 1:
        raise ValueError('n_iter must be >= 1, got %d' % n_iter)
    kind, params = distribution.device_energy()
    if kind != _lib.E_LINEAR_EXPR:
        names = dict((getattr(_lib, n), n[2:]) for n in dir(_lib) if n.startswith('E_') and isinstance(getattr(_lib, n), int))
        raise ValueError('group_pointwise: the per-group statistics are those of a grouped linear-model energy (LINEAR_EXPR '
                         'with groups: device_linear_grouped, MultinomialLogisticRegression); the energy of %s is %s'
                         % (type(distribution).__name__, names.get(kind, kind)))
    if not params.get('groups'):
        raise ValueError('group_pointwise: the energy of %s is a linear model without groups (device_linear, '
                         'device_linear_tall, GeneralizedLinearModel): its experts are its data rows and pointwise() / '
                         'waic() report on them' % type(distribution).__name__)
    if values is None:
        if not hasattr(distribution, 'group_values'):
            raise ValueError('group_pointwise: %s has no group_values(); pass values=' % type(distribution).__name__)
        if log_mean_exp is not None or per is not None:
            raise ValueError('log_mean_exp and per belong to values=: the distribution\'s own values carry theirs')
        values, log_mean_exp, per = distribution.group_values()
    values = [values] if isinstance(values, str) else [str(v) for v in values]
    engine.group_pointwise_args(values, log_mean_exp, per)
    flags = [False] * len(values) if log_mean_exp is None else [bool(f) for f in np.atleast_1d(log_mean_exp)]
    per = ['group'] * len(values) if per is None else ([per] if isinstance(per, str) else [str(k) for k in per])
    if compile_check:
        K, D = np.shape(params['W'])
        engine.group_pointwise_check(D, K, params['groups'], values, per)
    return values, flags, per


class Influence(object):
    """What ``influence()`` returns: how the experts j0 <= j < j1 of a linear-model energy (its data rows) move the
    coefficients x, from the device sums (include/mjhmc_hip.h: mjhmc_influence_read, _read_cross) ``W`` = sum w,
    ``Sx`` = sum w (x - cx), ``S2x`` = sum w (x - cx)^2, ``St`` = sum w (t - ct), ``S2t`` = sum w (t - ct)^2 and
    ``Cxt`` = sum w x (t - ct)^T of shape (D, J), J = j1 - j0, t_j the value (the pointwise log-likelihood l_j):

      ``mean_x = cx + Sx / W``, ``var_x``           of the coefficients; both variances are weighted POPULATION variances,
      ``mean_t = ct + St / W``, ``var_t``           clipped at 0
      ``cov = Cxt / W - mean_x (St / W)^T``         Cov(x_d, t_j), (D, J)
      ``corr``                                      cov / sqrt(var_x var_t^T); 0 where a variance is 0
      ``loo_shift = -cov``                          to first order E_{-j}[x] - E[x]: what deleting row j does to the
                                                    posterior mean; ``loo_mean(j)`` = mean_x + loo_shift[:, j - j0]
      ``ij_cov(rows=None, center=True)``            sum_j I_j I_j^T, I_j = cov[:, j]: the infinitesimal-jackknife covariance
                                                    of the posterior mean (Giordano and Broderick), valid under
                                                    misspecification; ``center`` takes the I_j about their mean over the rows
      ``distance(precision)``                       I_j^T precision I_j per expert, (J,): a Cook's distance
      ``most_influential(k, precision=None)``       the k experts of largest distance, largest first

    Experts are named by their index in the model throughout (``rows``, ``j``, the result of ``most_influential``).
    ``n_data``: the experts below it are data rows (None: all are); ``rows=None`` means those of them inside [j0, j1)."""

    def __init__(self, W, Sx, S2x, St, S2t, Cxt, n_states, experts, cx, ct, n_data=None):
        self.W, self.Sx, self.S2x, self.St, self.S2t, self.Cxt = float(W), Sx, S2x, St, S2t, Cxt
        self.total_weight, self.n_states = self.W, int(n_states)
        self.experts = (int(experts[0]), int(experts[1]))
        self.cx, self.ct = np.asarray(cx, dtype=np.float64), np.asarray(ct, dtype=np.float64)
        self.n_data = None if n_data is None else int(n_data)
        with np.errstate(divide='ignore', invalid='ignore'):
            mx, mt = Sx / self.W, St / self.W
            self.mean_x, self.mean_t = self.cx + mx, self.ct + mt
            self.var_x = np.maximum(S2x / self.W - mx * mx, 0.0)
            self.var_t = np.maximum(S2t / self.W - mt * mt, 0.0)
            self.cov = Cxt / self.W - np.outer(self.mean_x, mt)
            scale = np.sqrt(np.outer(self.var_x, self.var_t))
            self.corr = np.where(scale > 0, self.cov / np.where(scale > 0, scale, 1.0), 0.0)
        self.loo_shift = -self.cov

    def _columns(self, rows):
        j0, j1 = self.experts
        if rows is None:
            rows = np.arange(j0, j1 if self.n_data is None else max(j0, min(j1, self.n_data)))
        rows = np.atleast_1d(np.asarray(rows, dtype=np.int64))
        if rows.size and (rows.min() < j0 or rows.max() >= j1):
            raise ValueError('rows must be experts in [%d, %d)' % (j0, j1))
        return rows - j0

    def loo_mean(self, j):
        """the first-order posterior mean without expert (data row) j"""
        return self.mean_x + self.loo_shift[:, int(self._columns([j])[0])]

    def ij_cov(self, rows=None, center=True):
        I = self.cov[:, self._columns(rows)]
        if center and I.shape[1]:
            I = I - I.mean(axis=1, keepdims=True)
        return I.dot(I.T)

    def distance(self, precision):
        P = np.asarray(precision, dtype=np.float64)
        if P.shape != (self.cov.shape[0],) * 2:
            raise ValueError('precision must be (%d, %d)' % ((self.cov.shape[0],) * 2))
        return np.einsum('dj,de,ej->j', self.cov, P, self.cov)

    def most_influential(self, k, precision=None):
        """the k experts of largest ``distance``, largest first; ``precision=None`` takes diag(1 / var_x) (dimensions of
        zero variance left out)"""
        if precision is None:
            with np.errstate(divide='ignore'):
                precision = np.diag(np.where(self.var_x > 0, 1.0 / np.where(self.var_x > 0, self.var_x, 1.0), 0.0))
        d = self.distance(precision)
        order = np.argsort(-d, kind='stable')[:max(0, int(k))]
        return order + self.experts[0]


def influence_request(distribution, n_iter, value=None, experts=None, sharded=False, compile_check=True):
    """The checks ``influence()`` makes before anything runs, none of which needs a device: returns (value, (j0, j1)) or
    raises ValueError -- n_iter < 1, an energy that is not a linear model (named), a distribution without
    ``influence_value()`` when no value is given, more than one value, experts that are not a range 0 <= j0 < j1 <= K, a
    sharded sampler, an expression that does not compile (with the compiler's message, mjhmc_influence_check)."""
    n_iter = int(n_iter)
    if n_iter < 1:
        raise ValueError('n_iter must be >= 1, got %d' % n_iter)
    kind, params = distribution.device_energy()
    if kind != _lib.E_LINEAR_EXPR:
        names = dict((getattr(_lib, n), n[2:]) for n in dir(_lib) if n.startswith('E_') and isinstance(getattr(_lib, n), int))
        raise ValueError('influence: the influence of a data row is that of an expert of a linear-model energy (LINEAR_EXPR: '
                         'device_linear, device_linear_tall, GeneralizedLinearModel); the energy of %s is %s'
                         % (type(distribution).__name__, names.get(kind, kind)))
    refuse_grouped(distribution, 'influence', _GROUPED_PER_EXPERT)
    refuse_wide(distribution, 'influence')
    if value is None:
        if not hasattr(distribution, 'influence_value'):
            raise ValueError('influence: %s has no influence_value(); pass value=' % type(distribution).__name__)
        value = distribution.influence_value()
    if not isinstance(value, str):
        value = list(value)
        if len(value) != 1:
            raise ValueError('influence: one value per pass, got %d (more than one value is more than one call)' % len(value))
        value = str(value[0])
    engine.influence_args(value)
    K, D = np.shape(params['W'])
    j0, j1 = (0, K) if experts is None else (int(experts[0]), int(experts[1]))
    if j0 < 0 or j1 > K or j0 >= j1:
        raise ValueError('influence: experts=(%d, %d) is not a range 0 <= j0 < j1 <= K of the model\'s K = %d' % (j0, j1, K))
    if sharded:
        raise ValueError('influence: a sharded sampler (comm set) is not supported -- the sums are additive over ranks, '
                         'but summing them is out of scope here')
    if compile_check:
        engine.influence_check(D, K, value)
    return value, (j0, j1)


class HMCBase(object):
    """Hyper-parameters, counters and plumbing shared by all samplers (markov_jump_hmc.py:16-104)."""

    _mode = _lib.MODE_CONTROL

    def __init__(self, Xinit=None, E=None, dEdX=None, epsilon=1e-4, alpha=0.2, beta=None,
                 num_leapfrog_steps=5, distribution=None, seed=None, dtype=None, device=0, Vinit=None,
                 comm=None):
        self.num_leapfrog_steps = num_leapfrog_steps
        self.epsilon = epsilon
        self.beta = beta or alpha ** (1. / (self.epsilon * self.num_leapfrog_steps))
        self.original_epsilon = epsilon
        self.original_l = self.num_leapfrog_steps
        self.n_burn_in = 500
        self.p_flip = 0.5
        self.p_r = 1
        self.l_count = 0
        self.f_count = 0
        self.fl_count = 0
        self.r_count = 0
        self.grad_per_sample_step = self.num_leapfrog_steps
        self._seed, self._dtype, self._device, self._Vinit = seed, dtype, device, Vinit
        self._comm, self._plan = comm, None      # mjhmc_amd.parallel.Comm: shard particle columns over ranks
        self._pending = np.zeros(6, dtype=np.int64)  # local l, f, r, fl, E, dEdX increments not yet reduced
        self._acc_evals = np.zeros(2, dtype=np.int64)   # E / dEdX evaluations of the iteration in flight (retries included)
        self._iter_evals = []                           # per committed iteration of the CURRENT batch call: (E, dEdX), local
        self._dev = None
        self._in_retry = False
        if not isinstance(self, ContinuousTimeHMC):
            if not isinstance(distribution, Distribution):
                raise NotImplementedError(
                    'The MI355X engine runs energies that have a device functor: pass '
                    'distribution=<mjhmc_amd.misc.distributions.Distribution> (Xinit/E/dEdX callables '
                    'cannot be compiled for the GPU).')
            distribution.mjhmc = False
            distribution.reset()
            self._attach(distribution)

    # -- device plumbing -------------------------------------------------------------------
    def _attach(self, distribution):
        self.ndims = distribution.Xinit.shape[0]
        self.nbatch = distribution.Xinit.shape[1]
        self.energy_func = distribution.E
        self.grad_func = distribution.dEdX
        self.distribution = distribution
        seed = self._seed
        if seed is None:
            lo, hi = np.random.randint(0, 2 ** 32, size=2, dtype=np.uint64)
            seed = int(lo) | (int(hi) << 32)
            if self._comm is not None:                      # every rank must use rank 0's seed
                seed = int(self._comm.allreduce_ints([seed >> 1 if self._comm.rank == 0 else 0], 'sum')[0]) << 1
        self.seed = int(seed)
        X0, V0, first = distribution.Xinit, self._Vinit, 0
        if self._comm is not None:
            from ..parallel import ShardPlan
            self._plan = ShardPlan(self.nbatch, self._comm.world)
            first, stop = self._plan.span(self._comm.rank)
            X0 = X0[:, first:stop]
            V0 = None if V0 is None else V0[:, first:stop]
        self._dev = engine.make_sampler(distribution.bind(self._device), np.ascontiguousarray(X0), Vinit=V0,
                                        seed=self.seed, first_particle_id=first,
                                        dtype=self._dtype or getattr(distribution, 'state_dtype', 'float64'),
                                        mode=self._mode)
        self._dev.set_timing(False)     # (nothing here reads the device-side timing: two marker packets less per call)
        # HMCState.__init__ evaluates E and dEdX once on every particle (hmc_state.py:28-39)
        distribution.E_count += self.nbatch
        distribution.dEdX_count += self.nbatch

    def _push_hparams(self):
        self._dev.set_hparams(self.epsilon, self.num_leapfrog_steps, self.p_r, self.beta, self.p_flip)

    @property
    def state(self):
        return DeviceHMCState(self)

    @state.setter
    def state(self, Z):
        """Assigning an HMCState uploads its X (and V) (figures/poe_fig.py:59); with sharded columns every rank
        uploads its own block."""
        cols = slice(None) if self._plan is None else slice(*self._plan.span(self._comm.rank))
        self._dev.write(_lib.F_X, np.ascontiguousarray(Z.X[:, cols]))
        if getattr(Z, 'V', None) is not None:
            self._dev.write(_lib.F_V, np.ascontiguousarray(Z.V[:, cols]))

    # -- checkpoint / resume -----------------------------------------------------------------
    _SAVED = ('epsilon', 'num_leapfrog_steps', 'beta', 'p_r', 'p_flip', 'original_epsilon', 'original_l',
              'l_count', 'f_count', 'fl_count', 'r_count')

    def save_state(self, path):
        """Everything a run needs to continue exactly where it stands -- X, V, the inverse-L cache (H_flf, NaN =
        cold), the counter-RNG position, hyper-parameters and counters -- as an ``.npz`` file.  A sampler built on
        the same distribution and ``load_state``-ed continues bit for bit (the RNG is a pure function of
        (seed, particle id, tick))."""
        st = self.state
        meta = {k: np.asarray(getattr(self, k)) for k in self._SAVED}
        np.savez(path, X=st.X, V=st.V, H_flf=st.H_flf[0], dwelling_times=np.asarray(getattr(self, 'dwelling_times', 0.0)),
                 tick=np.uint64(self._dev.get_tick()), seed=np.uint64(self.seed),
                 E_count=self.distribution.E_count, dEdX_count=self.distribution.dEdX_count, **meta)

    def load_state(self, path):
        z = np.load(path if str(path).endswith('.npz') else str(path) + '.npz')
        if z['X'].shape != (self.ndims, self.nbatch):
            raise ValueError('checkpoint holds a %r state, this sampler is %r' % (z['X'].shape, (self.ndims, self.nbatch)))
        if int(z['seed']) != self.seed:
            raise ValueError('checkpoint was written with seed %d, this sampler has %d' % (int(z['seed']), self.seed))
        cols = slice(None) if self._plan is None else slice(*self._plan.span(self._comm.rank))
        self._dev.write(_lib.F_X, np.ascontiguousarray(z['X'][:, cols]))      # re-derives EX (and dE/dX), clears the cache
        self._dev.write(_lib.F_V, np.ascontiguousarray(z['V'][:, cols]))
        self._dev.write(_lib.F_HFLF, np.ascontiguousarray(z['H_flf'][cols]))
        self._dev.set_tick(int(z['tick']))
        for k in self._SAVED:
            setattr(self, k, z[k].item())
        self.distribution.E_count, self.distribution.dEdX_count = int(z['E_count']), int(z['dEdX_count'])
        if hasattr(self, 'dwelling_times'):
            self.dwelling_times = z['dwelling_times']
        return self

    def E(self, X):
        return self.energy_func(X).reshape((1, -1))

    def dEdX(self, X):
        return self.grad_func(X)

    def leap_prob(self, Z1, Z2):
        """Metropolis-Hastings probability of transitioning from state Z1 to state Z2 (markov_jump_hmc.py:106-114)."""
        Ediff = Z1.H() - Z2.H()
        p_acc = np.ones((1, Ediff.shape[1]))
        p_acc[Ediff < 0] = np.exp(Ediff[Ediff < 0])
        return p_acc

    def burn_in(self):
        self._run(self.n_burn_in)
        self._publish()

    def _account(self, st):
        self._pending[4] += st.E_evals
        self._pending[5] += st.dEdX_evals
        self._acc_evals += (st.E_evals, st.dEdX_evals)

    def _commit(self, st):
        self._pending[:4] += (st.l, st.f, st.r, st.fl)
        self._iter_evals.append(self._acc_evals.copy())
        self._acc_evals[:] = 0

    def eval_trace(self, n_last):
        """(E_evals, dEdX_evals) per iteration for the last ``n_last`` committed iterations of the most recent
        batch call (sample / _record / burn_in), summed over ranks: the increments of Distribution.E_count /
        dEdX_count a per-step host loop would observe (mjhmc/misc/autocor.py:246-248)."""
        tr = np.array(self._iter_evals[-n_last:], dtype=np.int64).reshape(-1, 2)
        if self._comm is not None:
            tr = self._comm.allreduce_ints(tr.ravel(), 'sum').reshape(-1, 2)
        return tr

    def _publish(self):
        """Fold this call's integer bookkeeping into the public counters (summed over ranks)."""
        inc = self._pending if self._comm is None else self._comm.allreduce_ints(self._pending, 'sum')
        self.l_count += int(inc[0])
        self.f_count += int(inc[1])
        self.r_count += int(inc[2])
        self.fl_count += int(inc[3])
        self.distribution.E_count += int(inc[4])
        self.distribution.dEdX_count += int(inc[5])
        self._pending[:] = 0

    # -- iteration driver (discrete-time samplers; the jump processes override _one) -----------
    def _one(self, ring_slot=-1, replay=None):
        self._push_hparams()
        rn = ru = None
        if replay is not None:
            rn, ru = replay.pop(0)
        stats, n_done = self._dev.iterate(1, replay_normal=rn, replay_unif=ru, ring_slot0=ring_slot)
        self._account(stats[0])
        self._commit(stats[0])

    def _run(self, n_iter, ring_slot0=-1, replay=None, download=None, keep_trace=False):
        """n_iter iterations launched back to back; the host only steps in on a non-finite rate.  ``download = (out, k0)``:
        ring slot ring_slot0 + i also goes to out[:, (k0 + i) * N : ...] while the following iterations run
        (mjhmc_iterate_download).  ``keep_trace``: this call continues a batch call that walks the device ring in chunks --
        eval_trace() describes the whole batch call, not its last chunk."""
        if not self._in_retry and not keep_trace:
            self._iter_evals = []                         # the trace describes one batch call, it does not grow for ever
        if replay is not None:                            # recorded random numbers: one attempt at a time
            for i in range(n_iter):
                self._one(ring_slot0 + i if ring_slot0 >= 0 else -1, replay)
            return
        # only the jump processes can meet a non-finite rate; the discrete-time samplers never roll back
        sync = self._comm is not None and self._mode != _lib.MODE_CONTROL
        done = 0
        while done < n_iter:
            self._push_hparams()
            slot = ring_slot0 + done if ring_slot0 >= 0 else -1
            todo = n_iter - done
            if sync and todo > 1:
                self._dev.checkpoint()                    # once per batch; a single iteration needs none (rollback)
            if download is not None:
                stats, n_done = self._dev.iterate_download(todo, slot, download[0], download[1] + done)
            else:
                stats, n_done = self._dev.iterate(todo, ring_slot0=slot)
            if sync:
                # the reference aborts the WHOLE batch on one bad particle: every rank keeps only the
                # iterations all ranks committed; a rank that ran ahead rolls back + replays (bit-identical:
                # the RNG is a pure function of (seed, particle id, tick))
                from ..parallel import agree_on_progress
                common = agree_on_progress(self._comm, n_done)
                if common < n_done:
                    if todo == 1:
                        self._dev.rollback()              # ping-pong inputs are intact; the tick stays consumed
                    else:
                        self._dev.restore()
                        if common:
                            redo, again = self._dev.iterate(common, ring_slot0=slot)
                            assert again == common
                        self._dev.advance_tick(1)         # the failed attempt's tick, consumed everywhere
                failed_somewhere = common < todo
                n_done = common
            else:
                failed_somewhere = len(stats) > n_done
            for st in stats[:n_done]:
                self._account(st)
                self._commit(st)
            done += n_done
            if failed_somewhere:                          # the attempt after the committed ones failed
                self._account(stats[n_done])
                self._retry(ring_slot0 + done if ring_slot0 >= 0 else -1, None)
                if download is not None:                  # the retried iteration's slot, plainly
                    N = self._dev.nparticles
                    k = download[1] + done
                    download[0][:, k * N:(k + 1) * N] = self._dev.ring_read(ring_slot0 + done, 1)
                done += 1

    def _retry(self, ring_slot, replay):
        raise ValueError('Infinite rate.')                # only the jump processes can get here

    def sampling_iteration(self, replay=None):
        """One step of every particle (markov_jump_hmc.py:116-148).  ``replay=[(normals (D,N),
        uniforms (2N+1) = accept, flip, R gate), ...]`` feeds recorded random numbers."""
        self._step(replay)
        self._publish()

    def _step(self, replay):
        if self._comm is not None:
            self._run(1)
        else:
            self._iter_evals = []
            self._one(-1, replay)

    # Sharded runs (extension): ``sampler.gather_root = r`` makes sample() with resample=False return the gathered block on
    # rank r only -- the other ranks take part in the collective, skip the re-tile and the download of a block they do not
    # want (mjhmc_comm_allgather_ring with host_out = NULL) and get None.  Default None: every rank gets the block, as a
    # single-process caller of the reference does.
    gather_root = None

    def _stack(self, n_samples, preserve_order, out=None):
        if self._comm is not None and self._comm.on_device:
            # the one data-path collective: device rings all-gathered over RCCL, re-tiled on the receiving GPU
            res = self._comm.allgather_ring(self._dev, 0, n_samples, bool(preserve_order), self._plan.counts, root=self.gather_root)
        else:
            local = self._dev.ring_read(0, n_samples, stacked=bool(preserve_order), out=out if self._comm is None else None)
            if self._comm is None:
                return local
            from ..parallel import assemble_stacked
            res = assemble_stacked(self._comm, self._plan, local, n_samples, bool(preserve_order))
            if self.gather_root is not None and int(self.gather_root) != self._comm.rank:
                res = None
        if res is None:
            return None
        if out is None:
            return res
        if out.shape != res.shape or out.dtype != np.float64:      # sharded run: the gathered block lands in the caller's array
            raise ValueError('out must be a float64 array of shape %r' % (res.shape,))
        out[...] = res
        return out

    def sample(self, n_samples=1000, preserve_order=False, replay=None, out=None):
        """markov_jump_hmc.py:150-173.  ``out`` (extension): a preallocated C-contiguous float64 array of the result's
        shape, (ndims, n_samples * nbatch) or (ndims, nbatch, n_samples), filled and returned instead of a fresh one."""
        if self._streams(preserve_order, replay):
            return self._sample_streamed(n_samples, out)
        self._record(n_samples, replay)
        return self._stack(n_samples, preserve_order, out)

    def _streams(self, preserve_order, replay):
        """np.concatenate(samples, axis=1) of an unsharded run with the counter RNG: every sample goes to the host while the
        next iterations run, and the device ring may be smaller than the run"""
        return self._comm is None and replay is None and not preserve_order and hasattr(self._dev, 'iterate_download')

    def _host_array(self, n_states, what, out=None):
        shape = (self.ndims, n_states * self.nbatch)
        if out is not None:
            if out.shape != shape or out.dtype != np.float64 or not out.flags.c_contiguous:
                raise ValueError('out must be a C-contiguous float64 array of shape %r' % (shape,))
            return out
        try:
            return np.empty(shape)
        except MemoryError:
            raise MemoryError('%s: %d states of %d x %d float64 are %.1f GB of host memory, which this machine does not give -- '
                              'draw fewer samples per call, or thin them' % (what, n_states, self.ndims, self.nbatch,
                                                                             8e-9 * self.ndims * self.nbatch * n_states))

    def _sample_streamed(self, n_iter, out=None, what='sample()'):
        """n_iter iterations, the state after each as columns [k N, (k + 1) N) of the returned (ndims, n_iter * nbatch) array.
        The device ring holds as many slots as fit (all of them if it can): a run bigger than the device walks it in
        chunks."""
        out = self._host_array(n_iter, what, out)
        slots = max(2, self._dev.ring_budget_slots(n_iter))
        self._dev.ring_alloc(slots)
        done = 0
        while done < n_iter:
            chunk = min(slots, n_iter - done)
            self._run(chunk, ring_slot0=0, download=(out, done), keep_trace=done > 0)
            done += chunk
        self._publish()
        return out

    # the jump processes weight every state by its holding time (ContinuousTimeHMC); a discrete-time chain's states count once
    _dwell_weighted = False

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
        if self.distribution.device_energy()[0] == _lib.E_HOST:
            raise ValueError('energy_observables: the energy is a pair of opaque Python callables, which are its only '
                             'evaluation -- there is no device evaluation of E and dE/dX to record (sample(preserve_order=True) '
                             'and the callables give them on the host)')
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
        n_iter, every = int(n_iter), int(every)
        if n_iter < 1:
            raise ValueError('n_iter must be >= 1, got %d' % n_iter)
        if every < 1:
            raise ValueError('every must be >= 1, got %d' % every)
        particles = min(int(self.nbatch), 8192) if particles is None else int(particles)
        if particles < 1 or particles > int(self.nbatch):
            raise ValueError('particles must be in [1, nbatch = %d], got %d' % (int(self.nbatch), particles))
        c = float(np.sqrt(self.ndims)) if c is None else float(c)
        if not np.isfinite(c) or c <= 0:
            raise ValueError('the kernel scale c must be finite and > 0, got %r' % c)
        if self.distribution.device_energy()[0] == _lib.E_HOST:
            raise ValueError('stein_discrepancy: the energy is a pair of opaque Python callables, which are its only '
                             'evaluation -- there is no device evaluation of dE/dX to form the Stein kernel from')
        if self._comm is not None:
            raise ValueError('stein_discrepancy: a sharded sampler (comm set) is not supported -- pairs of particles '
                             'across ranks are not formed')
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
        n_iter = int(n_iter)
        if n_iter < 1:
            raise ValueError('n_iter must be >= 1, got %d' % n_iter)
        if of is not None and shift is not None and np.size(shift) != of.n_values:
            raise ValueError('shift must have n_values = %d entries' % of.n_values)
        self._check_of(of)
        with self._RecordedRun(self, [n_iter], block, of) as run:
            est = run.own(run.src.estimator(cov))
            if shift is not None:
                shift = self._checked_shift(shift, of)
                est.set_shift(shift)
            def accumulate(k):
                if isinstance(of, EnergyObservables):
                    # slot by slot, as the block was evaluated: the moment pass adds a call's sum to its running totals, so
                    # one call per slot makes W, S1 and S2 independent of how the run is cut into blocks, bit for bit
                    for j in range(k):
                        est.accumulate(j, 1, w_slot0=1 + j if run.lead else -1)
                else:
                    est.accumulate(0, k, w_slot0=run.w_slot0)

            for _, k in run.blocks():
                accumulate(k)
                if shift is None:                          # the first block's own mean, then the same block again about it
                    W, S1 = self._reduce_sums(est.read())[:2]
                    shift = S1 / W
                    est.reset()
                    est.set_shift(shift)
                    accumulate(k)
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
        n_iter = int(n_iter)
        if n_iter < 1:
            raise ValueError('n_iter must be >= 1, got %d' % n_iter)
        K = int(self.ndims) if of is None else int(of.n_values)
        refuse_wide(self.distribution, 'cv_expectations')
        if int(self.ndims) > 512 or K > 512:
            raise ValueError('cv_expectations takes ndims <= 512 and K <= 512 values, got ndims = %d, K = %d' % (self.ndims, K))
        if n_iter * int(self.nbatch) <= 2 * int(self.ndims):
            raise ValueError('cv_expectations: n_iter * nbatch = %d states do not determine a regression on ndims = %d '
                             'control variates (more than 2 * ndims are needed)' % (n_iter * int(self.nbatch), self.ndims))
        if shift is not None and np.size(shift) != K:
            raise ValueError('shift must have %d entries' % K)
        self._check_of(of)
        refuse_grouped(self.distribution, 'cv_expectations',
                       'its sampler runs the multi-pass path with either state dtype, which has no single-launch '
                       'evaluation of dE/dX to take the control variates from')
        if self.distribution.device_energy()[0] == _lib.E_HOST:
            raise ValueError('cv_expectations: the energy is a pair of opaque Python callables, which are its only '
                             'evaluation -- there is no device evaluation of dE/dX to take the control variates from')
        if self._comm is not None:
            raise ValueError('cv_expectations: a sharded sampler (comm set) is not supported -- the sums are additive over '
                             'ranks, but that is out of scope: it has not been proved on a multi-rank machine')
        # the handle's dE/dX matrix is at most two slots (float32 gradient of a bfloat16 state); the partials of the
        # covariance and cross passes are at most ~2048 waves x 32 KiB each
        reserve = lambda: 2 * self._dev.ring_slot_bytes() + (160 << 20)
        with self._RecordedRun(self, [n_iter], block, of, reserve_bytes=reserve) as run:
            cm = run.own(run.src.cross_moments())
            if shift is not None:
                shift = self._checked_shift(shift, of)
                cm.set_shift(shift)
            for _, k in run.blocks():
                cm.accumulate(0, k, w_slot0=run.w_slot0)
                if shift is None:                          # the first block's own mean, then the same block again about it
                    sums = cm.read()
                    shift = sums[3] / sums[0]
                    cm.reset()
                    cm.set_shift(shift)
                    cm.accumulate(0, k, w_slot0=run.w_slot0)
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
        if self._comm is not None:
            raise ValueError('pointwise: a sharded sampler (comm set) is not supported -- the sums are additive over ranks, '
                             'but summing them is out of scope here')
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
        if self._comm is not None:
            raise ValueError('group_pointwise: a sharded sampler (comm set) is not supported -- the sums are additive over '
                             'ranks, but summing them is out of scope here')
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

    def _checked_shift(self, shift, of=None):
        shift = np.ascontiguousarray(np.asarray(shift, dtype=np.float64).reshape(-1))
        if of is not None:
            if shift.shape != (of.n_values,):
                raise ValueError('shift must have n_values = %d entries' % of.n_values)
        elif shift.shape != (self.ndims,):
            raise ValueError('shift must have ndims = %d entries' % self.ndims)
        if self._comm is not None:
            shift = self._comm.bcast(shift.copy(), 0)
        return shift

    def _ring_blocks(self, segments, block):
        """The block walk of expectations() and diagnostics(): runs sum(segments) states of every particle through the
        ring, at most ``block`` at a time and never across a segment boundary, and yields ``(segment, k)`` when the next k
        states sit in ring slots 0 .. k - 1 -- for the jump samplers with their holding times in dwell slots 1 .. k (the
        run's first block runs k + 1 iterations; every later one starts from a copy of the last state in the lead slot)."""
        lead = 1 if self._dwell_weighted else 0
        done = last = 0
        for seg, length in enumerate(segments):
            seg_done = 0
            while seg_done < length:
                k = min(block, length - seg_done)
                if not lead:
                    self._run(k, ring_slot0=0, keep_trace=done > 0)
                elif done == 0:
                    self._run(k + 1, ring_slot0=0)         # states in slots 0 .. k, their holding times in 1 .. k (+ the next block's)
                else:
                    self._dev.ring_copy(last, 0)           # the state whose holding time the first iteration of this block draws
                    self._run(k, ring_slot0=1, keep_trace=True)
                yield seg, k
                last, done, seg_done = k, done + k, seg_done + k

    class _RecordedRun(object):
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
            for seg, k in self.sampler._ring_blocks(self.segments, self.block):
                if self.fn is not None:
                    self.fn.evaluate(0, k, 0)
                yield seg, k

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
        if not split and n_iter < 2:
            raise ValueError('n_iter must be >= 2, got %d' % n_iter)
        if of is not None:
            if shift is not None and np.size(shift) != of.n_values:
                raise ValueError('shift must have n_values = %d entries' % of.n_values)
        elif shift is not None and np.size(shift) != self.ndims:
            raise ValueError('shift must have ndims = %d entries' % self.ndims)
        self._check_of(of)
        segments = [n_iter // 2, n_iter // 2] if split else [n_iter]
        grad0 = self.distribution.dEdX_count
        # (the per-chain sums have the ring's row layout and take memory: they exist before the budget is taken)
        with self._RecordedRun(self, segments, block, of,
                               early=lambda run: run.own(run.src.chain_stats(len(segments)))) as run:
            cs = run.head
            if shift is not None:
                shift = self._checked_shift(shift, of)
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
        n_iter, bins = int(n_iter), int(bins)
        if n_iter < 1:
            raise ValueError('n_iter must be >= 1, got %d' % n_iter)
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
                            q = 2.0 ** (np.floor(np.log2(W / n_first)) - 24)
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
        n_iter, bins = int(n_iter), int(bins)
        K = self.ndims if of is None else of.n_values
        if n_iter < 1:
            raise ValueError('n_iter must be >= 1, got %d' % n_iter)
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
        if self._comm is not None:
            raise ValueError('occupancy: a sharded sampler (comm set) is not supported -- the tables are additive over ranks, '
                             'but summing them is out of scope here')
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
                        q = 2.0 ** (np.floor(np.log2(W / n_first)) - 24)
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
        n_iter = int(n_iter)
        if n_iter < 1:
            raise ValueError('n_iter must be >= 1, got %d' % n_iter)
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

    def _record(self, n_samples, replay=None):
        """Run n_samples iterations, snapshotting X after each into device ring slots [0, n_samples)."""
        self._dev.ring_alloc(n_samples)
        self._run(n_samples, ring_slot0=0, replay=replay)
        self._publish()


class HMC(HMCBase):
    def __init__(self, *args, **kwargs):
        super(HMC, self).__init__(*args, **kwargs)
        self.p_flip = 1


class ControlHMC(HMCBase):
    def __init__(self, *args, **kwargs):
        super(ControlHMC, self).__init__(*args, **kwargs)
        self.p_flip = 1
        self.p_r = - np.log(1 - self.beta) * 0.5
        self.beta = 1


class ContinuousTimeHMC(HMCBase):
    """Base of the jump-process samplers (markov_jump_hmc.py:203-347)."""

    _mode = _lib.MODE_CTHMC

    def __init__(self, *args, **kwargs):
        self.resample = kwargs.pop('resample', True)
        distribution = kwargs.get('distribution')
        super(ContinuousTimeHMC, self).__init__(*args, **kwargs)
        if not (0 <= self.beta < 1):
            # the reference would recurse forever: p_r = -log(1-beta)/2 is inf/nan and every
            # attempt raises in draw_from (markov_jump_hmc.py:221, 376-385)
            raise ValueError('beta must satisfy 0 <= beta < 1, got %r' % (self.beta,))
        self.p_r = - np.log(1 - self.beta) * 0.5
        self.beta = 1
        if isinstance(distribution, Distribution):
            distribution.mjhmc = True
            if not distribution.generation_instance:
                distribution.reset()
            self._attach(distribution)
        else:
            raise NotImplementedError(
                'Unfortunately, you must define your distribution by subclassing '
                'mjhmc_amd.misc.distributions.Distribution (same rule as the reference, '
                'markov_jump_hmc.py:235-242).')
        self.dwelling_times = np.zeros(self.nbatch)

    _dwell_weighted = True     # expectations(): time averages of the jump process, not of its embedded chain

    def transition_rates(self, Z1, Z2):
        Ediff = Z1.H() - Z2.H()
        return np.exp(Ediff) ** .5

    # -- iteration driver --------------------------------------------------------------------
    def _retry(self, ring_slot, replay):
        """ContinuousTimeHMC lets draw_from's ValueError propagate (markov_jump_hmc.py:266-268)."""
        raise ValueError("Infinite rate. This occurs when calculating transition rates between states that "
                         "have a very large energy difference (mjhmc/misc/utils.py:43-48).")

    def _one(self, ring_slot=-1, replay=None):
        """One sampling_iteration including the reference's retry recursion."""
        self._push_hparams()
        rn = re = None
        if replay is not None:
            rn, re = replay.pop(0)
        stats, n_done = self._dev.iterate(1, replay_normal=rn, replay_exp=re, ring_slot0=ring_slot)
        self._account(stats[0])
        if n_done == 1:
            self._commit(stats[0])
        else:
            self._retry(ring_slot, replay)

    def _read_dwell(self):
        d = self._dev.read(_lib.F_DWELL)
        if self._comm is not None:
            from ..parallel import gather_vector
            d = gather_vector(self._comm, self._plan, d)
        self.dwelling_times = d

    def sampling_iteration(self, replay=None):
        """One jump of every particle.  ``replay=[(normals (D,N), unit_exps (3,N)), ...]`` feeds
        recorded random numbers (one pair per attempt) instead of the counter RNG."""
        self._step(replay)
        self._publish()
        self._read_dwell()

    def burn_in(self):
        super(ContinuousTimeHMC, self).burn_in()
        self._read_dwell()

    def sample(self, n_samples=1000, preserve_order=False, num_steps=None, replay=None, out=None):
        """markov_jump_hmc.py:293-338.  ``num_steps`` is accepted as an alias of ``n_samples``
        (the README calls ``sample(num_steps=10)``, README.md:36).  ``out`` (extension, ``resample=False`` only): a
        preallocated array to fill, see HMCBase.sample."""
        if num_steps is not None:
            n_samples = num_steps
        if self.resample:
            # (this path records into the ring and gathers columns from it: no staging copy per slot is charged)
            if self._streams(False, replay) and self._dev.ring_budget_slots(n_samples + 1, staging=False) < n_samples + 1:
                return self._resample_on_host(n_samples)
            self._dev.ring_alloc(n_samples + 1)
            self._run(n_samples + 1, ring_slot0=0, replay=replay)
            self._publish()
            self._read_dwell()
            if self._comm is not None:
                from ..parallel import assemble_resample
                out, self._last_resample_idx = assemble_resample(
                    self._comm, self._plan, n_samples, self._dev.ring_read_dwell(0, n_samples), self._dev.ring_gather,
                    dev=self._dev)
                return out
            dwell_t = self._dev.ring_read_dwell(0, n_samples).reshape(-1)   # time-major, as np.concatenate
            total_t = np.sum(dwell_t)
            cumul_t = np.cumsum(dwell_t)
            rand_vals = np.sort(np.random.random(n_samples * self.nbatch)) * total_t
            # first index with cumul_t > r, for every r at once (the reference loops, :326-328)
            sample_idx = np.searchsorted(cumul_t, rand_vals, side='right')
            if sample_idx.size and sample_idx[-1] >= dwell_t.size:
                raise IndexError('index 0 is out of bounds for axis 0 with size 0')   # infinite dwell time
            self._last_resample_idx = sample_idx
            return self._dev.ring_gather(sample_idx)
        if self._streams(preserve_order, replay):
            res = self._sample_streamed(n_samples, out)
            self._read_dwell()
            return res
        self._record(n_samples, replay)
        return self._stack(n_samples, preserve_order, out)

    def _resample_on_host(self, n_samples):
        """sample() with dwell-time resampling when the n_samples + 1 states do not fit the device: they are streamed to
        the host through a ring of the slots that do fit, and the columns are picked there (same uniforms, same indices)."""
        n_iter = n_samples + 1
        states = self._host_array(n_iter, 'sample(n_samples=%d, resample=True)' % n_samples)
        slots = max(2, self._dev.ring_budget_slots(n_iter))
        self._dev.ring_alloc(slots)
        dwell, done = [], 0
        while done < n_iter:
            chunk = min(slots, n_iter - done)
            self._run(chunk, ring_slot0=0, download=(states, done), keep_trace=done > 0)
            dwell.append(self._dev.ring_read_dwell(0, chunk))
            done += chunk
        self._publish()
        self._read_dwell()
        dwell_t = np.concatenate(dwell)[:n_samples].reshape(-1)
        cumul_t = np.cumsum(dwell_t)
        rand_vals = np.sort(np.random.random(n_samples * self.nbatch)) * np.sum(dwell_t)
        sample_idx = np.searchsorted(cumul_t, rand_vals, side='right')
        if sample_idx.size and sample_idx[-1] >= dwell_t.size:
            raise IndexError('index 0 is out of bounds for axis 0 with size 0')   # infinite dwell time
        self._last_resample_idx = sample_idx
        return states[:, sample_idx]

    def _record(self, n_samples, replay=None):
        super(ContinuousTimeHMC, self)._record(n_samples, replay)
        self._read_dwell()


class MarkovJumpHMC(ContinuousTimeHMC):
    """Markov Jump HMC, arXiv:1509.03808 (markov_jump_hmc.py:350-415)."""

    _mode = _lib.MODE_MJHMC

    def _retry(self, ring_slot, replay):
        """markov_jump_hmc.py:376-389: halve epsilon, double L, wipe the FLF cache, try again, restore."""
        self.epsilon *= 0.5
        self.num_leapfrog_steps *= 2
        depth = np.log(self.original_epsilon / self.epsilon) / np.log(2)
        print("Ecountered infinite rate, doubling back. Depth: {}".format(depth))
        if depth > MAX_RETRY_DEPTH:
            raise RuntimeError('non-finite transition rates persist after %d halvings' % MAX_RETRY_DEPTH)
        self._dev.reset_flf_cache()
        nested, self._in_retry = self._in_retry, True
        try:
            if self._comm is not None:
                self._run(1, ring_slot)
            else:
                self._one(ring_slot, replay)
        finally:
            self._in_retry = nested
        self.epsilon *= 2
        self.num_leapfrog_steps = int(self.num_leapfrog_steps / 2)
