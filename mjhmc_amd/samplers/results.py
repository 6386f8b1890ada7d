"""What the statistics methods of the samplers return: NumPy on the sums and tables a device handle has read.

Belongs here: a class that turns numbers already on the host into moments, quantiles, rates or criteria.  Does not belong
here: anything that needs the library, a device or a sampler -- this module imports numpy and the standard library only
(``Paths`` keeps the device grid it is given and takes ``misc.autocor``'s window rule when ``iat()`` is called).
"""
from __future__ import print_function

import numpy as np


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
