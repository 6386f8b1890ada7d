"""What a statistics method is asked for, and what it refuses before anything runs.

Belongs here: the ``of=`` descriptions (``Functionals``, ``Projections``, ``EnergyObservables``), every refusal that more
than one method makes, each worded once, and the ``*_request`` checks of the linear-model statistics.  None of it needs a
device or a sampler: a distribution, a communicator or a number is passed in.  Does not belong here: what a method
returns (results.py) and anything that runs (recorded.py).
"""
from __future__ import print_function

import numpy as np

from .. import _lib
from .. import engine


def checked_n_iter(n_iter, least=1):
    """``int(n_iter)``; ValueError below ``least``"""
    n_iter = int(n_iter)
    if n_iter < least:
        raise ValueError('n_iter must be >= %d, got %d' % (least, n_iter))
    return n_iter


def require_linear(distribution, what, sentence):
    """The parameters of the distribution's linear-model energy; ValueError, naming the energy it has, for any other."""
    kind, params = distribution.device_energy()
    if kind != _lib.E_LINEAR_EXPR:
        names = dict((getattr(_lib, n), n[2:]) for n in dir(_lib) if n.startswith('E_') and isinstance(getattr(_lib, n), int))
        raise ValueError('%s: %s; the energy of %s is %s' % (what, sentence, type(distribution).__name__, names.get(kind, kind)))
    return params


def refuse_host_energy(distribution, what, tail):
    """ValueError when the energy is given as opaque callables (E_HOST): ``tail`` says what the device cannot evaluate."""
    if distribution.device_energy()[0] == _lib.E_HOST:
        raise ValueError('%s: the energy is a pair of opaque Python callables, which are its only evaluation -- there is '
                         'no device evaluation of %s' % (what, tail))


_SUMS_NOT_REDUCED = 'the sums are additive over ranks, but summing them is out of scope here'


def refuse_sharded(comm, what, why):
    """ValueError for a sharded sampler: ``comm`` is its communicator (or True), None (or False) for an unsharded one."""
    if comm is not None and comm is not False:
        raise ValueError('%s: a sharded sampler (comm set) is not supported -- %s' % (what, why))


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

    slot_bytes = Functionals.slot_bytes

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
    checked_n_iter(n_iter)
    params = require_linear(distribution, 'pointwise', 'the per-expert statistics are those of a linear-model energy '
                            '(LINEAR_EXPR: device_linear, device_linear_tall, GeneralizedLinearModel)')
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
    checked_n_iter(n_iter)
    params = require_linear(distribution, 'group_pointwise', 'the per-group statistics are those of a grouped linear-model '
                            'energy (LINEAR_EXPR with groups: device_linear_grouped, MultinomialLogisticRegression)')
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


def influence_request(distribution, n_iter, value=None, experts=None, sharded=False, compile_check=True):
    """The checks ``influence()`` makes before anything runs, none of which needs a device: returns (value, (j0, j1)) or
    raises ValueError -- n_iter < 1, an energy that is not a linear model (named), a distribution without
    ``influence_value()`` when no value is given, more than one value, experts that are not a range 0 <= j0 < j1 <= K, a
    sharded sampler, an expression that does not compile (with the compiler's message, mjhmc_influence_check)."""
    checked_n_iter(n_iter)
    params = require_linear(distribution, 'influence', 'the influence of a data row is that of an expert of a linear-model '
                            'energy (LINEAR_EXPR: device_linear, device_linear_tall, GeneralizedLinearModel)')
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
    refuse_sharded(bool(sharded), 'influence', _SUMS_NOT_REDUCED)
    if compile_check:
        engine.influence_check(D, K, value)
    return value, (j0, j1)
