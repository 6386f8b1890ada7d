"""Energy-model interface of the drop-in (mirrors mjhmc/misc/distributions.py and the energy
formulas of mjhmc/misc/tf_distributions.py).

A ``Distribution`` here is a *description*: ``device_energy()`` names the HIP functor and its
parameters; evaluation (``E`` / ``dEdX``) and sampling run on the MI355X.  What is kept from the
reference: the constructor signatures, ``E/dEdX`` counting facades (distributions.py:62-75),
``Xinit/ndims/nbatch/mjhmc/generation_instance/backend/max_n_particles``, ``reset()``,
``__call__`` (NUTS convention, :172-180) and the per-class ``gen_init_X`` recipes.

Out of scope: the 1e6-step "fair initialisation" pickle cache behind
the reference's ``init_X`` (:96-149).  ``init_X`` here uses ``gen_init_X`` directly; pass your
own fair ``Xinit`` through ``LambdaDistribution(init=...)`` or by overriding ``init_X``.
"""
import numpy as np

from .. import _lib
from .. import engine


class Distribution(object):
    """Interface class; subclass it and provide ``device_energy`` (distributions.py:13-59)."""

    def __init__(self, ndims=2, nbatch=100):
        self.ndims = ndims
        self.nbatch = nbatch
        if not hasattr(self, 'backend'):
            self.backend = 'hip'
        self.mjhmc = None
        self.E_count = 0
        self.dEdX_count = 0
        self.generation_instance = False
        if not hasattr(self, 'state_dtype'):
            self.state_dtype = 'float64'         # arithmetic type of state and force on the device
        if not hasattr(self, 'max_n_particles'):
            self.max_n_particles = None
        self._dev = None
        self.init_X()

    # -- device binding -------------------------------------------------------------------
    def device_energy(self):
        """Return (kind, float64 parameter vector) of the HIP functor for this energy."""
        raise NotImplementedError('%s has no device functor: implement device_energy()' % type(self).__name__)

    def bind(self, device=0):
        """DeviceEnergy for this distribution on ``device`` (cached)."""
        if self._dev is None or self._dev.ctx.device != device:
            kind, params = self.device_energy()
            if kind == _lib.E_USER_EXPR:                   # params = (energy_expr, grad_expr, float64 parameters, stats, energy0_expr)
                self._dev = engine.DeviceEnergy.from_expr(engine.context(device), self.ndims, *params)
            elif kind == _lib.E_LINEAR_EXPR:               # params = dict(W=, b=, energy=, grad=, params=, expert_params=[, tall=][, wide=][, groups=])
                if params.get('groups'):
                    self._dev = engine.DeviceEnergy.from_linear_grouped(
                        engine.context(device), params['W'], params.get('b'), params['groups'], params['energy'], params['grad'],
                        params.get('params', ()), params.get('expert_params'))
                else:
                    make = (engine.DeviceEnergy.from_linear_wide if params.get('wide') else
                            engine.DeviceEnergy.from_linear_tall if params.get('tall') else engine.DeviceEnergy.from_linear)
                    self._dev = make(engine.context(device), params['W'], params.get('b'), params['energy'], params['grad'],
                                     params.get('params', ()), params.get('expert_params'))
            elif kind == _lib.E_HOST:                      # params = (energy_func, energy_grad_func): opaque callables
                self._dev = engine.DeviceEnergy.host(engine.context(device), self.ndims, *params)
            else:
                self._dev = engine.DeviceEnergy(engine.context(device), kind, self.ndims, params)
        return self._dev

    # -- reference API --------------------------------------------------------------------
    def E(self, X):
        self.E_count += X.shape[1]
        return self.E_val(X)

    def E_val(self, X):
        E, _ = self.bind().eval(X, want_E=True, want_grad=False, dtype=self.state_dtype)
        return E.reshape((1, -1))

    def dEdX(self, X):
        self.dEdX_count += X.shape[1]
        return self.dEdX_val(X)

    def dEdX_val(self, X):
        _, G = self.bind().eval(X, want_E=False, want_grad=True, dtype=self.state_dtype)
        return G

    def __hash__(self):
        raise NotImplementedError()

    def init_X(self):
        try:
            self.gen_init_X()
        except NotImplementedError:
            self.Xinit = np.random.randn(self.ndims, self.nbatch)      # distributions.py:137-139

    def gen_init_X(self):
        raise NotImplementedError()

    # -- fair-initialisation cache (distributions.py:104-149, 182-195) ----------------------------
    @staticmethod
    def _cache_directory(directory=None):
        import os
        return directory or os.environ.get('MJHMC_INIT_CACHE') or os.path.join(
            os.path.expanduser('~'), '.cache', 'mjhmc_amd', 'initializations')

    def cached_init_X(self, directory=None, **generator_kwargs):
        """Set ``Xinit`` from the cached burn-in end points of this distribution (MJHMC end points when the
        distribution serves a continuous-time sampler, ControlHMC's otherwise), generating and caching them first
        when the cache file does not exist -- the reference's ``init_X`` (distributions.py:96-149).  Unlike the
        reference this is opt-in: ``init_X`` here never starts a 10^6-step burn-in behind the caller's back.
        ``generator_kwargs`` (burn_in_steps, var_steps, seed) go to gen_mj_init.generate_initialization."""
        import os
        from . import gen_mj_init as G
        directory = self._cache_directory(directory)
        name = '{}_{}.pickle'.format(type(self).__name__, G.stable_digest(self))
        if not os.path.exists(os.path.join(directory, name)):
            old_nbatch, old_mjhmc = self.nbatch, self.mjhmc
            self.nbatch = self.max_n_particles or G.MAX_N_PARTICLES
            self.generation_instance = True
            try:
                self.gen_init_X()                                     # start from the biased initialisation
            except NotImplementedError:
                self.Xinit = np.random.randn(self.ndims, self.nbatch)    # "completely arbitrary choice" (:137-139)
            try:
                G.cache_initialization(self, directory, **generator_kwargs)
            finally:
                self.nbatch, self.mjhmc = old_nbatch, old_mjhmc
                self.generation_instance = False
        mjhmc_endpt, _, _, control_endpt = G.load_initialization(self, directory)
        self.Xinit = (mjhmc_endpt if self.mjhmc else control_endpt)[:, :self.nbatch]

    def load_cache(self, directory=None):
        """(mjhmc_endpt, emc_var_estimate, true_var_estimate, control_endpt) of this distribution's cache file;
        raises if it does not exist (distributions.py:182-195)."""
        from . import gen_mj_init as G
        return G.load_initialization(self, self._cache_directory(directory))

    def reset(self):
        self.E_count = 0
        self.dEdX_count = 0
        if not self.generation_instance:
            self.init_X()
        return self

    def __call__(self, X):
        rshp_X = X.reshape(len(X), 1)
        E = float(np.asarray(self.E(rshp_X)).reshape(()))
        dEdX = self.dEdX(rshp_X).T[0]
        return -E, -dEdX


class LambdaDistribution(Distribution):
    """'Anonymous' distribution (distributions.py:198-251, README.md:27-36).

    The reference's class ignores its callables (it evaluates a non-existent ``self.J``); the README contract is
    what is kept: ``energy_func`` / ``energy_grad_func`` define the distribution and ``init`` is the initial state.
    Python callables cannot run inside a GPU kernel, so the callables reach the device in one of four ways:

    * nothing, and the callables are recognised: they are probed on a few points and matched against the built-in
      elementwise families (isotropic Gaussian with any sigma -- the README example -- and diagonal Gaussians);
    * nothing, and they are NOT recognised (any opaque pair of callables, e.g. a dense quadratic form): the sampler
      keeps the state and the whole jump process on the device and calls ``energy_grad_func`` back once per leapfrog
      step and ``energy_func`` once per iteration (MJHMC_E_HOST, mjhmc_traj_* of include/mjhmc_hip.h) -- correct for
      any callables, slow by construction (a host round trip per leapfrog step);
    * ``device_expr=(energy_expr, grad_expr)`` [+ ``device_params``]: C expressions of one coordinate for a separable
      energy ``E(x) = sum_d energy_expr(x_d)``, ``dE/dx_d = grad_expr(x_d)`` with ``x`` the coordinate, ``d`` its
      index and ``p[k]`` the float64 ``device_params``; the engine's kernels are compiled around them with hipRTC
      (mjhmc_energy_create_expr).  When callables are given as well they are checked against the compiled energy.
      Coupled coordinates: ``device_expr=dict(stats=[...], energy=..., energy0=..., grad=...)`` -- the ``stats``
      expressions are summed over a particle's coordinates into ``S[k]``, which the other expressions may use:
      ``E = energy0(S) + sum_d energy(x_d, d, S)``, ``dE/dx_d = grad(x_d, d, S)`` (mjhmc_energy_create_expr_coupled);
    * ``device_linear=dict(W=, b=, energy=, grad=, params=(), expert_params=None)``: a linear-model energy
      ``E(x) = sum_j energy(u_j, j)``, ``u = W x + b`` (W (K, D), K, D <= 512), ``dE/dx = W^T grad(u)``, with ``energy`` /
      ``grad`` C expressions of ``u``, ``j``, ``p[k]`` (``params``) and ``q[m]`` (row m of ``expert_params``) evaluated in
      float32 on the ProductOfT matrix-core tile kernels (mjhmc_energy_create_linear).  ``state_dtype``: 'float64'
      (default: float64 state around the float32 force, as ProductOfT) or 'float32'.  Callables given as well are checked
      against the device energy at bind time at a float32-force bar: ``|dE| <= 1e-4 (1 + |E|)`` and
      ``max |d grad| <= 1e-4 max(1, max |grad|)`` on a few probe points;
    * ``device_linear_tall=dict(W=, b=, energy=, grad=, params=(), expert_params=None)``: the same contract for a model
      with more experts than dims -- W (K, D), D <= 512, K <= 2**20 (a GLM posterior: an expert per data row) -- on one
      fused matrix-core kernel that walks the experts in blocks of the padded D (mjhmc_energy_create_linear_tall); ``j`` is
      the global expert index.  Samplers run the engine's multi-pass path with either ``state_dtype``; the callables are
      checked at the same float32-force bar;
    * ``device_linear_wide=dict(W=, b=, energy=, grad=, params=(), expert_params=None)``: the same contract for a model
      with more dims than 512 -- W (K, D), D <= 4096, K <= 2**20 (a regression with a thousand coefficients) -- on one fused
      matrix-core kernel that walks blocks of 512 experts x chunks of 512 dims (mjhmc_energy_create_linear_wide); ``j`` is
      the global expert index.  The multi-pass path with either ``state_dtype``, the same bar; the per-expert passes
      (``pointwise``, ``waic``, ``influence``) and ``cv_expectations`` take at most 512 dims and refuse it;
    * ``device_linear_grouped=dict(W=, b=, groups=(C, G), energy=, grad=, params=(), expert_params=None)``: the tall contract
      plus a log-sum-exp over groups of experts, ``E(x) = sum_j energy(u_j, j) + sum_{g<G} LSE_{c<C} u_{gC+c}`` -- the
      first G * C rows of W are G groups of C consecutive experts (softmax regression: a data row per group, a class per
      member; 2 <= C <= 16), the rest plain experts -- on a fused matrix-core kernel of its own
      (mjhmc_energy_create_linear_grouped); ``j`` is the caller's expert index.  The multi-pass path, the same bar;
    * ``device_energy=(kind, params)``: one of the built-in device energies by name.
    """

    def __init__(self, energy_func=None, energy_grad_func=None, init=None, name=None, device_energy=None,
                 device_expr=None, device_params=(), device_linear=None, state_dtype='float64', device_linear_tall=None,
                 device_linear_grouped=None, device_linear_wide=None):
        self.energy_func = energy_func
        self.energy_grad_func = energy_grad_func
        self.init = np.array(init, dtype=np.float64)
        self.name = name or str(np.random.random())
        self._functor = device_energy
        self._checked = False
        self._bar32 = False
        if sum(m is not None for m in (device_linear, device_linear_tall, device_linear_grouped, device_linear_wide)) > 1:
            raise ValueError('give device_linear or device_linear_tall, not both'
                             if device_linear_grouped is None and device_linear_wide is None else
                             'give one of device_linear, device_linear_tall, device_linear_wide and device_linear_grouped')
        if device_linear_grouped is not None:
            if state_dtype not in ('float32', 'float64'):
                raise ValueError("device_linear state_dtype must be 'float32' or 'float64'")
            self.state_dtype = state_dtype
            lin = dict(device_linear_grouped)
            if 'groups' not in lin:
                raise ValueError('device_linear_grouped needs groups=(C, G)')
            W, b, params, q, groups = engine.grouped_linear_arrays(lin['W'], lin.get('b'), lin['groups'], lin.get('params', ()),
                                                                   lin.get('expert_params'))
            if W.shape[1] != self.init.shape[0]:
                raise ValueError('W has %d columns but init has %d dims' % (W.shape[1], self.init.shape[0]))
            self._functor = (_lib.E_LINEAR_EXPR, dict(W=W, b=b, energy=str(lin['energy']), grad=str(lin['grad']), params=params,
                                                      expert_params=q, tall=True, groups=groups))
            self._bar32 = True
        elif device_linear is not None or device_linear_tall is not None or device_linear_wide is not None:
            tall, wide = device_linear_tall is not None, device_linear_wide is not None
            if state_dtype not in ('float32', 'float64'):
                raise ValueError("device_linear state_dtype must be 'float32' or 'float64'")
            self.state_dtype = state_dtype
            lin = dict(device_linear_wide if wide else device_linear_tall if tall else device_linear)
            W, b, params, q = engine.linear_arrays(lin['W'], lin.get('b'), lin.get('params', ()), lin.get('expert_params'),
                                                   _tall=tall, _wide=wide)
            if W.shape[1] != self.init.shape[0]:
                raise ValueError('W has %d columns but init has %d dims' % (W.shape[1], self.init.shape[0]))
            self._functor = (_lib.E_LINEAR_EXPR, dict(W=W, b=b, energy=str(lin['energy']), grad=str(lin['grad']),
                                                      params=params, expert_params=q,
                                                      **(dict(wide=True) if wide else dict(tall=True) if tall else {})))
            self._bar32 = True
        elif device_expr is not None:
            if isinstance(device_expr, dict):              # coupled through per-particle statistics S[k]
                e_expr, g_expr = device_expr['energy'], device_expr['grad']
                stats = device_expr.get('stats', ())
                stats = [stats] if isinstance(stats, str) else [str(t) for t in stats]
                e0 = device_expr.get('energy0')
            else:
                (e_expr, g_expr), stats, e0 = device_expr, [], None
            self._functor = (_lib.E_USER_EXPR, (str(e_expr), str(g_expr), np.asarray(device_params, dtype=np.float64),
                                                stats, None if e0 is None else str(e0)))
        elif self._functor is None:
            self._functor = _recognise(energy_func, energy_grad_func, self.init.shape[0])
            if self._functor is None and energy_func is not None and energy_grad_func is not None:
                self._functor = (_lib.E_HOST, (energy_func, energy_grad_func))       # opaque callables: host call-backs
            self._checked = True
        super(LambdaDistribution, self).__init__(ndims=self.init.shape[0], nbatch=self.init.shape[1])

    def device_energy(self):
        if self._functor is None:
            raise NotImplementedError('LambdaDistribution %r needs energy_func and energy_grad_func (or device_expr= / '
                                      'device_energy=)' % self.name)
        return self._functor

    def bind(self, device=0):
        dev = super(LambdaDistribution, self).bind(device)
        if not self._checked and self.energy_func is not None and self.energy_grad_func is not None:
            # the callables are the contract (README.md:27-36): the device energy must be the same function
            self._checked = True
            P = np.random.RandomState(12345).randn(self.ndims, 7)
            E, G = dev.eval(P)
            e = np.asarray(self.energy_func(P), dtype=np.float64).reshape(-1)
            g = np.asarray(self.energy_grad_func(P), dtype=np.float64)
            if self._bar32:      # float32 force (device_linear): the bar of the docstring
                ok = (np.all(np.abs(E - e) <= 1e-4 * (1 + np.abs(e))) and
                      np.abs(G - g).max() <= 1e-4 * max(1.0, np.abs(g).max()))
            else:
                ok = np.allclose(E, e, rtol=1e-9, atol=1e-12) and np.allclose(G, g, rtol=1e-9, atol=1e-12)
            if not ok:
                raise ValueError('LambdaDistribution %r: the device energy disagrees with energy_func / '
                                 'energy_grad_func (max |dE| %g, max |d grad| %g)'
                                 % (self.name, np.abs(E - e).max(), np.abs(G - g).max()))
        return dev

    def gen_init_X(self):
        self.Xinit = self.init

    def __hash__(self):
        return hash((self.ndims, self.nbatch, self.name))


def _recognise(energy_func, grad_func, ndims):
    """Match user callables against the built-in Gaussian families by probing (no sampling is ever done with the
    callables themselves): g(x) = j * x elementwise with E = sum j x^2 / 2 -- isotropic when all j are equal."""
    if energy_func is None or grad_func is None:
        return None
    rng = np.random.RandomState(12345)
    P = rng.randn(ndims, 5)
    try:
        g = np.asarray(grad_func(P), dtype=np.float64)
        e = np.asarray(energy_func(P), dtype=np.float64).reshape(-1)
    except Exception:
        return None
    if g.shape != P.shape or e.shape != (5,):
        return None
    ratio = g / P
    j = np.median(ratio, axis=1)
    if np.any(j <= 0) or not np.allclose(ratio, j[:, None], rtol=1e-12, atol=0):
        return None
    if not np.allclose(e, 0.5 * np.sum(j[:, None] * P ** 2, axis=0), rtol=1e-12, atol=0):
        return None
    if np.allclose(j, j[0], rtol=1e-12, atol=0):
        return (_lib.E_ISO_GAUSS, np.array([1.0 / np.sqrt(float(np.median(j)))]))
    return (_lib.E_DIAG_GAUSS, j)


class Gaussian(Distribution):
    """Ill-conditioned Gaussian of the LAHMC paper (distributions.py:256-281)."""

    def __init__(self, ndims=2, nbatch=100, log_conditioning=6):
        self.conditioning = 10 ** np.linspace(-log_conditioning, 0, ndims)
        self.J = np.diag(self.conditioning)
        self.description = '%dD Anisotropic Gaussian, %g self.conditioning' % (ndims, 10 ** log_conditioning)
        super(Gaussian, self).__init__(ndims, nbatch)

    def device_energy(self):
        return (_lib.E_DIAG_GAUSS, np.asarray(self.conditioning, dtype=np.float64))

    def gen_init_X(self):
        self.Xinit = (1. / np.sqrt(self.conditioning).reshape((-1, 1))) * np.random.randn(self.ndims, self.nbatch)

    def __hash__(self):
        return hash((self.ndims, hash(tuple(self.conditioning))))


class RoughWell(Distribution):
    """distributions.py:283-312."""

    def __init__(self, ndims=2, nbatch=100, scale1=100, scale2=4):
        self.scale1 = scale1
        self.scale2 = scale2
        self.description = '{} Rough Well'.format(ndims)
        super(RoughWell, self).__init__(ndims, nbatch)

    def device_energy(self):
        return (_lib.E_ROUGH_WELL, np.array([self.scale1, self.scale2], dtype=np.float64))

    def gen_init_X(self):
        self.Xinit = self.scale1 * np.random.randn(self.ndims, self.nbatch)

    def __hash__(self):
        return hash((self.ndims, self.scale1, self.scale2))


class MultimodalGaussian(Distribution):
    """distributions.py:314-346 (as coded: modes at -/+ 2*separation along the first axis)."""

    def __init__(self, ndims=2, nbatch=100, separation=3):
        self.separation = separation
        self.sep_vec = np.array([separation] * nbatch + [0] * (ndims - 1) * nbatch).reshape(ndims, nbatch)
        self.sep_vec[0] += separation
        super(MultimodalGaussian, self).__init__(ndims, nbatch)

    def device_energy(self):
        return (_lib.E_MM_GAUSS, np.array([self.separation], dtype=np.float64))

    def modes(self):
        """(2, ndims): the centres of the two modes as the energy codes them (csrc/energy_mm.hip), -/+ 2 * separation on
        the first axis -- ``sampler.occupancy(n_iter, distribution.modes())`` counts the hops between them"""
        c = np.zeros((2, self.ndims))
        c[0, 0], c[1, 0] = -2.0 * self.separation, 2.0 * self.separation
        return c

    def init_X(self):
        self.Xinit = ((np.random.randn(self.ndims, self.nbatch) + self.sep_vec) +
                      (np.random.randn(self.ndims, self.nbatch) - self.sep_vec))

    def __hash__(self):
        return hash((self.ndims, self.separation))


class TestGaussian(Distribution):
    """Unit-variance (or sigma) isotropic Gaussian (distributions.py:348-370)."""
    __test__ = False  # not a pytest class

    def __init__(self, ndims=2, nbatch=100, sigma=1.):
        self.sigma = sigma
        super(TestGaussian, self).__init__(ndims, nbatch)

    def device_energy(self):
        return (_lib.E_ISO_GAUSS, np.array([self.sigma], dtype=np.float64))

    def gen_init_X(self):
        self.Xinit = np.random.randn(self.ndims, self.nbatch)

    def __hash__(self):
        return hash((self.ndims, self.sigma))


class TFGaussian(TestGaussian):
    """The reference's TensorFlow twin of TestGaussian (mjhmc/misc/tf_distributions.py:179-201; float32 there because the
    placeholder is, `state_dtype='float32'` selects the same here); extra keyword arguments (``device``, ...) are the
    TensorFlow plumbing of the reference and are accepted and ignored."""

    def __init__(self, ndims=2, nbatch=100, sigma=1., state_dtype='float64', **kwargs):
        self.state_dtype = state_dtype
        super(TFGaussian, self).__init__(ndims=ndims, nbatch=nbatch, sigma=sigma)


class Funnel(Distribution):
    """Neal's funnel (mjhmc/misc/tf_distributions.py:142-177).

    ``literal=False`` (default): the density the reference documents, x0 ~ N(0, scale^2),
    x_k ~ N(0, e^{x0}).  ``literal=True``: the energy exactly as the reference codes it (:161-165),
    which is the negated un-normalised log-density -- chains diverge on it, kept for one-shot
    E/dEdX parity only.
    """

    def __init__(self, scale=1.0, nbatch=50, ndims=10, literal=False):
        self.scale = float(scale)
        self.literal = literal
        super(Funnel, self).__init__(ndims, nbatch)

    def device_energy(self):
        return (_lib.E_FUNNEL_REF if self.literal else _lib.E_FUNNEL_NEAL, np.array([self.scale]))

    def gen_init_X(self):
        x_0 = np.random.normal(scale=self.scale, size=(1, self.nbatch))
        # exact draw from the funnel (the reference passes exp(x_0) as the std, :171-173)
        x_k = np.random.normal(scale=np.exp(x_0 / 2.), size=(self.ndims - 1, self.nbatch))
        self.Xinit = np.vstack((x_0, x_k))

    def __hash__(self):
        return hash((self.scale, self.ndims))


class CorrelatedGaussian(Distribution):
    """Gaussian with a dense covariance, E = 1/2 (x - mu)^T A (x - mu), A = cov^-1 the precision, on the ProductOfT
    matrix-core tile kernels as a linear-model energy (mjhmc_energy_create_linear): W = L^T and b = -L^T mu for the
    Cholesky factor A = L L^T, f(u) = u^2 / 2, f'(u) = u (float32 force).  Give ``cov`` or ``precision`` (D x D,
    D <= 512); with neither, a seeded random rotation of a spectrum spanning 10^log_conditioning.
    ``state_dtype``: 'float64' (default, float64 state around the float32 force) or 'float32'.  ``gen_init_X`` draws
    exactly from N(mu, cov)."""

    def __init__(self, cov=None, precision=None, mean=None, ndims=None, nbatch=100, state_dtype='float64',
                 log_conditioning=2, seed=0):
        if state_dtype not in ('float32', 'float64'):
            raise ValueError("CorrelatedGaussian state_dtype must be 'float32' or 'float64'")
        if cov is not None and precision is not None:
            raise ValueError('give cov or precision, not both')
        if cov is None and precision is None:
            D = 2 if ndims is None else int(ndims)
            rs = np.random.RandomState(seed)
            Q, R = np.linalg.qr(rs.randn(D, D))
            Q = Q * np.sign(np.diag(R))
            spec = 10.0 ** np.linspace(-log_conditioning / 2.0, log_conditioning / 2.0, D)
            cov = (Q * spec) @ Q.T
        if precision is None:
            cov = np.array(cov, dtype=np.float64)
            precision = np.linalg.inv(cov)
        else:
            precision = np.array(precision, dtype=np.float64)
            cov = np.linalg.inv(precision)
        if precision.ndim != 2 or precision.shape[0] != precision.shape[1]:
            raise ValueError('cov / precision must be square, got shape %r' % (precision.shape,))
        D = precision.shape[0]
        precision = (precision + precision.T) / 2
        cov = (cov + cov.T) / 2
        self.mean = np.zeros(D) if mean is None else np.array(mean, dtype=np.float64).reshape(D)
        self.cov, self.precision = cov, precision
        self.L = np.linalg.cholesky(precision)           # A = L L^T
        self.state_dtype = state_dtype
        self.backend = 'hip-mfma'
        super(CorrelatedGaussian, self).__init__(D, nbatch)

    def device_energy(self):
        W = self.L.T
        return (_lib.E_LINEAR_EXPR, dict(W=W, b=-W @ self.mean, energy='0.5f*u*u', grad='u', params=(),
                                         expert_params=None))

    def gen_init_X(self):
        C = np.linalg.cholesky(self.cov)
        self.Xinit = self.mean.reshape(-1, 1) + C @ np.random.randn(self.ndims, self.nbatch)

    def __hash__(self):
        import hashlib
        h = hashlib.sha1()
        for a in (self.precision, self.mean):
            h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
        return int(h.hexdigest()[:15], 16)


class GeneralizedLinearModel(Distribution):
    """Posterior of the coefficients x of a generalized linear model under the prior x ~ N(0, prior_scale^2 I):
    ``features`` (n, D), ``targets`` (n,).  A linear-model energy of K = n + D experts -- the n data rows, then the prior
    as D more experts with rows I / prior_scale and f = u^2 / 2:

    * ``'gaussian'``: y ~ N(a.x, noise_scale^2); rows features / noise_scale, b = -targets / noise_scale, f = u^2 / 2;
    * ``'logistic'``: y in {0, 1}, P(y = 1) = sigmoid(a.x); f = softplus(u) - y u, f' = sigmoid(u) - y;
    * ``'poisson'``: y ~ Poisson(exp(a.x)); f = exp(u) - y u, f' = exp(u) - y  (constants in y dropped).

    For the two non-Gaussian families the per-expert rows are q[0] = y and q[1] = 1 on the data rows, 0 on the prior rows
    (the expressions select the prior's term by q[1]).  K > 512 runs as a tall model on the fused block kernel
    (mjhmc_energy_create_linear_tall, D <= 512, K <= 2**20), K <= 512 on the tile kernels (mjhmc_energy_create_linear).
    More than 512 features need ``wide=True``: the model then runs as a wide one on the fused kernel over blocks of experts
    x chunks of dims (mjhmc_energy_create_linear_wide, D <= 4096, K <= 2**20), whatever its D; the per-expert passes
    ``pointwise``, ``waic`` and ``influence`` take at most 512 dims and refuse a wide model.  Without it such a model is
    refused as it always was: a caller who relies on those passes learns at construction that they are not to be had.
    ``E_host`` / ``dEdX_host`` are the same energy in float64 NumPy; ``posterior()`` is exact for the Gaussian family.
    ``gen_init_X`` draws N(0, init_scale^2) (from ``seed`` when given)."""

    _PRIOR = ('0.5f*u*u', 'u')
    _DATA = {
        'logistic': ('(u > 20.f ? u : log1pf(expf(u))) - q[0]*u', '1.f/(1.f + expf(-u)) - q[0]'),
        'poisson': ('expf(u) - q[0]*u', 'expf(u) - q[0]'),
    }

    def __init__(self, features, targets, family, prior_scale=1.0, noise_scale=1.0, nbatch=100, init_scale=0.1, seed=None,
                 state_dtype='float64', wide=False):
        if state_dtype not in ('float32', 'float64'):
            raise ValueError("GeneralizedLinearModel state_dtype must be 'float32' or 'float64'")
        if family not in ('gaussian', 'logistic', 'poisson'):
            raise ValueError("family must be 'gaussian', 'logistic' or 'poisson', got %r" % (family,))
        A = np.array(features, dtype=np.float64)
        y = np.array(targets, dtype=np.float64)
        if A.ndim != 2 or A.shape[0] < 1 or A.shape[1] < 1:
            raise ValueError('features must be an (n, D) matrix, got shape %r' % (A.shape,))
        n, D = A.shape
        if y.shape != (n,):
            raise ValueError('targets must have one entry per row of features (%d), got shape %r' % (n, y.shape))
        if not (prior_scale > 0 and noise_scale > 0):
            raise ValueError('prior_scale and noise_scale must be positive')
        if family == 'logistic' and not np.all((y == 0) | (y == 1)):
            raise ValueError('logistic targets must be 0 or 1')
        if family == 'poisson' and np.any(y < 0):
            raise ValueError('poisson targets must be non-negative')
        self.features, self.targets, self.family = A, y, family
        self.prior_scale, self.noise_scale = float(prior_scale), float(noise_scale)
        self.init_scale, self.seed = float(init_scale), seed
        prior = np.eye(D) / self.prior_scale
        if family == 'gaussian':
            self.W = np.vstack([A / self.noise_scale, prior])
            self.b = np.concatenate([-y / self.noise_scale, np.zeros(D)])
            self.q = None
        else:
            self.W = np.vstack([A, prior])
            self.b = np.zeros(n + D)
            self.q = np.vstack([np.concatenate([y, np.zeros(D)]), np.concatenate([np.ones(n), np.zeros(D)])])
        self.wide = bool(wide)
        if D > 512 and not self.wide:
            raise ValueError('GeneralizedLinearModel takes at most 512 dims in its tile and tall forms (features are %d x %d); '
                             'wide=True takes the wide form, up to 4096 dims, without pointwise / waic / influence' % (n, D))
        # the size limits, before anything else
        (engine.wide_linear_arrays if self.wide else engine.tall_linear_arrays)(self.W, self.b, (), self.q)
        self.nexperts = n + D
        self.state_dtype = state_dtype
        self.backend = 'hip-mfma'
        super(GeneralizedLinearModel, self).__init__(D, nbatch)

    def device_energy(self):
        if self.family == 'gaussian':
            e, g = self._PRIOR
        else:
            (de, dg), (pe, pg) = self._DATA[self.family], self._PRIOR
            e = 'q[1] != 0.f ? (%s) : (%s)' % (de, pe)
            g = 'q[1] != 0.f ? (%s) : (%s)' % (dg, pg)
        d = dict(W=self.W, b=self.b, energy=e, grad=g, params=(), expert_params=self.q)
        if self.wide:
            d['wide'] = True
        elif self.nexperts > 512:
            d['tall'] = True
        return (_lib.E_LINEAR_EXPR, d)

    _FITTED = {'logistic': '1.f/(1.f + expf(-u))', 'poisson': 'expf(u)'}

    def pointwise_values(self):
        """(values, log_mean_exp flags) of ``sampler.pointwise()`` / ``waic()`` over all K = n + D experts: value 0 is the
        pointwise log-likelihood l = -(energy expression), without the constants the energy leaves out
        (``log_lik_constants``), with log-mean-exp on; value 1 is the fitted mean -- u (gaussian: the standardised
        residual (a.x - y) / noise_scale, see ``fitted_from_value``), sigmoid(u) (logistic), exp(u) (poisson), and 0 on
        the prior's experts of the two non-Gaussian families (selected by q[1] as the energy selects them)."""
        energy = self.device_energy()[1]['energy']
        fitted = 'u' if self.family == 'gaussian' else 'q[1] != 0.f ? (%s) : 0.f' % self._FITTED[self.family]
        return ['-(%s)' % energy, fitted], [True, False]

    def influence_value(self):
        """the value of ``sampler.influence()``: value 0 of ``pointwise_values()``, the pointwise log-likelihood l of every
        expert without its constants (they do not enter a covariance) -- on the first ``n_data`` experts the data rows,
        on the last ndims the prior's terms"""
        return self.pointwise_values()[0][0]

    @property
    def n_data(self):
        """the experts that are data rows: the first n of the K = n + ndims"""
        return int(self.features.shape[0])

    def log_lik_constants(self):
        """the n per-row constants of log p(y_i | x) that the energy drops"""
        n = self.features.shape[0]
        if self.family == 'gaussian':
            return np.full(n, -np.log(self.noise_scale) - 0.5 * np.log(2 * np.pi))
        if self.family == 'logistic':
            return np.zeros(n)
        from scipy.special import gammaln
        return -gammaln(self.targets + 1.0)

    def fitted_from_value(self, v):
        """value 1 on the data rows -> the fitted mean of y: a.x = u noise_scale + y for the gaussian family"""
        v = np.asarray(v, dtype=np.float64)
        return v * self.noise_scale + self.targets if self.family == 'gaussian' else v

    def _terms(self, X):
        """u (K, n), f(u), f'(u) in float64"""
        u = self.W.dot(np.asarray(X, dtype=np.float64)) + self.b[:, None]
        f, fp = 0.5 * u * u, u.copy()
        if self.family != 'gaussian':
            nd = self.features.shape[0]
            ud, yd = u[:nd], self.targets[:, None]
            if self.family == 'logistic':
                f[:nd] = np.logaddexp(0.0, ud) - yd * ud
                fp[:nd] = 0.5 * (1.0 + np.tanh(0.5 * ud)) - yd        # sigmoid, without overflow
            else:
                f[:nd] = np.exp(ud) - yd * ud
                fp[:nd] = np.exp(ud) - yd
        return u, f, fp

    def E_host(self, X):
        return self._terms(X)[1].sum(axis=0).reshape((1, -1))

    def dEdX_host(self, X):
        return self.W.T.dot(self._terms(X)[2])

    def posterior(self):
        """(mean, cov) of the posterior; the Gaussian family only (the others have no closed form)"""
        if self.family != 'gaussian':
            raise NotImplementedError('posterior() is exact for the gaussian family only')
        precision = self.W.T.dot(self.W)
        cov = np.linalg.inv(precision)
        cov = (cov + cov.T) / 2
        return np.linalg.solve(precision, -self.W.T.dot(self.b)), cov

    def gen_init_X(self):
        rs = np.random if self.seed is None else np.random.RandomState(self.seed)
        self.Xinit = self.init_scale * rs.randn(self.ndims, self.nbatch)

    def __hash__(self):
        import hashlib
        h = hashlib.sha1()
        h.update(self.family.encode())
        for a in (self.features, self.targets, [self.prior_scale, self.noise_scale]):
            h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
        return int(h.hexdigest()[:15], 16)


class MultinomialLogisticRegression(Distribution):
    """Posterior of the coefficients of a multinomial logistic (softmax) regression under the prior B ~ N(0, prior_scale^2 I):
    ``features`` (n, F), ``targets`` (n,) integers in 0 .. C - 1, ``n_classes`` = C (2 <= C <= 16).  The state is
    x = vec(B), B (C, F) row-major, ndims = C F <= 512, and P(y = c | a) = softmax(B a)_c, so

        E(x) = sum_i [ LSE_c (B a_i)_c - (B a_i)_{y_i} ] + |x|^2 / (2 prior_scale^2).

    A grouped linear-model energy (mjhmc_energy_create_linear_grouped) of K = n C + C F experts: data expert i C + c has
    the row a_i in block c of x, q[0] = [c == y_i] and q[1] = 1 with f = -q[0] u (the log-sum-exp of the group is the
    kernel's); then the prior as C F more experts with rows I / prior_scale and f = u^2 / 2, selected by q[1] = 0 as
    GeneralizedLinearModel selects its prior.  ``E_host`` / ``dEdX_host`` are the same energy in float64 NumPy with a stable
    log-sum-exp; ``predict_proba(X)`` gives the class probabilities of ``features`` under coefficient vectors, on the
    host; ``group_values()`` / ``log_lik_constants()`` are what ``sampler.group_waic()`` asks the data rows on the device.
    ``gen_init_X`` draws N(0, init_scale^2) (from ``seed`` when given)."""

    def __init__(self, features, targets, n_classes, prior_scale=1.0, nbatch=100, init_scale=0.1, seed=None,
                 state_dtype='float64'):
        if state_dtype not in ('float32', 'float64'):
            raise ValueError("MultinomialLogisticRegression state_dtype must be 'float32' or 'float64'")
        A = np.array(features, dtype=np.float64)
        if A.ndim != 2 or A.shape[0] < 1 or A.shape[1] < 1:
            raise ValueError('features must be an (n, F) matrix, got shape %r' % (A.shape,))
        n, F = A.shape
        C = int(n_classes)
        if C != n_classes or C < 2 or C > engine.GROUP_MAX:
            raise ValueError('n_classes must be an integer in 2 .. %d, got %r' % (engine.GROUP_MAX, n_classes))
        y = np.asarray(targets)
        if y.shape != (n,):
            raise ValueError('targets must have one entry per row of features (%d), got shape %r' % (n, y.shape))
        yi = y.astype(np.int64)
        if not np.all(yi == y) or yi.min() < 0 or yi.max() >= C:
            raise ValueError('targets must be integers in 0 .. n_classes - 1 = %d' % (C - 1))
        if not prior_scale > 0:
            raise ValueError('prior_scale must be positive')
        if C * F > 512:
            raise ValueError('ndims = n_classes * F = %d is more than the 512 dims a linear model takes' % (C * F))
        self.features, self.targets, self.n_classes = A, yi, C
        self.prior_scale, self.init_scale, self.seed = float(prior_scale), float(init_scale), seed
        D = C * F
        Wd = np.zeros((n, C, D))
        for c in range(C):
            Wd[:, c, c * F:(c + 1) * F] = A
        self.W = np.vstack([Wd.reshape(n * C, D), np.eye(D) / self.prior_scale])
        self.b = np.zeros(n * C + D)
        onehot = (np.arange(C)[None, :] == yi[:, None]).astype(np.float64).reshape(-1)
        self.q = np.vstack([np.concatenate([onehot, np.zeros(D)]), np.concatenate([np.ones(n * C), np.zeros(D)])])
        self.groups = (C, n)
        engine.grouped_linear_arrays(self.W, self.b, self.groups, (), self.q)       # the size limits, before anything else
        self.nexperts = n * C + D
        self.state_dtype = state_dtype
        self.backend = 'hip-mfma'
        super(MultinomialLogisticRegression, self).__init__(D, nbatch)

    def device_energy(self):
        return (_lib.E_LINEAR_EXPR, dict(W=self.W, b=self.b, energy='q[1] != 0.f ? -q[0]*u : 0.5f*u*u',
                                         grad='q[1] != 0.f ? -q[0] : u', params=(), expert_params=self.q, tall=True,
                                         groups=self.groups))

    @property
    def n_data(self):
        return int(self.features.shape[0])

    def group_values(self):
        """(values, log_mean_exp flags, per) of ``sampler.group_pointwise()`` / ``group_waic()`` over the n data rows: value 0
        is the row's log-likelihood u_y - LSE_c u_c, as q[0]*(u - lse) summed over the row's classes (q[0] one-hot: one
        term is not zero), per group, with log-mean-exp on; value 1 is the softmax ``sm``, per member -- the fitted class
        probabilities."""
        return ['q[0]*(u - lse)', 'sm'], [True, False], ['group', 'member']

    def log_lik_constants(self):
        """the n per-row constants of log p(y_i | x) that value 0 of ``group_values()`` leaves out: none"""
        return np.zeros(self.features.shape[0])

    def _logits(self, X):
        """(n, C, N): B a_i for every coefficient vector (column) of X"""
        X = np.asarray(X, dtype=np.float64)
        B = X.reshape(self.n_classes, self.features.shape[1], -1)
        return np.einsum('if,cfn->icn', self.features, B)

    @staticmethod
    def _lse(u):
        """stable log-sum-exp over axis 1, and the softmax"""
        m = u.max(axis=1, keepdims=True)
        t = np.exp(u - m)
        s = t.sum(axis=1, keepdims=True)
        return (m + np.log(s))[:, 0], t / s

    def E_host(self, X):
        X = np.asarray(X, dtype=np.float64)
        u = self._logits(X)
        lse, _ = self._lse(u)
        own = np.take_along_axis(u, self.targets[:, None, None], axis=1)[:, 0]
        prior = 0.5 * np.sum(X * X, axis=0) / self.prior_scale ** 2
        return ((lse - own).sum(axis=0) + prior).reshape((1, -1))

    def dEdX_host(self, X):
        X = np.asarray(X, dtype=np.float64)
        _, sm = self._lse(self._logits(X))
        sm[np.arange(sm.shape[0]), self.targets] -= 1.0
        G = np.einsum('icn,if->cfn', sm, self.features).reshape(X.shape)
        return G + X / self.prior_scale ** 2

    def predict_proba(self, X, features=None):
        """(n, C, N): P(y = c | a_i) under every coefficient vector (column) of X (D, N); ``features``: other rows (m, F)"""
        X = np.asarray(X, dtype=np.float64)
        if X.ndim == 1:
            X = X[:, None]
        A = self.features if features is None else np.asarray(features, dtype=np.float64)
        B = X.reshape(self.n_classes, self.features.shape[1], -1)
        return self._lse(np.einsum('if,cfn->icn', A, B))[1]

    def gen_init_X(self):
        rs = np.random if self.seed is None else np.random.RandomState(self.seed)
        self.Xinit = self.init_scale * rs.randn(self.ndims, self.nbatch)

    def __hash__(self):
        import hashlib
        h = hashlib.sha1()
        h.update(b'multinomial')
        for a in (self.features, self.targets, [self.n_classes, self.prior_scale]):
            h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
        return int(h.hexdigest()[:15], 16)


class ProductOfT(Distribution):
    """Product of Student-t experts (distributions.py:373-453).  The reference builds E and its
    gradient with Theano in float32; here both GEMMs of the gradient run on the MI355X matrix
    cores (exact-f32 MFMA).  ndims == nbasis, as the reference's initialiser requires (:391-392); any size (up to 512 dims
    on the register-resident tile kernels, beyond that block by block on the engine's multi-pass path).

    ``state_dtype``: 'float64' (default) is the reference's own arithmetic -- float64 ``HMCState`` arrays around the
    float32 force (:408-415 with hmc_state.py:29-38) -- on the tile kernel with the state streamed through its epilogue
    (csrc/dense_pot64.hip); 'float32' (extension, BASELINE configs[2]'s wording) keeps the particle state in float32
    too: the fused float32 tile kernel, ~7 % faster."""

    def __init__(self, ndims=36, nbasis=36, nbatch=100, lognu=None, W=None, b=None, state_dtype='float64'):
        if ndims != nbasis:
            raise NotImplementedError("Initializer only works for ndims == nbasis")
        if state_dtype not in ('float32', 'float64'):
            raise ValueError("ProductOfT state_dtype must be 'float32' or 'float64'")
        self.nbasis = nbasis
        self.state_dtype = state_dtype
        self.backend = 'hip-mfma'
        if W is None:
            W = np.eye(ndims, nbasis)
        self.weights = np.array(W, dtype='float32')
        pre_nu = np.random.rand(nbasis,) * 2 + 2.1 if lognu is None else np.exp(lognu)
        self.nu = np.array(pre_nu, dtype='float32')
        self.bias = np.array(np.zeros((nbasis,)) if b is None else b, dtype='float32')
        super(ProductOfT, self).__init__(ndims, nbatch)

    def device_energy(self):
        params = np.concatenate([[float(self.nbasis)], self.weights.astype(np.float64).ravel(),
                                 self.nu.astype(np.float64), self.bias.astype(np.float64)])
        return (_lib.E_PRODUCT_OF_T, params)

    def gen_init_X(self):
        from scipy import stats
        Zinit = np.zeros((self.ndims, self.nbatch))
        for ii in range(self.ndims):
            Zinit[ii] = stats.t.rvs(self.nu[ii], size=self.nbatch)
        Yinit = Zinit - self.bias.reshape((-1, 1))
        self.Xinit = np.dot(np.linalg.inv(self.weights), Yinit)

    def __hash__(self):
        return hash((self.ndims, self.nbasis, hash(tuple(self.nu)), hash(tuple(self.weights.ravel())),
                     hash(tuple(self.bias.ravel()))))


class SparseImageCode(Distribution):
    """Posterior over sparse-coding coefficients (mjhmc/misc/tf_distributions.py:204-284):
    E = mean_p 1/2 |y_p - B a_p|^2 + lambda * sum log(1 + a^2)   (Cauchy; ``cauchy=False``: lambda * sum |a|).

    The reference reads ``distr_data/dump_{n_basis}.pkl`` (basis (256, n_basis) and image patches), which is
    not part of the reference checkout; pass ``basis`` (img_size, n_coeffs) and ``imgs`` (img_size, >= n_patches)
    instead.  State rows are patch-major (row p * n_coeffs + c), which is what the reference's reshape yields for
    one active column.  The device kernels (bf16 matrix-core operands, fp32 accumulation) cover img_size = 256,
    n_coeffs = 1024 or 512, n_patches 1 ... 32.

    ``state_dtype``: 'float32' (default) keeps the state as the reference does (TensorFlow float32 placeholders,
    tf_distributions.py:89); 'bfloat16' is BASELINE.json configs[4] ("bf16 state / fp32 accumulate"): half the state bytes,
    the same kernel time -- and a MarkovJumpHMC chain that runs measurably hot, because a state rounded to 8 bits at every
    commit makes L irreversible (F L F L z != z at the 2^-9 level) while the jump process relies on exactly that identity
    (tests/test_gpu_stationary.py::test_sic_stationary_law).  The discrete-time samplers
    (ControlHMC / HMC: Metropolis accept) keep the law with either."""

    def __init__(self, n_patches=9, n_batches=10, cauchy=True, n_basis=1024, basis=None, imgs=None, init=None,
                 state_dtype='float32'):
        self.max_n_particles = 50
        self.lmbda = 0.01
        if basis is None or imgs is None:
            raise IOError('distr_data/dump_%d.pkl is not shipped with the reference: pass basis= and imgs=' % n_basis)
        self.basis = np.asarray(basis, dtype=np.float64)
        self.imgs = np.asarray(imgs, dtype=np.float64)
        self.img_size, self.n_coeffs = self.basis.shape
        assert self.n_coeffs == n_basis
        self.n_patches = n_patches
        self.cauchy = cauchy
        self.patches = self.imgs[:, :n_patches].T            # (n_patches, img_size)
        self._init = init
        if state_dtype not in ('float32', 'bfloat16'):
            raise ValueError("SparseImageCode state_dtype must be 'float32' or 'bfloat16'")
        self.state_dtype = state_dtype
        self.backend = 'hip-mfma-bf16'
        super(SparseImageCode, self).__init__(ndims=n_patches * self.n_coeffs, nbatch=n_batches)

    def device_energy(self):
        params = np.concatenate([[float(self.n_patches), float(self.img_size), float(self.n_coeffs), self.lmbda,
                                  1.0 if self.cauchy else 0.0], self.basis.ravel(), self.patches.ravel()])
        return (_lib.E_SPARSE_CODE, params)

    def gen_init_X(self):
        if self._init is not None:
            self.Xinit = np.asarray(self._init, dtype=np.float64)
        else:
            self.Xinit = 0.1 * np.random.randn(self.ndims, self.nbatch)

    def __hash__(self):
        return hash((hash(self.imgs.tobytes()), hash(self.basis.tobytes()), hash(self.lmbda), hash(self.n_patches),
                     self.n_coeffs))
