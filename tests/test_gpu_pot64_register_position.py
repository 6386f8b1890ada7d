"""ProductOfT with float64 state: the tile kernel holds the float64 position as a register tile for the whole trajectory
(dense_pot64_kernels.hpp: kick_drift_pass works on registers alone; staged_start takes X from the staging image into
the tile, staged_end_x puts the tile back) and, at NB = 4, runs its GEMMs with half-chunk A-row sets
(dense_pot_tile.hpp: gemm_dim_half).  Each case is the product library against the multi-pass form of the same
arithmetic (the test build's MJHMC_POT64_MULTIPASS=1): X, V, dE/dX, E(X) and the transitions bit for bit; the kinetic
energy's squares are added up in another order in the two forms (EV, HFLF: 1e-12; DWELL, a difference of near-equal
rates: 1e-7) -- test_pot64_fused_equals_multipass's own tolerances.

Shapes: D = 512 / 130 / 36 are the three instances (NB = 4, 2, 1); N = 33 is two tiles, the second with one live
column, N = 64 two full ones; L = 1 has no middle pass (the first pass is the last drift), L = 2 exactly one, L = 5
several.  Every pair of (N, L), (N, mode) and (L, mode) occurs at every D."""
import numpy as np
import pytest

from tests.helpers import ref_init_weights, hooks_context, iterate_multipass_pair, assert_multipass_pair_equal

pytestmark = pytest.mark.gpu

def _pair(D, N, mode, bias_seed, x_seed, seed):
    from mjhmc_amd import engine, _lib
    ctxs = (engine.context(0), hooks_context(0))
    W, lognu = ref_init_weights(D, D)
    W = W + np.eye(D)
    params = np.concatenate([[float(D)], W.ravel(), np.exp(lognu), 0.1 * np.random.RandomState(bias_seed).randn(D)])
    ens = [engine.DeviceEnergy(c, _lib.E_PRODUCT_OF_T, D, params) for c in ctxs]
    X0 = np.random.RandomState(x_seed).randn(D, N)
    return [engine.DeviceSampler(en, X0, seed=seed, dtype='float64', mode=getattr(_lib, 'MODE_' + mode)) for en in ens]


_CASES = [(N, L, mode) for N, L, mode in ((33, 1, 'MJHMC'), (64, 1, 'CONTROL'), (33, 2, 'MJHMC'), (64, 2, 'CONTROL'),
                                          (33, 5, 'CONTROL'), (64, 5, 'MJHMC'))]


@pytest.mark.parametrize('N,L,mode', _CASES)
@pytest.mark.parametrize('D', [512, 130, 36])
def test_pot64_register_position_equals_multipass(D, N, L, mode, monkeypatch):
    """4 iterations (one call of 1, one of 3).  MJHMC: p_r = 0.4 lists R-movers, so the launches carry inverse-L items --
    the trajectory from (X, -V) whose end-point position is dropped -- in a padded last list tile."""
    pair = _pair(D, N, mode, bias_seed=2, x_seed=4, seed=11)
    hparams = (0.1, L, 0.4, 0.3) if mode == 'CONTROL' else (0.1, L, 0.4, 1.0)
    stats = [[], []]
    for n_it in (1, 3):
        a, b = iterate_multipass_pair(pair, n_it, hparams, monkeypatch)
        stats[0] += a
        stats[1] += b
        assert_multipass_pair_equal(pair, (D, N, L, mode, n_it))
    assert [t[:7] for t in stats[0]] == [t[:7] for t in stats[1]]
    if mode == 'MJHMC':
        n_flf_run = [t[7] for t in stats[0]]
        assert sum(n_flf_run) > 0, n_flf_run                      # inverse-L items were integrated ...
        assert any(n % 32 for n in n_flf_run), n_flf_run          # ... with a padded last list tile
    for s in pair:
        s.close()


def test_pot64_half_depth_gemm_one_step(monkeypatch):
    """The half-chunk A-row sets alone: D = 512, one tile, one leapfrog step, biases 0.1 randn.  dE/dX after one step is
    GEMM 2 of GEMM 1 of the drifted position: an A half-set that is stale, or requested for the wrong half-chunk,
    changes it."""
    from mjhmc_amd import _lib
    pair = _pair(512, 32, 'MJHMC', bias_seed=1, x_seed=3, seed=8)
    a, b = iterate_multipass_pair(pair, 1, (0.1, 1, 0.2, 1.0), monkeypatch)
    assert_multipass_pair_equal(pair, 'half-depth')
    assert [t[:7] for t in a] == [t[:7] for t in b]
    G =pair[0].read(_lib.F_DEDX)
    assert np.isfinite(G).all() and np.abs(G).max() > 0
    for s in pair:
        s.close()
