"""ProductOfT with float64 state: the tile kernel reads its particle rows at the start of a trajectory and writes them at
its end through an LDS staging image (dense_pot64_kernels.hpp: staged_start, staged_end_x, staged_end_vg).  Each case
is checked bit for bit against the multi-pass form of the same arithmetic (the test build's MJHMC_POT64_MULTIPASS=1),
at the shapes where the staging has edges: ragged batches (N not a multiple of 32: a padded last forward tile), inverse-L
items (MJHMC's R-movers, whose list's last tile repeats a column), NB = 1, 2, 4 (ndims <= 128, 256, 512), and L = 1 and 2,
where the first kick / drift pass is also the last drift."""
import numpy as np
import pytest

from tests.helpers import ref_init_weights, hooks_context, iterate_multipass_pair, assert_multipass_pair_equal

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('D,N,mode,L', [
    (100, 70, 'MJHMC', 1), (100, 300, 'CONTROL', 2),
    (200, 65, 'CTHMC', 1), (200, 300, 'MJHMC', 2),
    (512, 100, 'MJHMC', 1), (512, 70, 'MJHMC', 2), (512, 333, 'MJHMC', 3), (512, 70, 'CONTROL', 2), (512, 97, 'CTHMC', 1)])
def test_pot64_staged_rows_equal_multipass(D, N, mode, L, monkeypatch):
    from mjhmc_amd import engine, _lib
    ctxs = (engine.context(0), hooks_context(0))
    W, lognu = ref_init_weights(D, D)
    W = W + np.eye(D)
    params = np.concatenate([[float(D)], W.ravel(), np.exp(lognu), 0.1 * np.random.RandomState(2).randn(D)])
    ens = [engine.DeviceEnergy(c, _lib.E_PRODUCT_OF_T, D, params) for c in ctxs]
    X0 = np.random.RandomState(4).randn(D, N)
    pair = [engine.DeviceSampler(en, X0, seed=11, dtype='float64', mode=getattr(_lib, 'MODE_' + mode)) for en in ens]
    stats = [[], []]
    # p_r = 0.4: many R-movers, so every MJHMC iteration has inverse-L items
    hparams = (0.1, L, 0.4, 0.3) if mode == 'CONTROL' else (0.1, L, 0.4, 1.0)
    for n_it in (1, 3, 2):
        for k, st in enumerate(iterate_multipass_pair(pair, n_it, hparams, monkeypatch)):
            stats[k] += [t[:7] for t in st]
        assert_multipass_pair_equal(pair, n_it)
    assert stats[0] == stats[1]
    if mode == 'MJHMC':
        cold = [t[4] for t in stats[0]]
        assert any(n % 32 for n in cold), cold    # inverse-L items, with a padded last list tile
    for s in pair:
        s.close()
