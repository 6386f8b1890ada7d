"""ProductOfT with float64 state at NB = 4: both GEMMs of a gradient run their last half-chunk block by block
(dense_pot_tile.hpp: half_mfma_tail), and in a trajectory's middle steps phi / publish of the finished blocks issue
between GEMM 1's last MFMAs and their kick / drift between GEMM 2's (dense_pot64_kernels.hpp: StepTail).  Each case is
the product library against the multi-pass form of the same arithmetic (the test build's MJHMC_POT64_MULTIPASS=1),
whose GEMMs walk whole chunks (gemm_dim): a wrong k-order, B quad or A row in the block-ordered half-chunk, or an
element whose phi or pass is taken twice or not at all, shows.  Fields and tolerances are those of
test_gpu_pot64_register_position.py: X, V, dE/dX, E(X), the transitions and the counters bit for bit; the kinetic
energy's squares are added up in another order in the two forms (EV, HFLF: 1e-12; DWELL, a difference of near-equal
rates: 1e-7).

Weights: a DENSE W = randn(D, D) / sqrt(D) + I with biases 0.1 randn -- every k-term of every block is non-zero, so a
dropped or misplaced one changes a float32 sum (under the reference's 5 %-sparse recipe most terms are zero).

Shapes: D = 512 is the new path at NB = 4, exact; D = 400 the same with padded rows; D = 130 is NB = 2, whose path is
unchanged (a leak of the new path would show).  N = 32 is one full tile, N = 33 two, the second with one live column.
L = 1: the gradient is the energy step's (block-ordered GEMMs, whole-tile stage behind GEMM 1, no pass); L = 2: exactly
one middle step -- one phi and one pass under the GEMMs; L = 5: several.  Every pair of (L, mode), (N, L) and
(N, mode) occurs at every D."""
import functools

import numpy as np
import pytest

from tests.helpers import ref_init_weights, hooks_context, iterate_multipass_pair, assert_multipass_pair_equal

pytestmark = pytest.mark.gpu

@functools.lru_cache(maxsize=None)
def _params(D, bias_seed):
    rs = np.random.RandomState(100 + D)
    W = rs.randn(D, D) / np.sqrt(D) + np.eye(D)
    _, lognu = ref_init_weights(D, D)
    return np.concatenate([[float(D)], W.ravel(), np.exp(lognu), 0.1 * np.random.RandomState(bias_seed).randn(D)])


def _pair(D, N, mode, bias_seed, x_seed, seed):
    from mjhmc_amd import engine, _lib
    ctxs = (engine.context(0), hooks_context(0))
    params = _params(D, bias_seed)
    ens = [engine.DeviceEnergy(c, _lib.E_PRODUCT_OF_T, D, params) for c in ctxs]
    X0 = np.random.RandomState(x_seed).randn(D, N)
    return [engine.DeviceSampler(en, X0, seed=seed, dtype='float64', mode=getattr(_lib, 'MODE_' + mode)) for en in ens]


_CASES = [(33, 1, 'MJHMC'), (32, 1, 'CTHMC'), (33, 1, 'CONTROL'),
          (32, 2, 'MJHMC'), (33, 2, 'CTHMC'), (32, 2, 'CONTROL'),
          (33, 5, 'MJHMC'), (32, 5, 'CTHMC'), (33, 5, 'CONTROL')]


@pytest.mark.parametrize('N,L,mode', _CASES)
@pytest.mark.parametrize('D', [512, 400, 130])
def test_pot64_tail_blocks_equal_multipass(D, N, L, mode, monkeypatch):
    """1 + 3 iterations.  MJHMC: p_r = 0.4 lists R-movers, so the launches carry inverse-L items -- the trajectory from
    (X, -V) whose end-point position is dropped -- in a padded list tile."""
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
        assert sum(n_flf_run) > 0, n_flf_run                      # inverse-L items were integrated
    for s in pair:
        s.close()


def test_pot64_block_ordered_half_chunk_one_step(monkeypatch):
    """The block-ordered last half-chunk alone: D = 512, one tile, one leapfrog step, nothing under the GEMMs' tails.
    dE/dX after one step is GEMM 2 of GEMM 1 of the drifted position: a B quad or an A row of the last half-chunk
    taken for the wrong block, or the next GEMM's first half-set requested wrongly, changes it."""
    from mjhmc_amd import _lib
    pair = _pair(512, 32, 'MJHMC', bias_seed=1, x_seed=3, seed=8)
    a, b = iterate_multipass_pair(pair, 1, (0.1, 1, 0.2, 1.0), monkeypatch)
    assert_multipass_pair_equal(pair, 'block-ordered half-chunk')
    assert [t[:7] for t in a] == [t[:7] for t in b]
    G = pair[0].read(_lib.F_DEDX)
    assert np.isfinite(G).all() and np.abs(G).max() > 0
    for s in pair:
        s.close()
