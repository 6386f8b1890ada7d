"""GPU: what the four ring accumulators share (csrc/ring_source.hpp: RingAccumulator, acc_begin, acc_end, acc_destroy) --
the refusals of create and accumulate by error code and message, the state count, and the order-independent close --
for DeviceEstimator, DeviceChainStats, DeviceHistogram and DevicePairHistogram on the sampler's ring and on the derived
ring of a one-value functional.

The expected messages are written out here as the C sources word them; they are not read from the code under test."""
import numpy as np
import pytest

from tests.test_gpu_chainstats import _iso

pytestmark = pytest.mark.gpu

D, N, SLOTS = 3, 70, 3                       # Npad = 128 > N
KINDS = ('estimator', 'chainstats', 'histogram', 'pairhist')
RINGS = ('sample', 'derived')
# "... was re-allocated after mjhmc_<kind>_create: create <this>"
A_NEW = {'estimator': 'a new estimator', 'chainstats': 'a new one', 'histogram': 'a new histogram',
         'pairhist': 'a new pair histogram'}
NO_RING = {'sample': 'the sampler has no sample ring yet (call mjhmc_ring_alloc first)',
           'derived': 'the functionals have no derived ring yet (call mjhmc_functionals_ring_alloc first)'}
INVALID = -1                                 # MJHMC_ERR_INVALID


def _sampler():
    """the iso Gaussian, float64, with SLOTS recorded states"""
    s = _iso(D, N, 7)
    return s, s._dev


def _make(kind, dev, on):
    """an accumulator of ``kind`` on the sampler's ring (on = None) or on the derived ring of ``on``"""
    src = dev if on is None else on
    if kind == 'estimator':
        return src.estimator(False)
    if kind == 'chainstats':
        return src.chain_stats(1)
    if kind == 'histogram':
        return src.histogram(8, -8.0, 8.0)
    return src.pair_histogram([[0, 0]] if on is not None else [[0, 1]], 8, -8.0, 8.0)


def _n_states(kind, acc):
    if kind == 'estimator':
        return acc.read()[4]
    if kind == 'chainstats':
        n_chains, per_chain = acc.read()[:2]
        return n_chains * per_chain
    return acc.read()[3]


def _refused(call, message):
    """``call`` raises with MJHMC_ERR_INVALID and exactly ``message``"""
    from mjhmc_amd._lib import EngineError
    with pytest.raises(EngineError) as e:
        call()
    assert str(e.value) == 'libmjhmc_hip: %s (status %d)' % (message, INVALID)


@pytest.mark.parametrize('ring', RINGS)
@pytest.mark.parametrize('kind', KINDS)
def test_shared_refusals_and_state_count(kind, ring):
    s, dev = _sampler()
    fn = None
    if ring == 'sample':
        _refused(lambda: _make(kind, dev, None), NO_RING['sample'])       # create before any ring exists
        dev.ring_alloc(SLOTS)
        s._run(SLOTS, ring_slot0=0)
    else:
        dev.ring_alloc(SLOTS)
        s._run(SLOTS, ring_slot0=0)
        fn = dev.functionals(['S[0]'], ['d == 0 ? x : 0.0'])
        _refused(lambda: _make(kind, dev, fn), NO_RING['derived'])
        fn.ring_alloc(SLOTS)
        fn.evaluate(0, SLOTS, 0)
    acc = _make(kind, dev, fn)

    acc.accumulate(0, 2, w_slot0=1)                                       # a good block: n = 2 states per particle
    assert _n_states(kind, acc) == 2 * N

    _refused(lambda: acc.accumulate(0, 0), 'n must be >= 1')
    _refused(lambda: acc.accumulate(1, 3), 'state slots [1, 4) are outside the ring of 3')
    _refused(lambda: acc.accumulate(-1, 1), 'state slots [-1, 0) are outside the ring of 3')
    _refused(lambda: acc.accumulate(0, 2, w_slot0=2),
             'dwell slots [2, 4) are outside the ring of 3 (-1 asks for unit weights)')
    _refused(lambda: acc.accumulate(0, 1, w_slot0=-2),
             'dwell slots [-2, -1) are outside the ring of 3 (-1 asks for unit weights)')
    assert _n_states(kind, acc) == 2 * N                                  # a refused block adds nothing

    acc.accumulate(2, 1)                                                  # unit weights, the last slot
    assert _n_states(kind, acc) == 3 * N

    (dev if fn is None else fn).ring_alloc(SLOTS + 2)                     # a new ring: the handle was made for the old one
    _refused(lambda: acc.accumulate(0, 1), 'the %s ring was re-allocated after mjhmc_%s_create: create %s'
             % (ring, kind, A_NEW[kind]))
    assert _n_states(kind, acc) == 3 * N

    if fn is not None:                                                    # the functional first: it frees the accumulator
        fn.close()
        acc.close()
        assert acc.handle is None
    acc.close()                                                           # (and closing twice is harmless)
    dev.close()


def test_sampler_close_with_live_accumulators_on_both_rings():
    s, dev = _sampler()
    dev.ring_alloc(SLOTS)
    s._run(SLOTS, ring_slot0=0)
    fn = dev.functionals(['S[0]'], ['d == 0 ? x : 0.0'])
    fn.ring_alloc(SLOTS)
    fn.evaluate(0, SLOTS, 0)
    live = [_make(kind, dev, on) for on in (None, fn) for kind in KINDS]
    for acc in live:
        acc.accumulate(0, SLOTS)
    dev.close()                                                           # frees the functional and all eight handles
    assert dev.handle is None
    for acc in live + [fn]:
        acc.close()                                                       # nothing left to free: no call into the library
        assert acc.handle is None
