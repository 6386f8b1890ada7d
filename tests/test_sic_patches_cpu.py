"""CPU: what the SparseImageCode patch-count cases (tests/test_gpu_sic_patches.py) rest on, recomputed with the oracle alone.
tests.helpers.sic_tile_layout restates how the tile kernels cut a 32-column tile (sic_particles_per_tile in
csrc/dense_sic.hpp, col_of and kYLds in csrc/dense_sic.hip); if kP, kYLds or col_of changes there, the restatement is
updated with it, this table fails, and the patch counts must be chosen again so that every edge is still reached.  For
every sampler case of the GPU module: the oracle's own run at the chosen step size makes the tallies of its table, stays
finite and meets the step-size rule (at least two each of L, F and R and an R before the last iteration), and no smaller
step size of the grid does; the float32- and the float64-accumulating restatements decide differently (MarkovJumpHMC:
the transition; ControlHMC: the accept; ContinuousTimeHMC: the first clock) on at most tie_ceiling(N) particles of any
compared iteration; the float32 spread is the recorded one, and every allowance in WIDER is max(bar, 4 x spread)."""
import numpy as np
import pytest

from oracle import mjhmc_oracle as orc
from tests import test_gpu_sic_patches as S
from tests.helpers import bits_equal, load, sic_tile_layout, sic_tiles, tie_ceiling, to_bf16

# n_patches: (ppt, working columns, idle columns, patches in LDS)
LAYOUT = {1: (32, 32, 0, True), 2: (16, 32, 0, True), 3: (10, 30, 2, True), 4: (8, 32, 0, True), 5: (6, 30, 2, False),
          8: (4, 32, 0, False), 9: (3, 27, 5, False), 10: (3, 30, 2, False), 11: (2, 22, 10, False), 16: (2, 32, 0, False),
          17: (1, 17, 15, False), 31: (1, 31, 1, False), 32: (1, 32, 0, False)}


@pytest.mark.parametrize('P', sorted(LAYOUT))
def test_tile_layout_table(P):
    ppt, cpt, idle, lds = LAYOUT[P]
    assert sic_tile_layout(P) == (ppt, cpt, idle, lds)
    assert cpt == ppt * P and cpt + idle == 32 and ppt * P <= 32 < (ppt + 1) * P


def test_tile_layout_thresholds_and_tiles():
    assert [sic_tile_layout(P)[0] for P in range(1, 33)] == [32, 16, 10, 8, 6, 5, 4, 4] + [3] * 2 + [2] * 6 + [1] * 16
    assert [sic_tile_layout(P)[3] for P in range(1, 33)] == [True] * 4 + [False] * 28
    for P in (0, 33):
        with pytest.raises(ValueError):
            sic_tile_layout(P)
    with pytest.raises(ValueError):
        sic_tiles(1, 0)
    assert sic_tiles(1, 70) == (3, 6) and sic_tiles(5, 13) == (3, 1) and sic_tiles(5, 12) == (2, 6)
    assert sic_tiles(17, 5) == (5, 1) and sic_tiles(32, 1) == (1, 1) and sic_tiles(9, 7) == (3, 1) and sic_tiles(3, 10) == (1, 10)


def test_coverage_of_the_patch_counts():
    Ps = set(S.PATCHES)
    assert Ps == set(LAYOUT) == {1, 2, 3, 4, 5, 8, 9, 10, 11, 16, 17, 31, 32} and len(S.PATCHES) == 13
    lds = {P for P in range(1, 33) if sic_tile_layout(P)[3]}
    assert max(lds) in Ps and max(lds) + 1 in Ps                                   # both sides of kYLds
    two = max(P for P in range(1, 33) if sic_tile_layout(P)[0] == 2)
    assert two in Ps and two + 1 in Ps and sic_tile_layout(two + 1)[0] == 1          # both sides of ppt 2 -> 1
    assert {P for P in range(1, 33) if sic_tile_layout(P)[2] == 0} <= Ps            # every exact fill of the tile
    most = max(sic_tile_layout(P)[2] for P in range(1, 33))
    assert any(sic_tile_layout(P)[2] == most for P in Ps)                           # the largest idle count
    assert any(sic_tile_layout(P)[2] == 1 for P in Ps)
    # the batches: three tiles with a ragged last one of one particle, or one of the listed counts
    for P in Ps:
        ppt, N = sic_tile_layout(P)[0], S.N_OF[P]
        assert N == 2 * ppt + 1 or (P, N) in {(1, 70), (3, 10), (9, 7), (17, 5), (31, 4), (32, 4)}, (P, N)
        assert P * N <= 140
    assert S.N_OF[1] == 70 and [S.N_OF[P] for P in (2, 4, 5, 8, 10, 11, 16, 17)] == [33, 17, 13, 9, 7, 5, 5, 5]
    batches = ({(k[1], k[2]) for k in S.MJ_CASES + S.CONTROL_CASES + [S.CT_CASE]} |
               {(P, N) for P in Ps for N in S.eval_batches(P)})
    for P, N in batches:
        tiles, last = sic_tiles(P, N)
        assert (last < sic_tile_layout(P)[0]) != ((P, N) in S.EXACT_FILL), (P, N, 'neither ragged nor listed as an exact fill')
    assert {(P, 1) for P in Ps} <= batches and {(P, 2 * sic_tile_layout(P)[0]) for P in (4, 5, 17, 32)} <= batches


def test_the_sub_tables():
    assert S.ATOMS_512 == (1, 4, 5, 16, 17, 32) and S.FLOAT32 == (1, 4, 5, 17, 32) and S.LAPLACE == (1, 5)
    assert S.SHORT == (1, 5, 17) and S.SMALL_BATCH == (5, 17) and S.FUSED == (5, 17, 32) and S.REPLAY == (5, 17)
    assert S.CONTROL == ((5, 'bfloat16'), (17, 'bfloat16'), (32, 'bfloat16'), (5, 'float32'))
    assert S.LEAP == ((5, 1024), (17, 1024), (32, 1024), (5, 512))
    cases = S.MJ_CASES + S.CONTROL_CASES + [S.CT_CASE]
    assert len(set(cases)) == len(cases) and set(cases) == set(S.TABLE)
    mj = set(S.MJ_CASES)
    assert all(S.case('mj', P) in mj for P in S.PATCHES)
    assert all(S.case('mj', P, nc=512) in mj for P in S.ATOMS_512)
    assert all(S.case('mj', P, state='float32') in mj for P in S.FLOAT32)
    assert all(S.case('mj', P, cauchy=False) in mj for P in S.LAPLACE)
    assert all(S.case('mj', P, L=L, nc=nc) in mj for P in S.SHORT for L in (1, 2) for nc in (1024, 512))
    assert all(S.case('mj', P, N=N) in mj for P in S.SMALL_BATCH for N in (1, 2 * sic_tile_layout(P)[0]))
    assert len(mj) == 13 + 6 + 5 + 2 + 12 + 4
    assert all(eps in S.EPS_GRID for eps in S.EPS.values())
    assert all(S.case('mj', P, nc=nc) in mj for P, nc in S.LEAP) and all(S.case('mj', P) in mj for P in S.REPLAY)


def test_control_seed_opens_the_refresh_gate_early():
    """CONTROL_SEED is the first seed from 47 up whose batch-wide refresh gate (one uniform per tick, below p_r) opens within
    the first two iterations"""
    p_r = -np.log(1 - S.BETAS['control']) * 0.5

    def opens(seed):
        rng = orc.PhiloxRNG(seed, np.arange(2))
        u = []
        for _ in range(2):
            u.append(rng.uniform())
            rng.next_attempt()
        return min(u) < p_r
    assert S.SEEDS['control'] == S.CONTROL_SEED and opens(S.CONTROL_SEED)
    assert not any(opens(seed) for seed in range(47, S.CONTROL_SEED))


def _same_spread(got, recorded):
    """the recorded figure is the measured one to its two digits"""
    return np.allclose(got, recorded, rtol=0.05, atol=0)


ALL_CASES = S.MJ_CASES + S.CONTROL_CASES + [S.CT_CASE]


@pytest.mark.parametrize('key', ALL_CASES, ids=[k[0] + '-' + i for k, i in zip(ALL_CASES, S._ids(ALL_CASES))])
def test_case_on_the_oracle_alone(key):
    """the recorded tallies, the step-size rule (`choose_eps` again: no smaller step size of the grid meets it), a finite run,
    the recorded spread, and the near ties of the inputs themselves"""
    N = key[2]
    eps, run0 = S.choose_eps(key)
    assert eps == S.EPS[key], (key, 'the smallest step size of the grid that meets the rule', eps)
    run = S.oracle_run(key, eps, True)
    assert run['finite'] and S.rule_ok(run), (key, run['counts'])
    assert run['counts'] == run0['counts'] == S.TALLIES[key], (key, 'the table no longer holds the tallies of the oracle run', run['counts'])
    l, f, r, fl = run['counts']
    assert min(l + fl, f, r) >= 2 and run['early_r']
    if key[0] == 'mj':
        assert l + f + r == N * run['n_iter'] and fl == 0
    assert len(run['ties']) == run['n_iter'] and max(run['ties']) <= tie_ceiling(N), (key, 'near ties of the inputs', run['ties'])
    assert _same_spread(run['spread'], S.SPREAD[key]), (key, 'spread', run['spread'], S.SPREAD[key])


def test_wider_follows_the_rule():
    """WIDER holds exactly the cases where MARGIN x the recorded spread exceeds a bar (delta_rel, e_rtol; x_tol is the bar
    everywhere), at max(bar, MARGIN x spread)"""
    want = {key: S.allowance(spread) for key, spread in S.SPREAD.items() if S.allowance(spread) != S.BARS}
    assert set(S.WIDER) == set(want)
    for key, (allowed, spread) in S.WIDER.items():
        assert spread == S.SPREAD[key] and np.allclose(allowed, want[key], rtol=1e-12, atol=0), (key, allowed, want[key])
        assert all(a >= b for a, b in zip(allowed, S.BARS)) and allowed[1] == S.BARS[1]
    assert S.MARGIN == 4.0 and S.BARS == (5e-4, 1.0 / 128, 5e-4)


def test_accumulate_dtype_default_is_bit_for_bit_and_float32_is_close():
    """accumulate_dtype: the default reproduces E_val / dEdX_val bit for bit (the formulas of the restatement written out
    here, and the golden fixture at full precision); float32 accumulation stays within float32 rounding of it and differs"""
    g = load('g2_dense')
    tag, P = 'sic_p9_n4_cauchy', 9
    X = g[tag + '_X']
    B, imgs, _ = S._problem(P, 1024)
    Y = imgs[:, :P].T
    plain = orc.SparseImageCode(B, Y, lmbda=0.01, cauchy=True)
    assert S.rel(plain.E_val(X)[0], g[tag + '_E']) < 1e-9 and S.rel(plain.dEdX_val(X), g[tag + '_g']) < 1e-9
    assert bits_equal(plain.E_val(X), orc.SparseImageCode(B, Y, lmbda=0.01, cauchy=True, accumulate_dtype=np.float64).E_val(X))
    for cauchy in (True, False):
        e64 = orc.SparseImageCode(B, Y, lmbda=0.01, cauchy=cauchy, operand_rounding=to_bf16)
        e32 = orc.SparseImageCode(B, Y, lmbda=0.01, cauchy=cauchy, operand_rounding=to_bf16, accumulate_dtype=np.float32)
        Xb = to_bf16(X)
        # the restatement as it was before the argument existed
        Bb = to_bf16(B)
        R = np.einsum('ic,pcn->pin', Bb, to_bf16(Xb).reshape(P, 1024, -1)) - Y[:, :, None]
        pen = np.sum(np.log(1 + Xb ** 2), axis=0) if cauchy else np.sum(np.abs(Xb), axis=0)
        E = (np.mean(np.sum(0.5 * R ** 2, axis=1), axis=0) + 0.01 * pen).reshape((1, -1))
        G = (np.einsum('ic,pin->pcn', Bb, to_bf16(R / P)).reshape(Xb.shape) +
             0.01 * (2 * Xb / (1 + Xb ** 2) if cauchy else np.sign(Xb)))
        assert bits_equal(e64.E_val(Xb), E) and bits_equal(e64.dEdX_val(Xb), G)
        eE, eG = S.rel(e32.E_val(Xb), E), S.rel(e32.dEdX_val(Xb), G)
        # float32 sums of 256 / 1024 products of O(1) terms: well inside the device bars, and not the float64 values.  A
        # gradient element whose scaled residual rounds to the other bf16 neighbour moves by 2^-9 of one product of 256
        assert 0 < eE < 2e-6 and 0 < eG < 2e-4, (cauchy, eE, eG)
    with pytest.raises(ValueError):
        orc.SparseImageCode(B, Y, accumulate_dtype=np.float16)
