"""CPU: the lanes-per-particle / elements-per-lane table the group-form oracle cases (tests/test_gpu_groups_oracle.py) were
chosen from.  tests.helpers.group_shape restates pick_shape (csrc/api.hip) and jump_instance restates launch_jump_t
(csrc/launchers.hpp); if a threshold moves there, the restatement is updated with it, this table fails, and the cases
must be chosen again so that every instance is still reached."""
import pytest

from tests.helpers import group_shape, jump_instance

# (dtype, ndims): (E, lanes, the chunks fill the group, (FULLROW, WPP) of a fused MarkovJumpHMC call, of a single iteration)
TABLE = {
    ('float64', 34): (8, 8, False, (False, 0), (False, 0)),
    ('float64', 64): (8, 8, True, (True, 0), (True, 0)),
    ('float64', 100): (8, 16, False, (False, 0), (False, 0)),
    ('float64', 128): (8, 16, True, (True, 0), (True, 0)),
    ('float64', 253): (8, 32, False, (False, 0), (False, 0)),
    ('float64', 255): (8, 32, True, (True, 6), (True, 0)),      # odd: one padding element inside the last chunk
    ('float64', 256): (8, 32, True, (True, 6), (True, 0)),
    ('float64', 300): (8, 64, False, (False, 0), (False, 0)),
    ('float64', 512): (8, 64, True, (True, 5), (True, 1)),
    ('float64', 513): (16, 64, False, (False, 0), (False, 0)),
    ('float64', 1021): (16, 64, False, (False, 0), (False, 0)),
    ('float64', 1023): (16, 64, True, (True, 5), (True, 1)),    # odd
    ('float64', 1024): (16, 64, True, (True, 5), (True, 1)),
    ('float32', 64): (16, 4, True, (True, 3), (True, 3)),
    ('float32', 100): (16, 8, False, (False, 0), (False, 0)),
    ('float32', 1024): (16, 64, True, (True, 5), (True, 1)),
    ('float32', 1025): (32, 64, False, (False, 0), (False, 0)),
    ('float32', 2048): (32, 64, True, (True, 5), (True, 1)),
}


@pytest.mark.parametrize('dtype,D', sorted(TABLE))
def test_group_shape_table(dtype, D):
    E, lanes, full, fused, single = TABLE[(dtype, D)]
    got = group_shape(D, dtype)
    assert got == (E, lanes.bit_length() - 1, full), (dtype, D, got)
    assert jump_instance(*got, fused=True) == fused and jump_instance(*got, fused=False) == single
    assert jump_instance(*got, fused=True, block_decide=False) == single
    assert jump_instance(*got, fused=True, mode='control') == (False, 0) == jump_instance(*got, fused=False, mode='ct')


def test_group_shape_thresholds():
    """the neighbours of every threshold of pick_shape, and the cases' dimensions are the ones the GPU module runs"""
    from tests import test_gpu_groups_oracle as G
    assert [group_shape(D) for D in (2, 3, 8, 9, 32, 33)] == [(2, 0, True), (8, 0, False), (8, 0, True), (8, 1, False),
                                                              (8, 2, True), (8, 3, False)]
    assert group_shape(1025) == (0, 0, False) and group_shape(2049, 'float32') == (0, 0, False)   # the multi-pass path
    assert group_shape(4, 'float32') == (4, 0, True) and group_shape(5, 'float32') == (16, 0, False)
    dims = set(G.F64_DIMS + G.ODD_RAGGED)
    assert dims == {D for dt, D in TABLE if dt == 'float64'} and set(G.F32_DIMS) == {D for dt, D in TABLE if dt == 'float32'}
    for name, D in G.FUSED + G.SINGLE + G.LONG:
        assert D in dims
    assert all(G._n(D, dt) == (70 if TABLE[(dt, D)][1] == 64 else 130) for dt, D in TABLE)
