"""The launch schedule of an mjhmc_iterate call (csrc/schedule.hpp: select_schedule) against a table written down by hand
from the predicates the schedules had when they were one function.  The A/B equality tests on the GPU (test_gpu_fused.py,
test_gpu_dense_parity.py, test_gpu_rows_oracle.py) flip a switch and compare two samplers bit for bit: a predicate that
silently changed would make them compare a schedule with itself, and pass.  The table holds every parametrisation of those
tests with and without the switch, and the boundaries of every predicate.

tests/schedule_table.cpp is compiled with the host compiler that ships with ROCm (no HIP, no GPU) and prints the schedule
of every row."""
import os
import subprocess

import pytest

from tests.helpers import group_shape

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = '/opt/rocm/lib/llvm/bin/clang++'
K_FUSE_BELOW = 160000        # csrc/schedule.hpp: kFuseBelow (test_the_threshold_is_the_one_the_table_assumes)
MM_RELAY_MIN_L = 4           # csrc/energies.hpp: MMGaussF::kRelayMinL


def row(kind, D, N, n_iter, L=6, mode='mjhmc', replay=False, no_fuse=False, no_compact=False, fuse_below=None,
        pot64_multipass=False):
    """the ScheduleInputs mjhmc_iterate fills (iterate.hip: schedule_inputs) for a float64 sampler of `kind`, as a line of
    schedule_table.cpp's input.  kind: an elementwise energy's name, 'user', or a dense one -- 'pot' (float32 state),
    'pot64' (float64 state: Shape::wide, the tile kernel), 'pot_big' (float64, beyond the tile kernels), 'sic'."""
    wide = tile = False
    logG = 0
    if kind in ('pot', 'sic'):
        family = 'dense'
    elif kind in ('pot64', 'pot_big'):
        family, wide, tile = 'dense', True, kind == 'pot64'
    else:
        E, logG, _ = group_shape(D)
        wide = E == 0                       # more than 64 lanes x 16 elements: the multi-pass path
        if kind == 'user':
            family = 'user'
        elif kind in ('E_ISO_GAUSS', 'E_DIAG_GAUSS'):
            family = 'gaussian'
        elif (kind in ('E_FUNNEL_NEAL', 'E_FUNNEL_REF', 'E_MM_GAUSS') and E == 8 and mode == 'mjhmc' and logG in (1, 2)
              and not (kind == 'E_MM_GAUSS' and L < MM_RELAY_MIN_L)):
            family = 'rows'                 # iterate.hip: fused_rows()
        else:
            family = 'other'
    return ' '.join(str(v) for v in (family, int(wide), int(tile), N, D, logG, int(mode == 'mjhmc'), L, n_iter, int(replay),
                                     int(no_fuse), int(no_compact), '-' if fuse_below is None else fuse_below,
                                     int(pot64_multipass)))


# (label, inputs, expected schedule).  A/B pairs carry the same label stem with "/a" and "/b"; PAIRS_THAT_MUST_DIFFER names
# the stems whose two sides the GPU test means to be different schedules.
TABLE = []
PAIRS_THAT_MUST_DIFFER = []


def pair(stem, a, b, differ=True):
    TABLE.append((stem + '/a', a[0], a[1]))
    TABLE.append((stem + '/b', b[0], b[1]))
    if differ:
        assert a[1] != b[1], stem
        PAIRS_THAT_MUST_DIFFER.append(stem)


# test_gpu_fused.py::test_fused_equals_single_iterations: a runs n_iter (and then 3) iterations in one call, b one per call;
# L = 6.  b's schedule: the compacted passes from 16384 MarkovJumpHMC particles up (below a wave per particle), else plain.
for kind, D, N, mode, n_iter, single in [
        ('E_ISO_GAUSS', 512, 130, 'mjhmc', 7, 'Plain'), ('E_ISO_GAUSS', 256, 131, 'mjhmc', 9, 'Plain'),
        ('E_DIAG_GAUSS', 256, 64, 'mjhmc', 66, 'Plain'), ('E_ISO_GAUSS', 64, 500, 'mjhmc', 70, 'Plain'),
        ('E_ISO_GAUSS', 40, 129, 'mjhmc', 5, 'Plain'), ('E_ISO_GAUSS', 2, 100, 'mjhmc', 9, 'Plain'),
        ('E_DIAG_GAUSS', 32, 300, 'mjhmc', 6, 'Plain'), ('E_FUNNEL_NEAL', 32, 300, 'mjhmc', 6, 'Plain'),
        ('E_FUNNEL_NEAL', 31, 20011, 'mjhmc', 5, 'Compact'), ('E_FUNNEL_NEAL', 31, 200003, 'mjhmc', 5, 'Compact'),
        ('E_FUNNEL_NEAL', 21, 131, 'mjhmc', 70, 'Plain'), ('E_FUNNEL_NEAL', 16, 700, 'mjhmc', 9, 'Plain'),
        ('E_FUNNEL_NEAL', 11, 65, 'mjhmc', 7, 'Plain'), ('E_ROUGH_WELL', 4, 48, 'mjhmc', 8, 'Plain'),
        ('E_MM_GAUSS', 3, 40, 'mjhmc', 8, 'Plain'), ('E_MM_GAUSS', 32, 300, 'mjhmc', 6, 'Plain'),
        ('E_MM_GAUSS', 27, 20011, 'mjhmc', 5, 'Compact'), ('E_MM_GAUSS', 27, 200003, 'mjhmc', 5, 'Compact'),
        ('E_MM_GAUSS', 12, 700, 'mjhmc', 9, 'Plain'), ('E_ROUGH_WELL', 40, 200, 'control', 6, 'Plain'),
        ('E_ISO_GAUSS', 16, 200, 'control', 12, 'Plain'), ('E_ISO_GAUSS', 24, 77, 'cthmc', 12, 'Plain')]:
    stem = 'fused_equals_single[%s-%d-%d-%s-%d]' % (kind, D, N, mode, n_iter)
    pair(stem, (row(kind, D, N, n_iter, mode=mode), 'Fused'), (row(kind, D, N, 1, mode=mode), single))
    TABLE.append((stem + '/then3', row(kind, D, N, 3, mode=mode), 'Fused'))

# test_gpu_fused.py::test_compacted_inverse_pass_equals_in_kernel: MJHMC_NO_FUSE on both sides, calls of 1 and 3
# iterations, L = 7; b sets MJHMC_NO_COMPACT.  ('E_FUNNEL_NEAL', 21, 9000) lies below the 16384 particles the compacted
# passes start at: both of its sides are the plain schedule, and were before the schedules were split.
for kind, D, N in [('E_FUNNEL_NEAL', 32, 20000), ('E_ISO_GAUSS', 6, 70001), ('E_ROUGH_WELL', 40, 16400),
                   ('E_FUNNEL_NEAL', 31, 20011), ('E_FUNNEL_NEAL', 21, 9000), ('E_FUNNEL_REF', 16, 40001),
                   ('E_FUNNEL_REF', 11, 33000), ('E_FUNNEL_NEAL', 9, 16385)]:
    for n in (1, 3):
        compacts = N >= 16384
        pair('compacted_equals_in_kernel[%s-%d-%d]x%d' % (kind, D, N, n),
             (row(kind, D, N, n, L=7, no_fuse=True), 'Compact' if compacts else 'Plain'),
             (row(kind, D, N, n, L=7, no_fuse=True, no_compact=True), 'Plain'), differ=compacts)

# test_gpu_fused.py::test_list_carried_between_calls_equals_a_scan_per_call: MJHMC_NO_FUSE, calls of 1, 2 and 3 iterations,
# L = 7 and 5.  Its switch (MJHMC_NO_LIST_CARRY) is no input of the choice: BOTH sides must be the compacted passes.  The
# "fused call in between" is 4 iterations without MJHMC_NO_FUSE.
for kind, D, N in [('E_FUNNEL_NEAL', 32, 20000), ('E_FUNNEL_NEAL', 21, 20011), ('E_ROUGH_WELL', 40, 16400)]:
    for n in (1, 2, 3):
        for L in (7, 5):
            TABLE.append(('list_carried[%s-%d-%d]x%d,L%d' % (kind, D, N, n, L), row(kind, D, N, n, L=L, no_fuse=True), 'Compact'))
    TABLE.append(('list_carried[%s-%d-%d]fused call' % (kind, D, N), row(kind, D, N, 4, L=5), 'Fused'))

# test_gpu_fused.py::test_compacted_passes_failure_in_the_middle_of_a_batch: a Gaussian with MJHMC_NO_FUSE, 12 iterations at
# L = 5, then 3 at L = 10; b sets MJHMC_NO_COMPACT
for n, L in ((12, 5), (3, 10)):
    pair('compacted_failure_in_the_middle x%d' % n, (row('E_ISO_GAUSS', 24, 20000, n, L=L, no_fuse=True), 'Compact'),
         (row('E_ISO_GAUSS', 24, 20000, n, L=L, no_fuse=True, no_compact=True), 'Plain'))

# test_gpu_rows_oracle.py::_path: `fused` is a call of several iterations against one per call; the row form (9 <= D <= 32,
# the mixture from L = 4) is a fused launch at EVERY batch size, the group form only below kFuseBelow particles
for name, kind in (('neal', 'E_FUNNEL_NEAL'), ('literal', 'E_FUNNEL_REF'), ('mm3', 'E_MM_GAUSS')):
    for D in (8, 9, 13, 16, 17, 21, 27, 31, 32, 33):
        for L in (3, 4, 12):
            rows = 9 <= D <= 32 and not (kind == 'E_MM_GAUSS' and L < 4)
            stem = 'rows_oracle_path[%s-%d-L%d]' % (name, D, L)
            pair(stem + 'N1000', (row(kind, D, 1000, 8, L=L), 'Fused'), (row(kind, D, 1000, 1, L=L), 'Plain'))
            pair(stem + 'N200003', (row(kind, D, 200003, 8, L=L), 'Fused' if rows else 'Compact'),
                 (row(kind, D, 200003, 1, L=L), 'Compact'), differ=rows)

# test_gpu_dense_parity.py / test_gpu_pot64_staged_rows.py: MJHMC_POT64_MULTIPASS against the float64 tile kernel
for n in (1, 5):
    pair('pot64_multipass x%d' % n, (row('pot64', 100, 5000, n, L=3), 'DenseParts'),
         (row('pot64', 100, 5000, n, L=3, pot64_multipass=True), 'Multipass'))

# the boundaries of every predicate
TABLE += [
    ('n_iter 1', row('E_ISO_GAUSS', 64, 500, 1), 'Plain'),
    ('n_iter 2', row('E_ISO_GAUSS', 64, 500, 2), 'Fused'),
    ('N = kFuseBelow - 1', row('E_ROUGH_WELL', 40, K_FUSE_BELOW - 1, 2), 'Fused'),
    ('N = kFuseBelow', row('E_ROUGH_WELL', 40, K_FUSE_BELOW, 2), 'Compact'),
    ('N = kFuseBelow, Gaussian', row('E_DIAG_GAUSS', 40, K_FUSE_BELOW, 2), 'Fused'),
    ('N = 16383', row('E_ROUGH_WELL', 40, 16383, 1), 'Plain'),
    ('N = 16384', row('E_ROUGH_WELL', 40, 16384, 1), 'Compact'),
    ('D = 4', row('E_ROUGH_WELL', 4, 200000, 2), 'Fused'),
    ('D = 5', row('E_ROUGH_WELL', 5, 200000, 2), 'Compact'),
    ('logG = 5', row('E_ROUGH_WELL', 256, 200000, 1), 'Compact'),
    ('logG = 6', row('E_ROUGH_WELL', 257, 200000, 1), 'Plain'),
    ('logG = 6, several iterations', row('E_ROUGH_WELL', 257, 200000, 4), 'Plain'),
    ('replay, small batch', row('E_ISO_GAUSS', 64, 500, 2, replay=True), 'Plain'),
    ('replay, big batch', row('E_ROUGH_WELL', 40, 20000, 1, replay=True), 'Plain'),
    ('replay, dense', row('pot', 100, 5000, 2, replay=True), 'DenseParts'),
    ('user expression, small', row('user', 16, 500, 4), 'Plain'),
    ('user expression, big', row('user', 16, 200000, 1), 'Plain'),
    ('CONTROL, big batch', row('E_ROUGH_WELL', 40, 20000, 1, mode='control'), 'Plain'),
    ('CONTROL, big batch, several iterations', row('E_ROUGH_WELL', 40, 200000, 4, mode='control'), 'Plain'),
    ('float64 ProductOfT, L = 0', row('pot64', 100, 5000, 3, L=0), 'Multipass'),
    ('float64 ProductOfT, L = 1', row('pot64', 100, 5000, 3, L=1), 'DenseParts'),
    ('ProductOfT beyond the tile kernels', row('pot_big', 600, 5000, 3), 'Multipass'),
    ('wide elementwise rows', row('E_ISO_GAUSS', 2049, 100, 3), 'Multipass'),
    ('float32 ProductOfT', row('pot', 100, 5000, 64), 'DenseParts'),
    ('float32 ProductOfT, one iteration, MJHMC_NO_FUSE', row('pot', 100, 5000, 1, no_fuse=True), 'DenseParts'),
    ('SparseImageCode', row('sic', 1024, 2000, 16), 'DenseParts'),
    ('MJHMC_FUSE_BELOW=0 sets the row form aside', row('E_FUNNEL_NEAL', 32, 200003, 2, fuse_below=0), 'Compact'),
    ('MJHMC_FUSE_BELOW unset: the row form fuses', row('E_FUNNEL_NEAL', 32, 200003, 2), 'Fused'),
    ('MJHMC_FUSE_BELOW=1000000', row('E_ROUGH_WELL', 40, 200000, 2, fuse_below=1000000), 'Fused'),
    ('MJHMC_FUSE_BELOW=0, D <= 4 still fuses', row('E_ROUGH_WELL', 4, 200000, 2, fuse_below=0), 'Fused'),
]


@pytest.fixture(scope='module')
def chosen(tmp_path_factory):
    assert os.path.exists(CLANG), 'the host compiler that ships with ROCm'
    exe = str(tmp_path_factory.mktemp('schedule') / 'schedule_table')
    subprocess.check_call([CLANG, '-std=c++17', '-O1', '-Wall', '-Werror', os.path.join(ROOT, 'tests', 'schedule_table.cpp'),
                           '-o', exe])
    out = subprocess.run([exe], input='\n'.join(r for _, r, _ in TABLE) + '\n', stdout=subprocess.PIPE, check=True,
                         universal_newlines=True).stdout.split()
    assert len(out) == len(TABLE)
    return dict(zip((label for label, _, _ in TABLE), out))


def test_labels_are_unique():
    labels = [label for label, _, _ in TABLE]
    assert len(set(labels)) == len(labels)


def test_schedules_match_the_table(chosen):
    wrong = [(label, want, chosen[label]) for label, _, want in TABLE if chosen[label] != want]
    assert not wrong, wrong


def test_switched_pairs_take_different_schedules(chosen):
    assert len(PAIRS_THAT_MUST_DIFFER) > 100
    same = [stem for stem in PAIRS_THAT_MUST_DIFFER if chosen[stem + '/a'] == chosen[stem + '/b']]
    assert not same, same


def test_the_threshold_is_the_one_the_table_assumes():
    import re
    hpp = open(os.path.join(ROOT, 'mjhmc_amd', 'csrc', 'schedule.hpp')).read()
    assert int(re.search(r'kFuseBelow\s*=\s*(\d+)', hpp).group(1)) == K_FUSE_BELOW
    assert '#include <hip' not in hpp and 'handles.hpp' not in hpp        # nothing of HIP: the host compiler alone builds it
    ew = open(os.path.join(ROOT, 'mjhmc_amd', 'csrc', 'energies.hpp')).read()
    assert int(re.search(r'struct MMGaussF.*?kRelayMinL\s*=\s*(\d+)', ew, flags=re.S).group(1)) == MM_RELAY_MIN_L
