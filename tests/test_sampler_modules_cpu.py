"""The four modules of mjhmc_amd.samplers behind the sampler classes: what markov_jump_hmc.py still exports, what results.py
may import, and the public methods of the samplers with their signatures.  No library, no device."""
import ast
import inspect
import os
import sys

import pytest

from mjhmc_amd.samplers import markov_jump_hmc, recorded, requests, results

# every public name of markov_jump_hmc.py before it was split, and the module that holds it now (None: it stayed, or it
# was an import of the module's own that callers could reach through it)
HOMES = {
    'AutocorrelationTimes': results, 'ControlVariateExpectations': results, 'Diagnostics': results,
    'EffectiveSamples': results, 'Expectations': results, 'Influence': results, 'JointMarginals': results,
    'Marginals': results, 'Occupancy': results, 'Paths': results, 'PointwiseStatistics': results,
    'SteinDiscrepancy': results, 'Temperature': results, 'Waic': results, 'merge_log_sum_exp': results,
    'EnergyObservables': requests, 'Functionals': requests, 'Projections': requests, 'group_pointwise_request': requests,
    'influence_request': requests, 'pointwise_request': requests, 'refuse_grouped': requests, 'refuse_wide': requests,
    'ContinuousTimeHMC': None, 'ControlHMC': None, 'HMC': None, 'HMCBase': None, 'MarkovJumpHMC': None,
    'MAX_RETRY_DEPTH': None, 'DeviceHMCState': None, 'Distribution': None, 'HMCState': None, 'engine': None, 'np': None,
    'print_function': None,
}

STATISTICS = {
    'cv_expectations': '(self, n_iter, of=None, block=None, shift=None)',
    'diagnostics': '(self, n_iter, split=True, block=None, shift=None, of=None)',
    'energy_observables': '(self)',
    'expectations': '(self, n_iter, cov=False, block=None, shift=None, of=None)',
    'functionals': '(self, values, stats=(), params=(), names=None)',
    'group_pointwise': '(self, n_iter, values=None, log_mean_exp=None, per=None, block=None)',
    'group_waic': '(self, n_iter, block=None)',
    'influence': '(self, n_iter, value=None, experts=None, block=None, shift=None)',
    'joint_marginals': '(self, n_iter, pairs, bins=64, range=None, block=None, span=8.0, of=None)',
    'marginals': '(self, n_iter, bins=256, range=None, block=None, span=8.0, of=None)',
    'occupancy': '(self, n_iter, centres, radius=None, of=None, block=None)',
    'paths': '(self, n_iter, n_grid=None, dt=None, block=None)',
    'pointwise': '(self, n_iter, values=None, log_mean_exp=None, block=None)',
    'projections': '(self, A, b=None, link=None, params=(), names=None)',
    'stein_discrepancy': '(self, n_iter, every=1, particles=None, c=None, block=None)',
    'temperature': '(self, n_iter, split=True, block=None)',
    'waic': '(self, n_iter, block=None)',
}
BASE = dict(STATISTICS, **{
    'E': '(self, X)',
    'burn_in': '(self)',
    'dEdX': '(self, X)',
    'eval_trace': '(self, n_last)',
    'gather_root': None,                                   # (a class attribute, not a method)
    'leap_prob': '(self, Z1, Z2)',
    'load_state': '(self, path)',
    'sample': '(self, n_samples=1000, preserve_order=False, replay=None, out=None)',
    'sampling_iteration': '(self, replay=None)',
    'save_state': '(self, path)',
    'state': 'property',
})
JUMP = dict(BASE, **{
    'sample': '(self, n_samples=1000, preserve_order=False, num_steps=None, replay=None, out=None)',
    'transition_rates': '(self, Z1, Z2)',
})
PUBLIC = {'HMCBase': BASE, 'ContinuousTimeHMC': JUMP, 'MarkovJumpHMC': JUMP}


def test_every_name_the_module_exported_is_still_there_as_the_object_of_its_new_home():
    assert len(HOMES) == 35
    for name, home in sorted(HOMES.items()):
        assert hasattr(markov_jump_hmc, name), name
        if home is not None:
            assert getattr(markov_jump_hmc, name) is getattr(home, name), name
            assert getattr(home, name).__module__ == home.__name__, name
    assert markov_jump_hmc.HMCBase._RecordedRun is recorded.RecordedRun
    assert issubclass(markov_jump_hmc.HMCBase, recorded.RecordedStatistics)


def _imports(path):
    """(top-level module name, relative level, the function it sits in or None) of every import statement of a file"""
    with open(path) as f:
        tree = ast.parse(f.read())
    found = []

    def walk(node, inside):
        for child in ast.iter_child_nodes(node):
            if isinstance(child, ast.Import):
                found.extend((a.name.split('.')[0], 0, inside) for a in child.names)
            elif isinstance(child, ast.ImportFrom):
                found.append(((child.module or '').split('.')[0], child.level, inside))
            elif isinstance(child, (ast.FunctionDef, ast.ClassDef)):
                walk(child, child.name if inside is None else inside + '.' + child.name)
            else:
                walk(child, inside)
    walk(tree, None)
    return found


def test_results_imports_numpy_and_the_standard_library_only():
    """by the file's syntax tree: importing the package pulls in everything else, so an import would prove nothing.  One
    exception, stated here: ``Paths.iat`` takes misc.autocor's window rule when it is called, not when the module loads"""
    stdlib = getattr(sys, 'stdlib_module_names', None) or {'fractions'}
    outside = []
    for name, level, inside in _imports(os.path.abspath(results.__file__.replace('.pyc', '.py'))):
        if level == 0 and (name in ('numpy', '__future__') or name in stdlib):
            continue
        outside.append((name, level, inside))
    assert outside == [('misc', 2, 'Paths.iat')]


@pytest.mark.parametrize('cls', sorted(PUBLIC))
def test_public_methods_and_signatures_of_the_samplers(cls):
    c = getattr(markov_jump_hmc, cls)
    table = PUBLIC[cls]
    assert sorted(a for a in dir(c) if not a.startswith('_')) == sorted(table)
    for name, want in sorted(table.items()):
        v = inspect.getattr_static(c, name)
        if want == 'property':
            assert isinstance(v, property), name
        elif want is None:
            assert not callable(v), name
        else:
            assert str(inspect.signature(v)) == want, name
    for name in STATISTICS:                                # the statistics come from the mixin, and from nowhere else
        assert inspect.getattr_static(c, name) is recorded.RecordedStatistics.__dict__[name], name
