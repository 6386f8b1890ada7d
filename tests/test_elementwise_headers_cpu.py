"""CPU: the headers elementwise.hpp was split into.  Each compiles on its own (a one-line translation unit that includes it
alone passes hipcc's device-side syntax check), sampler_args.hpp is plain structs that host code and hipRTC can both take,
elementwise.hpp is the umbrella and nothing else, and a user expression is compiled against jump_kernel.hpp alone."""
import os
import re
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'mjhmc_amd', 'csrc')
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
HEADERS = ['sampler_args', 'lane_group', 'jump_math', 'energies', 'group_form', 'jump_process', 'jump_kernel', 'row_tile',
           'row_form', 'step_kernel', 'launcher_decls', 'launchers']


def text(name):
    return open(os.path.join(CSRC, name)).read()


@pytest.mark.parametrize('header', HEADERS)
def test_header_compiles_on_its_own(header, tmp_path):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.fail('hipcc not found: the headers cannot be checked')
    flags = subprocess.check_output(['make', '-s', 'print-flags'], cwd=CSRC, text=True).split()
    tu = tmp_path / ('only_%s.hip' % header)
    tu.write_text('#include "%s.hpp"\n' % header)
    r = subprocess.run([HIPCC] + flags + ['--cuda-device-only', '-fsyntax-only', '-I', CSRC, str(tu)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_umbrella_includes_every_piece_and_holds_nothing_else():
    lines = [l.strip() for l in text('elementwise.hpp').split('\n')]
    code = [l for l in lines if l and not l.startswith('//')]
    assert code[0] == '#pragma once'
    assert all(re.fullmatch(r'#include "\w+\.hpp"', l) for l in code[1:]), code
    assert {l.split('"')[1][:-4] for l in code[1:]} == set(HEADERS)


def test_the_argument_blocks_are_plain_structs():
    src = text('sampler_args.hpp')
    assert '__device__' not in src and '__global__' not in src and '#include <hip' not in src


def test_a_user_expression_is_compiled_against_the_jump_kernel_header_alone():
    body = text('user_expr.hip')
    body = body[body.index('std::string user_expr_source('):body.index('std::vector<std::string> user_expr_kernel_names(')]
    assert re.findall(r'#include \\"(\w+\.hpp)\\"', body) == ['jump_kernel.hpp']
