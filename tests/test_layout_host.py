"""
The one definition of the gather-table formats (fem-elastoplasticity_amd/csrc/fep_layout.h) on the CPU: tests/layout_host.cpp
puts every field of every packed word at its extreme values (unpack(pack(f)) == f, no bit outside the field, *_fits true at the
greatest value and false one past it), checks run_entry against lists expanded by hand, the LDS regions of the P1 tile
kernels (no overlap, 16-byte alignment, the total the launchers and the planner used to write out), the patch image
(injective, inside its slot count) and sym_block_index's symmetry.  The planner, the launchers and the kernels call these
same functions.  No GPU.
"""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, 'tests', 'layout_host.cpp')


@pytest.fixture(scope='module')
def harness(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.skip('g++ not available')
    exe = str(tmp_path_factory.mktemp('layout') / 'layout_host')
    res = subprocess.run(['g++', '-std=c++17', '-O2', '-o', exe, SRC], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-3000:]
    return exe


def test_every_layout_function_holds_at_its_extremes(harness):
    res = subprocess.run([harness], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(res.stdout)
    assert res.returncode == 0 and 'result ok' in res.stdout and 'FAILED' not in res.stdout, res.stdout[-3000:]
    for group in ('packed words: 11 formats', 'run_entry: 4 tables', 'p1_tile_lds: ', 'patch image: ', 'XCD order: '):
        assert group in res.stdout, (group, res.stdout)
