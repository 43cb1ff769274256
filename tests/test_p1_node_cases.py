"""
The case list of the P1 node route's per-entry test reaches the plan forms it claims (CPU only): every mesh of
tests/p1_node_cases.py through the host plan builder (fep_host::build_p1_plan in a plain build of tests/host_san.cpp, its
`plan` mode), against the same table test_p1_node_route_gpu.py checks the library's plan line with.  Every plan is validated
against its mesh by fep_host::validate_p1_plan on the way.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import p1_node_cases as cases
from conftest import ROOT

SRC = os.path.join(ROOT, 'tests', 'host_san.cpp')


@pytest.fixture(scope='module')
def harness(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.skip('g++ not available')
    exe = str(tmp_path_factory.mktemp('plan') / 'host_plan')
    res = subprocess.run(['g++', '-std=c++17', '-O2', '-pthread', '-o', exe, SRC], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         text=True)
    assert res.returncode == 0, res.stdout[-3000:]
    return exe


def _plan(harness, tmp_path, name):
    elem, coord, _ = cases.mesh(name)
    path = str(tmp_path / f'{name}.bin')
    elem = np.ascontiguousarray(elem, dtype=np.int32)
    with open(path, 'wb') as f:
        np.array([3, elem.shape[1], coord.shape[1]], dtype=np.int32).tofile(f)
        elem.tofile(f)
    res = subprocess.run([harness, path, '2', 'plan'], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert res.returncode == 0 and 'result ok' in res.stdout, (name, res.stdout[-3000:])
    return cases.parse_host(res.stdout)


@pytest.mark.parametrize('name', list(cases.CASES) + [cases.BENCH[0]])
def test_case_reaches_its_plan_form(harness, tmp_path, name):
    want = cases.BENCH[2] if name == cases.BENCH[0] else cases.CASES[name][1]
    got = _plan(harness, tmp_path, name)
    print(f'[plan] {name}: {got}')
    cases.check_form(name, got, want)


def test_every_plan_form_has_a_case_and_every_state():
    """Each combination of (segments, element lists as runs, node lists as runs) the default plan can come out as is met
    with per-point materials (wide), constant materials, an initial strain (tsx) and an accepting step; and the sizes the
    issue names are in the table: one staged node per lane, a list longer than 200, one tile, the benchmark's form."""
    by_form = {}
    for name, (state, form) in cases.CASES.items():
        if form is None or 'segs' not in form:
            continue
        by_form.setdefault((form['segs'], form['rng'], form['fused_rng']), set()).add(state)
    assert set(by_form) == {(1, 1, 1), (2, 1, 1), (1, 0, 0), (2, 0, 0), (1, 1, 0)}
    for form, states in by_form.items():
        assert {'wide', 'tsx', 'accept'} <= states, (form, states)        # tsx and accept run on constant materials
    forms = [f for _, f in cases.CASES.values() if f]
    assert any(f.get('NL') == 256 and f.get('L', (0,))[0] > 200 for f in forms)
    assert any(f.get('last', (0,))[0] == 256 for f in forms) and any(f.get('last', (0, 0))[1] == 1 for f in forms)
    assert cases.BENCH[2]['segs'] == 2 and cases.BENCH[2]['rng'] == 1


def test_the_dropped_element_is_the_last_tiles_own(harness, tmp_path):
    """rect17x12-1: the dropped element is the last node's only one and the last tile owns it: that tile loses the node,
    its block row and the blocks its two neighbours had with it (5 blocks), and one owned element."""
    a, b = _plan(harness, tmp_path, 'rect17x12'), _plan(harness, tmp_path, 'rect17x12-1')
    assert a['last'][0] == 256 and a['last'][0] - b['last'][0] == 5 and a['last'][1] - b['last'][1] == 1
    assert a['last'][2] - b['last'][2] == 1


def test_mixed_orientation_case_has_reversed_elements():
    from elem_ref import ElemRef
    from meshes import fep
    elem, coord, _ = cases.mesh('mixed24')
    assert (ElemRef(elem, coord, fep.element_tables('P1')).det() < 0).mean() > 0.3
