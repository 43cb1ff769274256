"""
The step plan (fem-elastoplasticity_amd/csrc/fep_step_plan.h) on the CPU: tests/step_plan_host.cpp plans every StepFacts x
StepWants and checks what every step must satisfy (one writer per wanted output, operands for every assembly, one counter sum
over the grid that counted, no one-kernel step that accepts, the shape of staged steps and of fep_assemble_dev, preallocated
scratch for every step that may run in a stream capture), then compares the plan's stage list with the launches the profiler
recorded for tools/step_trace.py's matrix (tests/golden/step_launches.json).  The runner, the scratch allocator and
fep_ctx_kernel_names read this same plan_step.  No GPU.
"""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT
from step_launches import ROUTE_ID, golden_cases, no_open_contexts

SRC = os.path.join(ROOT, 'tests', 'step_plan_host.cpp')

@pytest.fixture(scope='module')
def harness(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.skip('g++ not available')
    exe = str(tmp_path_factory.mktemp('step_plan') / 'step_plan_host')
    res = subprocess.run(['g++', '-std=c++17', '-O2', '-o', exe, SRC], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-3000:]
    return exe


def test_every_plan_holds_its_invariants_and_equals_the_recorded_launches(harness, tmp_path):
    cases = golden_cases()
    assert len(cases) == 2 * 3 * 5 * (2 * 2 * 5 * 2 + 3)
    no_open = no_open_contexts(cases)
    assert no_open == {('Q1-4', 'default'), ('Q1-4', 'patch')}, no_open       # 16 elements, one patch of up to 64
    path = tmp_path / 'cases.txt'
    with open(path, 'w') as f:
        for label, ctx, route, dp, w, stages in cases:
            f.write(f'{ROUTE_ID[route]} {dp} {int(ctx in no_open)} ' + ' '.join(str(v) for v in w.values()) + ' ' + ' '.join(stages) + '\n')
    res = subprocess.run([harness, str(path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(res.stdout)
    assert res.returncode == 0 and 'result ok' in res.stdout and 'FAILED' not in res.stdout, res.stdout[-3000:]
    assert f'golden: {len(cases)} recorded cases compared' in res.stdout, res.stdout
    assert 'plans: ' in res.stdout
