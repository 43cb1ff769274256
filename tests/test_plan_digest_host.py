"""
The planner's tables do not depend on how its work is split over threads (CPU only).  fep_host.h fills the P1 and patch
tables in parallel_chunks, worker-local pieces joined afterwards; tests/plan_digest_host.cpp prints the length and an
FNV-1a digest of every table of every plan variant, and the output with FEP_HOST_THREADS=1 must equal the output with 16,
on every mesh of tests/p1_node_cases.py and on the fans of tests/fan_mesh.py (P1, P2, P4).  No digest is pinned: the formats
may change; two builds of the planner are compared by running the same program against both.
"""
import os
import shutil
import subprocess

import pytest

import p1_node_cases as cases
from conftest import ROOT
from fan_mesh import fan_mesh
from test_host_sanitizers import FANS, _dump

SRC = os.path.join(ROOT, 'tests', 'plan_digest_host.cpp')
P1_TABLES = ('tdesc', 'rec', 'perm2', 'elist_pad', 'rng_tab', 'nlist_pad', 'nrng_tab', 'codes_pad', 'pkv', 'elnodes')
PATCH_TABLES = ('pdesc', 'plist', 'pel', 'pnodes', 'items', 'fitems', 'codes', 'fcodes', 'fix', 'ffix', 'fixT')


@pytest.fixture(scope='module')
def harness(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.skip('g++ not available')
    exe = str(tmp_path_factory.mktemp('digest') / 'plan_digest_host')
    res = subprocess.run(['g++', '-std=c++17', '-O2', '-pthread', '-o', exe, SRC], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         text=True)
    assert res.returncode == 0, res.stdout[-3000:]
    return exe


def _digest(harness, path, threads):
    res = subprocess.run([harness, path], env=dict(os.environ, FEP_HOST_THREADS=str(threads)), stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-3000:]
    return res.stdout.splitlines()


def _same_for_every_split(harness, path, n_p):
    one, many = _digest(harness, path, 1), _digest(harness, path, 16)
    assert one == many, [(a, b) for a, b in zip(one, many) if a != b][:10]
    # every table of every variant is there: 6 P1 plans (P1 meshes), 3 patch sizes x 4 groupings
    tables = [l.split()[:2] for l in one if ' scalars ' not in l]
    if n_p == 3:
        assert sum(1 for p, _ in tables if p.startswith('p1[')) == 6 * len(P1_TABLES), one
        assert {t for p, t in tables if p.startswith('p1[')} == set(P1_TABLES)
    assert sum(1 for p, _ in tables if p.startswith('patch[')) == 12 * len(PATCH_TABLES), one
    assert {t for p, t in tables if p.startswith('patch[')} == set(PATCH_TABLES)
    return one


@pytest.mark.parametrize('name', list(cases.CASES))
def test_tables_of_the_node_route_cases_do_not_depend_on_the_split(harness, tmp_path, name):
    elem, coord, _ = cases.mesh(name)
    path = str(tmp_path / 'm.bin')
    _dump(path, elem, coord.shape[1], coord)
    lines = _same_for_every_split(harness, path, 3)
    assert any(l.startswith('p1[default] scalars rc 0 ') for l in lines), lines[:12]


@pytest.mark.parametrize('t,k', FANS)
def test_tables_of_the_fans_do_not_depend_on_the_split(harness, tmp_path, t, k):
    elem, coord = fan_mesh(k, t, shuffle=k % 2 == 1)
    path = str(tmp_path / 'm.bin')
    _dump(path, elem, coord.shape[1], coord)
    _same_for_every_split(harness, path, elem.shape[0])
