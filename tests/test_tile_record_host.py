"""
The P1 tile records (fep_host.h, P1Plan::rec: what p1_node_lds_kernel and p1_fused_kernel fetch at entry, one 256-byte
record per tile) on the CPU: for every P1 mesh the host tests build plans of — structured, strips, Delaunay in row order and
randomly numbered, the tsx-tunnel mesh, orphan nodes, one element, high-degree fans — and for every plan variant that changes
what a record holds (one / two / four segments, list form, unpacked, two-kernel plan), tests/tile_record_host.cpp decodes
each record the way the kernels do and compares it with the plan's own descriptor, element list and node list, entry by
entry; it also checks the stride, the alignment of the parts and that a run table that is not in use holds no live run.
Built with g++ -fsanitize=address,undefined as a stand-alone program.  No GPU.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import p1_node_cases as cases
from conftest import ROOT
from test_host_sanitizers import _dump, _meshes

SRC = os.path.join(ROOT, 'tests', 'tile_record_host.cpp')
VARIANTS = ('default', 'one segment', 'lists', 'unpacked', 'two kernels', 'four segments')


@pytest.fixture(scope='module')
def harness(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.skip('g++ not available')
    exe = str(tmp_path_factory.mktemp('tile_record') / 'tile_record_host')
    res = subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-pthread', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                          '-o', exe, SRC], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-3000:]
    return exe


def _check(harness, path, name):
    res = subprocess.run([harness, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert res.returncode == 0 and 'result ok' in res.stdout, (name, res.stdout[-3000:])
    assert 'runtime error' not in res.stdout and 'Sanitizer' not in res.stdout, (name, res.stdout[-3000:])
    lines = {l.split('[')[1].split(']')[0]: l for l in res.stdout.splitlines() if l.startswith('records [')}
    assert sorted(lines) == sorted(VARIANTS), res.stdout
    for v, l in lines.items():
        assert ': rc 0 check 0 record 0 tiles ' in l, l
        tiles = int(l.split(' tiles ')[1].split()[0])
        assert int(l.split(' bytes ')[1]) == 256 * tiles, l                 # one record of 256 bytes per tile
    return lines


def test_records_decode_to_the_plan_on_every_host_mesh(fep, harness, tmp_path):
    seen = {'rng 1': 0, 'rng 0': 0, 'segs 2': 0, 'fused 1/0': 0}
    for name, (elem, n_n, *_) in _meshes(fep).items():
        if np.shape(elem)[0] != 3:
            continue
        path = str(tmp_path / f'{name}.bin')
        _dump(path, elem, n_n)
        lines = _check(harness, path, name)
        assert ' rng 0 ' in lines['lists'], lines['lists']                  # the list form leaves the run part empty
        for key in seen:
            seen[key] += f' {key} ' in lines['default'] + ' '
    assert seen['rng 1'] and seen['rng 0'] and seen['segs 2'], seen         # run form, list form, two segments: all met


@pytest.mark.parametrize('name', ['square2', 'rect53x10', 'strip1x301', 'square60', 'renumbered24', 'delaunay150', 'swapped24-wide',
                                  'fan15s', 'orphans'])
def test_records_of_the_node_route_cases(harness, tmp_path, name):
    """The meshes of the node route's GPU cases whose plan form differs: one tile, a last tile of one node, strips, two
    segments, lists, two segments with lists, element runs with node lists, a fan, nodes of no element."""
    elem, coord, _ = cases.mesh(name)
    path = str(tmp_path / 'm.bin')
    _dump(path, elem, coord.shape[1])
    lines = _check(harness, path, name)
    _, form = cases.CASES[name]
    d = lines['default']
    for key, field in (('segs', ' segs {} '), ('rng', ' rng {} '), ('tiles', ' tiles {} ')):
        if key in form and not isinstance(form[key], tuple):
            assert field.format(form[key]) in d, (key, d)
    if 'fused_rng' in form:
        assert f' fused 1/{form["fused_rng"]} ' in d, d
