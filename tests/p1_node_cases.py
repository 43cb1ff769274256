"""
The cases of the P1 node route's per-entry test, and the plan form each of them exists for: one table, read by
test_p1_node_route_gpu.py (the library's own plan line, printed under FEP_VERBOSE) and by test_p1_node_cases.py (the host
plan builder through tests/host_san.cpp, no GPU), so that the case list can be maintained on a machine without a GPU and
the GPU test fails if library and harness disagree.

A plan form (fep_host.h: build_p1_plan) is what the kernels branch on:
  segs        segments per tile, 1 (row strips) or 2 (two-row tiles)
  rng         the tiles' element lists as <= 8 runs (1) or as lists (0): the template argument RNG of both kernels
  fused_rng   the node lists of the K,F-only step as runs (1) or as lists (0): `fused 1/M` of the plan line
  L, NL       the longest staged element list and node list over the tiles; NL = 256 is one staged node per lane
  tiles       the number of workgroups
  last        (host side only) blocks, nodes and owned elements of the last tile
CASES maps a name to (state, form); form holds exact values (int), or (lo, hi) ranges for the meshes whose numbering is
random.  `mesh(name)` builds the mesh of a case; the state names are those of test_element_route_gpu._state.

Structured residues: a tile holds at most 256 blocks, interior nodes have 7, so about 36 nodes.  rect(52 | 53 | 54, 10)
end in a tile of 16 nodes, of ONE node (3 blocks) and of 31 nodes; rect(47, 8) and rect(17, 12) end in a tile of exactly
256 blocks; `-1` drops the last element, the only one of the last node, which then has no block and belongs to no tile:
the last tile loses a node and five blocks, and in rect(17, 12), where it owns that element, one of its `own`.

swapped24 is the one form no ordinary mesh of the suite gives, element lists that compress with node lists that do not
(rng 1, fused_rng 0): square(24) with three neighbouring node ids exchanged with three far ones, and the elements those
six nodes touch moved to the end of the element list, so that a tile's remote nodes cost one run of elements and four
runs of nodes each.  Found by a search over such exchanges with the host harness.
"""
import re
import zlib

import numpy as np

import meshes
from conftest import load_golden
from fan_mesh import fan_mesh

ONE = dict(segs=1, rng=1, fused_rng=1)
TWO = dict(segs=2, rng=1, fused_rng=1)
LISTS = dict(rng=0, fused_rng=0)

CASES = {
    # -- structured residues
    'rect52x10': ('plain', dict(TWO, tiles=16, L=112, NL=104, last=(97, 16, 0))),
    'rect53x10': ('wide', dict(TWO, tiles=17, L=114, NL=104, last=(3, 1, 0))),
    'rect54x10': ('tsx', dict(TWO, tiles=16, L=114, NL=104, last=(189, 31, 8))),
    'rect54x10-1': ('accept', dict(TWO, tiles=16, L=114, NL=104, last=(185, 30, 8))),
    'rect47x8': ('accept', dict(ONE, tiles=11, L=146, NL=116, last=(256, 51, 5))),
    'rect17x12': ('plain', dict(ONE, tiles=6, L=104, NL=74, last=(256, 43, 47))),
    'rect17x12-1': ('wide', dict(ONE, tiles=6, L=104, NL=74, last=(251, 42, 46))),
    # -- one tile, two tiles
    'square1': ('plain', dict(ONE, tiles=1, L=2, NL=4)),
    'square2': ('accept', dict(ONE, tiles=1, L=8, NL=10)),
    'square7': ('tsx', dict(ONE, tiles=2, L=72, NL=50)),
    # -- geometry: general triangles, det < 0, cells 1 : 1000, nearly right angles
    'jittered24': ('wide', dict(ONE, tiles=17, L=120, NL=88)),
    'mixed24': ('accept', dict(ONE, tiles=17, L=120, NL=88)),
    'aniso': ('plain', dict(ONE, tiles=4, L=88, NL=60)),
    'nearright24': ('tsx', dict(ONE, tiles=17, L=120, NL=88)),
    # -- strips: short tiles
    'strip301x1': ('tsx', dict(TWO, tiles=13, L=70, NL=72)),
    'strip1x301': ('wide', dict(ONE, tiles=12, L=54, NL=56)),
    'strip3x2000': ('accept', dict(ONE, tiles=191, L=70, NL=50)),
    # -- two segments, runs
    'square60': ('wide', dict(TWO, tiles=111, L=114, NL=90)),
    # -- lists, one staged node per lane
    'renumbered150': ('accept', dict(LISTS, segs=1, NL=256, L=(201, 256))),
    'renumbered24': ('plain', dict(LISTS, segs=1, tiles=17)),
    'delaunay24r': ('wide', dict(LISTS, segs=1)),
    'tsx': ('tsx', dict(LISTS, segs=1, tiles=13, L=218, NL=218)),
    # -- two segments with list tables
    'shuffled150': ('accept', dict(LISTS, segs=2, tiles=657, L=126, NL=112)),
    'shuffled60': ('tsx', dict(LISTS, segs=2, tiles=111, L=114, NL=90)),
    'delaunay150': ('wide', dict(LISTS, segs=2)),
    # -- element lists as runs, node lists as lists
    'swapped24-accept': ('accept', dict(segs=1, rng=1, fused_rng=0, tiles=17)),
    'swapped24-wide': ('wide', dict(segs=1, rng=1, fused_rng=0, tiles=17)),
    'swapped24-tsx': ('tsx', dict(segs=1, rng=1, fused_rng=0, tiles=17)),
    # -- nodes of no element
    'orphans': ('accept', dict(ONE, tiles=6, L=94, NL=64)),
    # -- a diagonal block of 15 contributions, the last length the packed descriptor holds; 16: the element route
    'fan15': ('wide', dict(ONE, tiles=1, L=46, NL=32, last=(181, 31, 45))),
    'fan15s': ('tsx', dict(ONE, tiles=1, L=46, NL=32, last=(181, 31, 45))),
    'fan16': ('plain', None),
}
# the whole benchmark mesh, a test of its own on the GPU (every entry)
BENCH = ('square708', 'plain', dict(TWO, tiles=14444, L=126, NL=112, last=(118, 24, 0)))
ORPHANS = (50, -1)                                # 'orphans': the nodes of no element
SWAPS = ((373, 148), (374, 588), (375, 526))      # 'swapped24'

HOST_LINE = re.compile(r'p1 plan \[default\]: rc 0 check 0 tiles (\d+) segs (\d+) staged \d+ \([\d.]+ per element\) nodes \d+ '
                       r'L (\d+) C (\d+) NL (\d+) lds 1 rng (\d) pk (\d) fused (\d)/(\d)')
HOST_LAST = re.compile(r'last tile: blocks (\d+) nodes (\d+) own (\d+) staged \d+')
LIB_LINE = re.compile(r'\[fep\] P1 plan: (\d+) tiles of <= 256 blocks in <= (\d+) segment\(s\), staged elements \d+ '
                      r'\([\d.]+ per element, <= (\d+) per tile\), staged nodes <= (\d+), codes <= (\d+); '
                      r'lds 1 rng (\d) pk (\d) fused (\d)/(\d)')


def seed(name):
    return zlib.crc32(f'P1 node {name}'.encode())


def parse_host(out):
    """The form the host harness printed, or None where the default plan is not packed (the element route)."""
    m = HOST_LINE.search(out)
    assert m, out[-2000:]
    tiles, segs, L, C, NL, rng, pk, fused, fused_rng = [int(v) for v in m.groups()]
    if not pk:
        return None
    assert fused == 1
    last = HOST_LAST.search(out)
    return dict(tiles=tiles, segs=segs, L=L, NL=NL, rng=rng, fused_rng=fused_rng, last=tuple(int(v) for v in last.groups()))


def parse_lib(err):
    """The form of the library's plan line (the last context created), or None where it printed none."""
    m = LIB_LINE.findall(err)
    if not m:
        return None
    tiles, segs, L, NL, C, rng, pk, fused, fused_rng = [int(v) for v in m[-1]]
    assert pk == 1 and fused == 1
    return dict(tiles=tiles, segs=segs, L=L, NL=NL, rng=rng, fused_rng=fused_rng)


def check_form(name, got, want):
    """`got` (parse_host / parse_lib) has the form the table states for the case; keys `got` lacks are not its to check."""
    if want is None:
        assert got is None, (name, got)
        return
    assert got is not None, name
    for k, v in want.items():
        if k not in got:
            continue
        if isinstance(v, tuple) and k != 'last':
            assert v[0] <= got[k] <= v[1], (name, k, got[k], v)
        else:
            assert got[k] == v, (name, k, got[k], v)


def mesh(name):
    """(elem, coord, typical element size h) of a case."""
    rng = np.random.default_rng(seed(name))
    m = re.match(r'rect(\d+)x(\d+)(?:-(\d+))?$', name)
    if m:
        nx, ny, k = int(m.group(1)), int(m.group(2)), int(m.group(3) or 0)
        elem, coord = meshes.rect('P1', nx, ny)
        return meshes.drop_last(elem, k), coord, 10 / max(nx, ny)
    m = re.match(r'strip(\d+)x(\d+)$', name)
    if m:                                                                   # on 10 x 10: cells of 1 : 300, 1 : 670
        nx, ny = int(m.group(1)), int(m.group(2))
        return (*meshes.rect('P1', nx, ny), 10 / max(nx, ny))
    m = re.match(r'square(\d+)$', name)
    if m:
        n = int(m.group(1))
        return (*meshes.square('P1', n), 10 / n)
    if name == 'aniso':                                                     # cells 1 : 1000
        return (*meshes.rect('P1', 10, 10, 10.0, 0.01), 1e-3)
    if name == 'tsx':
        g = load_golden('tsx')
        return np.ascontiguousarray(g['elem'], dtype=np.int64), np.ascontiguousarray(g['coord'], dtype=float), 2.0
    if name == 'orphans':                                                   # test_p1_mesh_with_a_node_of_no_element's
        elem, coord = meshes.square('P1', 12)
        coord = np.concatenate([coord[:, :50], [[3.3], [4.4]], coord[:, 50:], [[20.0], [20.0]]], axis=1)
        return np.where(elem >= 50, elem + 1, elem), coord, 10 / 12
    if name.startswith('fan'):
        k = int(re.match(r'fan(\d+)', name).group(1))
        return (*fan_mesh(k, 'P1', shuffle=name.endswith('s')), 2 * np.pi / k)
    if name.startswith('shuffled'):                                         # the elements in random order, the nodes as they are
        n = int(name[8:])
        elem, coord = meshes.square('P1', n)
        return np.ascontiguousarray(elem[:, rng.permutation(elem.shape[1])]), coord, 10 / n
    if name.startswith('renumbered'):
        n = int(name[10:])
        elem, coord = meshes.square('P1', n)
        coord = meshes.jitter(elem, coord, 0.1, rng)
        return (*meshes.renumber(elem, coord, rng), 10 / n)
    if name == 'delaunay150':                                               # row order
        return (*meshes.delaunay('P1', 150, rng), 10 / 150)
    if name == 'delaunay24r':
        return (*meshes.renumber(*meshes.delaunay('P1', 24, rng), rng), 10 / 24)
    elem, coord = meshes.square('P1', 24)
    if name in ('jittered24', 'mixed24'):
        coord = meshes.jitter(elem, coord, 0.15, rng)
        if name == 'mixed24':
            elem = meshes.mixed_orientation(elem, rng)
        return elem, coord, 10 / 24
    if name == 'nearright24':
        return elem, near_right(coord, rng), 10 / 24
    if name.startswith('swapped24'):
        jig = np.random.default_rng(seed('swapped24'))                      # one mesh for the three states
        coord = meshes.jitter(elem, coord, 0.1, jig)
        m = np.arange(coord.shape[1])
        for a, b in SWAPS:
            m[a], m[b] = b, a
        elem = m[elem]
        touched = np.isin(elem, np.array(SWAPS).ravel()).any(axis=0)
        order = np.concatenate([np.flatnonzero(~touched), np.flatnonzero(touched)])
        return np.ascontiguousarray(elem[:, order]), np.ascontiguousarray(coord[:, m]), 10 / 24
    raise KeyError(name)


def near_right(coord, rng, amount=1e-9):
    """Every interior node of a structured mesh moved by up to `amount` in each direction: right angles that are not quite
    right, so that the gradient of a triangle's right-angle node has a component of ~1e-9 of the others', which
    -(d[0] + d[1]) gives with the absolute error of the large ones."""
    coord = np.array(coord, dtype=float, copy=True)
    x, y = coord
    inner = (x > x.min()) & (x < x.max()) & (y > y.min()) & (y < y.max())
    coord[:, inner] += rng.uniform(-amount, amount, size=(2, int(inner.sum())))
    return coord
