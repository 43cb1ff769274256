"""
The P1 tile kernels' head (p1_node_lds_kernel, p1_fused_kernel: the tile's 256-byte record fetched in one scalar round trip at
entry, fep_kernels.hip.h load_tile_rec) on the smallest meshes that can break the record or the head:

  one tile          square(2): 2 x 2 cells, 8 elements
  7, 8, 9 tiles     square(15), square(16), square(17): the grid is rounded up to a multiple of 8 workgroups, so one, no and
                    seven workgroups leave at `wg >= n_wg`
  partial segment   rect(53, 10): two-segment tiles, the last tile is ONE node (3 blocks)
  1 / 2 segments    strip(1, 301) and the tsx-tunnel mesh (row strips) against square(60) (two-row tiles).  Tiles of 3 and
                    4 segments exist only in the measurement build (FEP_P1_SEGS); the product's plans have at most 2.
  list form         renumbered24: random numbering, neither list compresses into runs (RNG = false: the record's run part is
                    empty); swapped24: element runs with node LISTS
  Delaunay          jittered Delaunay points in row order
  materials, e0     per-point materials spanning decades (`wide`), the initial strain of the tsx case (`tsx`)

Every case runs test_element_route_gpu._run_case on the node route, which asserts, for the mesh:
  * K and F of the two-kernel full-output step equal the one-kernel K,F-only step (and the K-only, F-only steps) bit for bit
    — the two kernels' heads differ, so this is an independent check of both;
  * E, K and F within the per-entry bounds of tests/elem_ref.py against the float64 element reference (C_E, C_K, C_F of
    test_element_route_gpu.py, unchanged);
  * fep_assemble_dev(ds, s) equal to the step's K and F;
  * ind_p and the branch counts exact against the oracle's return map;
and the plan is replayed by FEP_VALIDATE_PLAN (record against tables included).  Each case also pins the tile count.
"""
import numpy as np
import pytest

import meshes
import p1_node_cases as cases
from test_element_route_gpu import _run_case

pytestmark = pytest.mark.gpu

# name -> (mesh, state, expected form).  `mesh`: a p1_node_cases name or a callable -> (elem, coord, h)
CASES = {
    'one_tile': ('square2', 'plain', dict(tiles=1, segs=1, rng=1, fused_rng=1)),
    'tiles7': ('square15', 'wide', dict(tiles=7, segs=1, rng=1, fused_rng=1)),
    'tiles8': ('square16', 'tsx', dict(tiles=8, segs=1, rng=1, fused_rng=1)),
    'tiles9': ('square17', 'accept', dict(tiles=9, segs=1, rng=1, fused_rng=1)),
    'partial_segment': ('rect53x10', 'tsx', dict(tiles=17, segs=2, rng=1, fused_rng=1)),
    'strip_one_segment': ('strip1x301', 'tsx', dict(tiles=12, segs=1, rng=1, fused_rng=1)),
    'tsx_one_segment': ('tsx', 'wide', dict(tiles=13, segs=1, rng=0, fused_rng=0)),
    'square_two_segments': ('square60', 'tsx', dict(tiles=111, segs=2, rng=1, fused_rng=1)),
    'lists': ('renumbered24', 'wide', dict(tiles=17, segs=1, rng=0, fused_rng=0)),
    'element_runs_node_lists': ('swapped24-wide', 'tsx', dict(tiles=17, segs=1, rng=1, fused_rng=0)),
    'delaunay': (lambda rng: (*meshes.delaunay('P1', 24, rng), 10 / 24), 'wide', dict(segs=1)),
}


@pytest.mark.parametrize('name', list(CASES))
def test_tile_head_on_small_meshes(fep, monkeypatch, capfd, name):
    mesh, state, form = CASES[name]
    rng = np.random.default_rng(cases.seed(f'tile record {name}'))
    elem, coord, h = mesh(rng) if callable(mesh) else cases.mesh(mesh)
    plan = _run_case(fep, monkeypatch, capfd, 'P1', 'node', elem, coord, state, h, rng)
    print(f'[plan] {name}: {plan}')
    cases.check_form(name, plan, form)
