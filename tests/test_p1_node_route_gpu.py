"""
The P1 node route (p1_point_kernel + p1_node_lds_kernel for a full-output step, p1_fused_kernel for the K,F-only step: the
default of every P1 mesh and the headline of bench.py) against the element-by-element float64 reference, entry by entry,
in every form its host plan comes out as.

The three stages, their tolerances and the bitwise pins of the K,F-only, K-only, F-only steps and assemble(ds, s) are
test_element_route_gpu._run_case's.  Stage 3 differs in what it compares with, because the node route's kernels assemble
from the 48-byte record (gradients of local nodes 0 and 1, d[2] = -(d[0] + d[1]); elem_ref's module docstring):
  * against the RECORD form on its plain scale: C_K['P1'] = 10, C_F['P1'] = 8, the element route's bounds, unchanged: the
    node route sums these very terms, in another order;
  * against the EXACT form (the table gradients) on the widened scale: C + C_RECORD = 14, 12.
Every case asserts the plan form it exists for, from the library's own plan line, against the table of
tests/p1_node_cases.py that test_p1_node_cases.py checks on the CPU with the host plan builder.

Measured worst ratios (MI355X, every case of this module, the benchmark mesh included), each beside its bound:
  E 3.13 (6);  record form, plain scale: K 4.73 (10), F 5.13 (8);  exact form, widened scale: K 4.65 (14), F 4.66 (12).
The benchmark mesh alone: E 2.25, K 4.49, F 3.93; K 3.76, F 3.65.  No case exceeded a bound, so none was raised, and no
count of roundings had to be made for one.
"""
import numpy as np
import pytest

import p1_node_cases as cases
from elem_ref import ElemRef
from test_element_route_gpu import _run_case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('name', list(cases.CASES))
def test_node_route_vs_reference_per_entry(fep, monkeypatch, capfd, name):
    state, form = cases.CASES[name]
    elem, coord, h = cases.mesh(name)
    rng = np.random.default_rng(cases.seed(name) + 1)
    keep = {}
    # form None: a node of 16 elements does not fit the packed descriptor, the mesh must come back on the element route
    plan = _run_case(fep, monkeypatch, capfd, 'P1', 'default' if form is None else 'node', elem, coord, state, h, rng, keep=keep)
    if form is None:
        assert 'eb' in plan                                          # the patch plan's figures
        return
    print(f'[plan] {name}: {plan}')
    cases.check_form(name, plan, form)
    if name == 'orphans':                                            # nodes of no element: no lane writes their force
        F = keep['full']['F']
        for n in cases.ORPHANS:
            assert F[2 * n] == 0 and F[2 * n + 1] == 0
    if name == 'mixed24':
        assert (ElemRef(elem, coord, fep.element_tables('P1')).det() < 0).mean() > 0.3


def test_node_route_whole_benchmark_mesh(fep, monkeypatch, capfd):
    """square(708), the 1 002 528 elements bench.py measures: every CSR entry of K and every entry of F, not a sample."""
    name, state, form = cases.BENCH
    elem, coord, h = cases.mesh(name)
    assert elem.shape[1] == 1_002_528
    plan = _run_case(fep, monkeypatch, capfd, 'P1', 'node', elem, coord, state, h, np.random.default_rng(708))
    print(f'[plan] {name}: {plan}')
    cases.check_form(name, plan, form)
