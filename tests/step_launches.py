"""
The launches the profiler recorded for tools/step_trace.py's matrix (tests/golden/step_launches.json: {case label: [kernel
names]}, taken from the commit before the step plan), read for the tests that hold the plan (test_step_plan_host.py) and
fep_ctx_kernel_names (test_step_launches_gpu.py) to them.
"""
import json
import os
import re

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'step_launches.json')
SUM_KERNELS = ('counts_finalize_kernel', 'counts_reduce_kernel')

# a recorded kernel name -> the stage that launches it (tests/step_plan_host.cpp, stages_of)
STAGE_OF = [
    (r'^p1_point_\w*kernel(<\d+>)?$|^point_\w*kernel<[\d, ]+>$', 'point'),
    (r'^element_kernel<\d+, \d+, true, ', 'element_u'),
    (r'^element_kernel<\d+, \d+, false, ', 'element_ds'),
    (r'^p1_fused_kernel<(true|false), \d+, (true|false), 1, 1, false, ', 'one_kernel'),
    (r'^p1_fused_kernel<false, \d+, (true|false), 1, 1, true, ', 'from_nodes'),
    (r'^p1_node_lds_kernel<', 'tile'),
    (r'^p1_node_kernel$', 'direct'),
    (r'^fixup_kernel$', 'fixup'),
    (r'^csr_reduce_pk_kernel$', 'reduce_pk'),
    (r'^csr_reduce_kernel<\d+>$', 'reduce'),
    (r'^force_reduce_kernel$', 'force'),
    (r'^counts_finalize_kernel$', 'finalize'),
    (r'^counts_reduce_kernel$', 'counts_reduce'),
]
ROUTE_ID = {'P1Node': 0, 'Patch': 1, 'Coo': 2}
WANTS = {'all': 'e s ds ind_p K F', 'KF': 'K F', 'K': 'K', 'F': 'F', 'points': 'e s ds ind_p'}


def stage_of(kernel):
    hits = [stage for pattern, stage in STAGE_OF if re.search(pattern, kernel)]
    assert len(hits) == 1, (kernel, hits)
    return hits[0]


def route_of(mesh, route):
    """The route a context of tools/step_trace.py's matrix takes (fep_api.hip, choose_route)"""
    return {'default': 'P1Node' if mesh.startswith('P1') else 'Patch', 'patch': 'Patch', 'coo': 'Coo'}[route]


def recorded():
    """{case label: [kernel names]}"""
    with open(GOLDEN) as f:
        return json.load(f)


def golden_cases():
    """[(label, (mesh, route), the route it is, dp, wants dict, recorded stages)] of the recorded launches"""
    cases = []
    for label, kernels in recorded().items():
        part = label.split('/')
        mesh, route, model = part[:3]
        w = dict.fromkeys(('accept', 'e', 's', 'ds', 'ind_p', 'K', 'F', 'counts', 'field', 'assemble'), 0)
        if part[3].startswith('assemble:'):
            w['assemble'] = 1
            outputs = WANTS[part[3].split(':')[1]]
        else:
            w['field'], w['accept'], w['counts'] = int(part[3][-1]), int(part[4][-1]), int(part[6][-1])
            outputs = WANTS[part[5].split(':')[1]]
        for k in outputs.split():
            w[k] = 1
        cases.append((label, (mesh, route), route_of(mesh, route), int(model == 'dp'), w, [stage_of(k) for k in kernels]))
    return cases


def no_open_contexts(cases):
    """The (mesh, route) contexts whose patches leave no open block (one patch).  A fix-up launch that sums no counters has an
    empty grid there and its launcher skips it: the record of such a context shows fixup_kernel in no case without the counter
    sum -- in none at all, or the record is inconsistent."""
    found = set()
    for ctx in {c[1] for c in cases}:
        mine = [c for c in cases if c[1] == ctx and c[2] == 'Patch' and not c[4]['counts'] and (c[4]['K'] or c[4]['F'])]
        if mine and not any('fixup' in c[5] for c in mine):
            found.add(ctx)
    return found
