"""
fep_ctx_kernel_names against the launches the profiler recorded (tests/golden/step_launches.json, tools/step_trace.py): on
the record's two meshes, every route and every material model, kernel_names(0) and kernel_names(1) are the kernels of the
recorded non-accepting step with every output / with K and F alone, the counter-sum kernels left out, joined by ' + '.  The
string bench.py labels its roofline with is thereby what a step of that context launched, for every route and model.

One term is the record's own to explain: fixup_kernel with an empty grid is not launched.  On a mesh whose patches leave no
open block (the Q1 mesh of 16 elements is one patch; step_launches.no_open_contexts reads this off the record) the fix-up runs
only to sum the branch counters, which a staged step leaves to counts_reduce_kernel: there the name list keeps a fixup_kernel
that the record lacks, and nothing else may differ.
"""
import pytest

from step_launches import SUM_KERNELS, golden_cases, no_open_contexts, recorded, route_of

pytestmark = pytest.mark.gpu

RECORD = recorded()
NO_OPEN = no_open_contexts(golden_cases())
MODELS = ('dp', 'vm', 'mc', 'vmps', 'vmi')


def recorded_names(mesh, route, model, wants):
    kernels = RECORD[f'{mesh}/{route}/{model}/field0/accept0/step:{wants}/counts1']
    return [k for k in kernels if k not in SUM_KERNELS]


@pytest.mark.parametrize('route', ['default', 'patch', 'coo'])
@pytest.mark.parametrize('t,n', [('P1', 20), ('Q1', 4)])
def test_kernel_names_are_the_recorded_launches(fep, monkeypatch, t, n, route):
    if route == 'default':
        monkeypatch.delenv('FEP_ROUTE', raising=False)
    else:
        monkeypatch.setenv('FEP_ROUTE', route)
    mesh = fep.square_mesh(n, t, 10)
    ctx = fep.MeshContext(mesh['elements'], mesh['coordinates'])
    name = f'{t}-{n}'
    try:
        for model in MODELS:
            ctx.set_model(model)
            for which, wants in ((0, 'all'), (1, 'KF')):
                got = ctx.kernel_names(which).split(' + ')
                want = recorded_names(name, route, model, wants)
                if (name, route) in NO_OPEN and 'fixup_kernel' not in want:
                    assert route_of(name, route) == 'Patch' and got[-1] == 'fixup_kernel', (model, which, got, want)
                    got = got[:-1]
                print(model, which, got)
                assert got == want, (model, which, got, want)
    finally:
        ctx.close()
