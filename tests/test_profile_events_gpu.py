"""
The in-situ profile of a context (fep_ctx_profile_begin / fep_ctx_profile_end): every fep_step_dev / fep_assemble_dev call
records four events, so that N profiled calls report n_steps == N and three finite, non-negative mean intervals, on every
route and for every call form (bench.py --full and tools/elem_bench.py read them).
"""
import math

import numpy as np
import pytest

from conftest import dp_materials
from routes import assert_route

pytestmark = pytest.mark.gpu

N_CALLS = 5


@pytest.mark.parametrize('t,route', [('P1', 'node'), ('P2', 'patch'), ('P2', 'coo')])
def test_profile_reports_every_call(fep, monkeypatch, t, route):
    import torch
    if route == 'coo':
        monkeypatch.setenv('FEP_ROUTE', 'coo')
    else:
        monkeypatch.delenv('FEP_ROUTE', raising=False)
    mesh = fep.square_mesh(16, t, 10)
    ctx = fep.MeshContext(mesh['elements'], mesh['coordinates'])
    assert_route(ctx, route)
    n = ctx.n_int
    ctx.set_materials(*dp_materials(n))
    dev = torch.device('cuda', 0)
    f64 = dict(dtype=torch.float64, device=dev)
    x, y = mesh['coordinates']
    U = np.array([2.5e-4 * y * (x / 10), -1.5e-4 * y * (x < 5) + 2.0e-4 * y * (x >= 5)])
    Ud = torch.from_numpy(np.ascontiguousarray(U.reshape(-1, order='F'))).to(dev)
    Ep = torch.zeros((4, n), **f64); S = torch.zeros((4, n), **f64); DS = torch.zeros((9, n), **f64)
    ind = torch.zeros(n, dtype=torch.uint8, device=dev); Kd = torch.zeros(ctx.nnz, **f64); F = torch.zeros(ctx.n_dof, **f64)
    cnt = torch.zeros(2, dtype=torch.int64, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    forms = {
        'full': lambda: ctx.step_dev(st, Ud.data_ptr(), ep=Ep.data_ptr(), s=S.data_ptr(), ds=DS.data_ptr(),
                                     ind_p=ind.data_ptr(), k_data=Kd.data_ptr(), f_out=F.data_ptr(), counts=cnt.data_ptr()),
        'kf': lambda: ctx.step_dev(st, Ud.data_ptr(), ep=Ep.data_ptr(), k_data=Kd.data_ptr(), f_out=F.data_ptr(),
                                   counts=cnt.data_ptr()),
        'assemble': lambda: ctx.assemble_dev(st, ds=DS.data_ptr(), s=S.data_ptr(), k_data=Kd.data_ptr(), f_out=F.data_ptr()),
    }
    for form, call in forms.items():
        call()                                                  # (lazy allocations outside the profile)
        torch.cuda.synchronize()
        ctx.profile_begin()
        for _ in range(N_CALLS):
            call()
        ms, n_steps = ctx.profile_end(st)
        assert n_steps == N_CALLS, (form, n_steps)
        assert set(ms) == {'element', 'csr', 'force'}
        assert all(math.isfinite(v) and v >= 0.0 for v in ms.values()), (form, ms)
    ctx.close()
