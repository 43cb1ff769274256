"""
load_traction_kernel and load_volume_kernel at the shapes where they can go wrong, per entry against the high-precision
reference of tests/loads_exact.py (inputs: tests/load_cases.py, checked on the host by tests/test_loads_exact_host.py).

Traction: fep_load_traction_host through fep.load_traction and fep_load_traction_dev on torch tensors, on more than one
workgroup with a ragged last block (255 / 256 / 257 / 513 loaded nodes), 2- to 5-node edges, 1 to 8 surface points, the
curved tunnel wall and the ellipses of curved_cases as a caller gets them from `surf` / `surf_curve`, shuffled, repeated and
reversed edges, a hub of 40 edges beside lanes with one, node ids at both ends of 100 000, and no edges at all.
Bounds: loads_exact.traction_bound / volume_bound per entry (derived in that module's docstring),
load_cases.pressure_total_bound for the total of a pressure on a closed loop (derived there).  Everything else is bytes.
Every test prints the worst ratio to its bound before it asserts.
"""
from importlib import import_module

import numpy as np
import pytest

import load_cases as lc

pytestmark = pytest.mark.gpu

NAN = float('nan')


def _lib(fep):
    return import_module(fep.__name__ + '._lib')


def _device(fep):
    return import_module(fep.__name__ + '.hotpath').default_device()


def _ptr(fep, a):
    return _lib(fep).ptr(a)


class _DevCall:
    """One fep_load_traction_dev call on torch tensors: xy_d, t_int_d uploaded, f_out_d filled with NaN beforehand."""

    def __init__(self, fep, case, stream=None, **over):
        import torch
        self.dev = torch.device('cuda', _device(fep))
        self.n_n = case.n_n
        self.ed = np.ascontiguousarray(case.edges, dtype=np.int32)
        self.xy = torch.from_numpy(case.coord).to(self.dev)
        self.t = torch.from_numpy(case.t_int).to(self.dev)
        self.out = torch.full((2 * case.n_n,), NAN, dtype=torch.float64, device=self.dev)
        torch.cuda.synchronize()
        st = (stream or torch.cuda.current_stream(self.dev)).cuda_stream
        a = dict(n_n=case.n_n, n_e_s=case.n_e_s, n_p_s=case.n_p_s, n_q_s=case.n_q_s, edges=_ptr(fep, self.ed),
                 xy=self.xy.data_ptr(), t=self.t.data_ptr(), out=self.out.data_ptr())
        a.update(over)
        self.code = _lib(fep).lib().fep_load_traction_dev(self.dev.index, st, a['n_n'], a['n_e_s'], a['n_p_s'], a['n_q_s'], a['edges'],
                                                          a['xy'], _ptr(fep, case.h), _ptr(fep, case.dh), _ptr(fep, case.wf),
                                                          a['t'], a['out'])
        torch.cuda.synchronize()

    def raw(self):
        return self.out.cpu().numpy()

    def f(self):
        """(2, n_n): the (n_n, 2) interleaving undone."""
        return np.ascontiguousarray(self.raw().reshape(self.n_n, 2).T)


@pytest.mark.parametrize('name', lc.TRACTION_NAMES)
def test_traction_both_forms_per_entry(fep, name):
    import torch
    case = lc.traction_case(fep, name)
    exact, lim, m = lc.exact(case)
    coord0, t0 = case.coord.copy(), case.t_int.copy()
    host = fep.load_traction(*case.args())
    assert host.shape == (2, case.n_n) and host.dtype == np.float64
    lc.within(name + ' host form', host, exact, lim)                        # every entry, none left out
    assert host.tobytes() == fep.load_traction(*case.args()).tobytes()
    assert case.coord.tobytes() == coord0.tobytes() and case.t_int.tobytes() == t0.tobytes()
    side = torch.cuda.Stream(device=_device(fep))
    calls = [_DevCall(fep, case), _DevCall(fep, case), _DevCall(fep, case, stream=side), _DevCall(fep, case, stream=side)]
    for k, c in enumerate(calls):
        what = (name, 'device form, call', k)
        assert c.code == 0, what
        raw = c.raw()
        assert raw.shape == (2 * case.n_n,) and not np.isnan(raw).any(), what            # the NaN fill is gone everywhere
        f = c.f()
        off = f[:, m == 0]
        assert np.all(off == 0) and not np.signbit(off).any(), what                         # exactly 0.0 off the loaded nodes
        assert f.tobytes() == host.tobytes(), what                                          # host form == device form, bytes
        assert c.xy.cpu().numpy().tobytes() == coord0.tobytes() and c.t.cpu().numpy().tobytes() == t0.tobytes(), what
    dev = calls[0].f()
    lc.within(name + ' device form', dev, exact, lim)
    if case.pressure is not None and case.closed:
        b = lc.pressure_total_bound(case, dev)
        tot = np.abs(dev.sum(axis=1))
        print(f'{name}: |sum f| = {tot}, bound {b}, sum |f| = {np.abs(dev).sum(axis=1)}')
        assert np.all(tot <= b)
    if case.sorted_edges is not None:                                       # the order (e, a) is part of the contract: not bitwise
        srt = fep.load_traction(case.sorted_edges, case.coord, case.sorted_t, case.h, case.dh, case.wf)
        d = np.abs(srt - host)
        print(f'{name}: sorted against shuffled edges, worst |delta| / (2 bound) = {float((d / np.where(lim > 0, 2 * lim, 1.0)).max()):.3f}')
        assert np.all(d <= 2 * lim)


def test_traction_refusals_reach_no_kernel(fep):
    """Ordinary error returns: FEP_EINVAL = -1 for sizes outside 2..5 nodes / 1..8 points, a misaligned f_out_d and a missing
    t_int_d, FEP_ERANGE = -5 for a node id of n_n; f_out_d keeps its NaN fill, and a valid call passes after each."""
    case = lc.traction_case(fep, 'tunnel wall level 0 P2, 2-point, random, shuffled')
    exact, lim, m = lc.exact(case)
    bad_id = np.ascontiguousarray(case.edges, dtype=np.int32)
    bad_id[2, 7] = case.n_n
    refusals = [('n_p_s = 1', dict(n_p_s=1), -1), ('n_p_s = 6', dict(n_p_s=6), -1), ('n_q_s = 0', dict(n_q_s=0), -1),
                ('n_q_s = 9', dict(n_q_s=9), -1), ('f_out_d + 8', 'misaligned', -1), ('t_int_d NULL', dict(t=None), -1),
                ('node id n_n', dict(edges=_ptr(fep, bad_id)), -5)]
    for what, over, code in refusals:
        if over == 'misaligned':
            import torch
            big = torch.full((2 * case.n_n + 2,), NAN, dtype=torch.float64, device=torch.device('cuda', _device(fep)))
            c = _DevCall(fep, case, out=big.data_ptr() + 8)
            assert np.isnan(big.cpu().numpy()).all(), what
        else:
            c = _DevCall(fep, case, **over)
        assert c.code == code, (what, c.code)
        assert np.isnan(c.raw()).all(), what                                # nothing was written
        ok = _DevCall(fep, case)
        assert ok.code == 0, what
        lc.within(f'valid call after the refusal of {what}', ok.f(), exact, lim)
    l = _lib(fep).lib()
    ed = np.ascontiguousarray(case.edges, dtype=np.int32)
    out = np.full(2 * case.n_n, NAN)
    p = lambda a: _ptr(fep, a)                                                  # noqa: E731
    for n_p_s, n_q_s in ((1, 2), (6, 2), (3, 0), (3, 9)):
        assert l.fep_load_traction_host(_device(fep), case.n_n, case.n_e_s, n_p_s, n_q_s, p(ed), p(case.coord), p(case.h), p(case.dh),
                                        p(case.wf), p(case.t_int), p(out)) == -1
    assert l.fep_load_traction_host(_device(fep), case.n_n, case.n_e_s, 3, 2, p(ed), p(case.coord), p(case.h), p(case.dh), p(case.wf),
                                    None, p(out)) == -1
    assert np.isnan(out).all()
    lc.within('host form after the refusals', fep.load_traction(*case.args()), exact, lim)


# ---- volume ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', lc.VOLUME_NAMES)
def test_volume_per_entry_and_weight_override(fep, name):
    import torch
    t, elem, coord, f_rand = lc.volume_mesh(fep, name)
    n_n = coord.shape[1]
    ctx = fep.MeshContext(elem, coord)
    assert ctx.element_type.name == t
    w = ctx.geometry()[2].ravel().copy()
    assert w.min() > 0 and w.size == f_rand.shape[1]
    h = lc.hatp(fep, t)
    dev = torch.device('cuda', ctx.device)
    w2_d = torch.from_numpy(2 * w).to(dev)
    st = torch.cuda.current_stream(dev).cuda_stream

    def dev_form(**kw):
        out = torch.full((ctx.n_dof,), NAN, dtype=torch.float64, device=dev)
        ctx.load_volume_dev(st, out.data_ptr(), **kw)
        torch.cuda.synchronize()
        return np.ascontiguousarray(out.cpu().numpy().reshape(n_n, 2).T)

    f_d = torch.from_numpy(np.ascontiguousarray(f_rand)).to(dev)
    for kind, host_kw, dev_kw, f in (('random', dict(f_v_int=f_rand), dict(f_v_int=f_d.data_ptr()), f_rand),
                                     ('uniform', dict(uniform=lc.UNIFORM), dict(uniform=lc.UNIFORM), lc.uniform_field(w.size))):
        exact, lim, m = lc.exact_volume(elem, n_n, f, h, w)
        what = f'{name} {kind} (largest m = {m.max()})'
        host = ctx.load_volume(**host_kw)
        lc.within(what + ' host form', host, exact, lim)                   # every entry
        d1 = dev_form(**dev_kw)
        assert d1.tobytes() == host.tobytes() == dev_form(**dev_kw).tobytes(), what
        assert ctx.load_volume(hatp=h, weight=w, **host_kw).tobytes() == host.tobytes(), what
        # a caller's weights on the device form: twice the context's -> twice the result, exactly (a power of two)
        d2 = dev_form(weight=w2_d.data_ptr(), **dev_kw)
        assert not np.isnan(d2).any() and np.array_equal(d2, 2 * d1), what
        assert d2.tobytes() == ctx.load_volume(weight=2 * w, **host_kw).tobytes(), what
        assert w2_d.cpu().numpy().tobytes() == (2 * w).tobytes() and f_d.cpu().numpy().tobytes() == f_rand.tobytes()
    if name == 'fan 255 P1':
        assert m.max() == 255
    ctx.close()
