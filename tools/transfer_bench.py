#!/usr/bin/env python3
"""
Times the state transfer across refinement (fep_mesh_child_corners_dev, fep_transfer_nodes_dev, fep_transfer_points_dev) on
the tunnel mesh of tests/golden/tsx.npz refined `refine` times (5: 908 288 triangles) with the elements whose centroid lies
within `--radius` of the tunnel's centre marked (8: about 30 %; the mesh is graded towards the tunnel), for P1 and P4, in one process and one session:

  resident   device tensors in -> device tensors out, HIP events after a warm-up: the corner codes, the node transfer of the
             interleaved displacement (n_comp = 2) and the point transfer of a plastic strain (4 rows), each and together
  copy       a plain device copy of the same output bytes, timed the same way in the same run: the yardstick
  twin       the NumPy twin (transfer_nodes_np, transfer_points_np, child_corners), one run: it is the slow side
  h2d_d2h    what a host round trip of the state would add to the twin: U and Ep down, the transferred ones up (the copies the
             device path saves)

and checks that device and twin agree bit for bit.  One JSON line, written to profiles/transfer_bench.json unless `--out`.

    python tools/transfer_bench.py [--refine 5] [--radius 8] [--type P1,P4] [--passes 5]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def events(torch, f, passes):
    ts = []
    for _ in range(passes):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        f()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return {'best_ms': min(ts), 'median_ms': float(np.median(ts))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--refine', type=int, default=5)
    ap.add_argument('--radius', type=float, default=8.0)
    ap.add_argument('--type', default='P1,P4')
    ap.add_argument('--passes', type=int, default=5)
    ap.add_argument('--device', type=int, default=0)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'transfer_bench.json'))
    a = ap.parse_args()
    import torch
    fep = importlib.import_module('fem-elastoplasticity_amd')
    fep.build()
    dev = a.device
    tdev = torch.device('cuda', dev)
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'tsx.npz'))
    coord, elem = fep.refine_uniform(g['coord'], g['elem'], levels=a.refine, device=dev)
    cx, cy = coord[0][elem].mean(axis=0), coord[1][elem].mean(axis=0)
    marked = cx * cx + cy * cy < a.radius ** 2
    res = {'tool': 'transfer_bench', 'refine': a.refine, 'device_name': torch.cuda.get_device_name(dev), 'n_e': int(elem.shape[1]),
           'n_marked': int(marked.sum()), 'marked_share': float(marked.mean())}
    coord_d, elem_d = torch.from_numpy(coord).to(tdev), torch.from_numpy(elem.astype(np.int32)).to(tdev)
    marked_d = torch.from_numpy(marked.view(np.uint8)).to(tdev)
    with fep.DeviceMesh(coord_d, elem_d, dev, on_device=True) as m:
        m.mark(marked_d, on_device=True)
        c_d, e_d, p_d = m.refine_marked_dev()
        cor_d = m.child_corners_dev()                                                 # warm-up
        torch.cuda.synchronize(dev)
        res['resident_corners'] = events(torch, m.child_corners_dev, a.passes)
    coord_c, elem_c = c_d.cpu().numpy(), e_d.cpu().numpy().astype(np.int64)
    parent, corners = p_d.cpu().numpy().astype(np.int64), cor_d.cpu().numpy()
    res['n_child'] = int(parent.size)
    t0 = time.perf_counter()
    twin_corners = fep.child_corners(coord, elem, marked)
    res['twin_corners_ms'] = 1e3 * (time.perf_counter() - t0)
    res['corners_bit_equal'] = twin_corners.tobytes() == corners.tobytes()
    rng = np.random.default_rng(1)
    for t in a.type.split(','):
        n_q = fep.ELEMENT_SHAPE[fep.LagrangeElementType[t]][1]
        if t == 'P1':
            ep, n_np, ec, n_nc = elem, coord.shape[1], elem_c, coord_c.shape[1]
        else:
            hp, hc = fep.create_midpoints(t, coord, elem, device=dev), fep.create_midpoints(t, coord_c, elem_c, device=dev)
            ep, n_np, ec, n_nc = hp['elem_ext'], hp['coord_ext'].shape[1], hc['elem_ext'], hc['coord_ext'].shape[1]
            del hp, hc
        u, q = rng.uniform(-1, 1, size=(n_np, 2)), rng.uniform(-1, 1, size=(4, elem.shape[1] * n_q))
        ep_d, ec_d = torch.from_numpy(ep.astype(np.int32)).to(tdev), torch.from_numpy(ec.astype(np.int32)).to(tdev)
        u_d, q_d = torch.from_numpy(u).to(tdev), torch.from_numpy(q).to(tdev)
        out_u = fep.transfer_nodes_dev(t, ep_d, ec_d, p_d, cor_d, u_d, n_nc)          # warm-ups: tables, owner scratch
        out_q = fep.transfer_points_dev(t, p_d, cor_d, q_d)
        torch.cuda.synchronize(dev)
        r = {'n_n_parent': int(n_np), 'n_n_child': int(n_nc),
             'output_bytes': int(out_u.numel() * 8 + out_q.numel() * 8 + cor_d.numel())}
        r['resident_nodes'] = events(torch, lambda: fep.transfer_nodes_dev(t, ep_d, ec_d, p_d, cor_d, u_d, n_nc, out=out_u), a.passes)
        r['resident_points'] = events(torch, lambda: fep.transfer_points_dev(t, p_d, cor_d, q_d, out=out_q), a.passes)
        r['resident_total_ms'] = res['resident_corners']['median_ms'] + r['resident_nodes']['median_ms'] + r['resident_points']['median_ms']
        copies = [torch.empty_like(o) for o in (out_u, out_q, cor_d)]

        def copy():
            for dst, src in zip(copies, (out_u, out_q, cor_d)):
                dst.copy_(src)
        copy()
        r['copy'] = events(torch, copy, a.passes)
        r['total_over_copy'] = r['resident_total_ms'] / r['copy']['median_ms']

        def round_trip():
            u_d.cpu(), q_d.cpu()
            out_u.copy_(torch.from_numpy(got_u)), out_q.copy_(torch.from_numpy(got_q))
        got_u, got_q = out_u.cpu().numpy(), out_q.cpu().numpy()
        r['h2d_d2h'] = events(torch, round_trip, a.passes)
        t0 = time.perf_counter()
        want_u = fep.transfer_nodes_np(t, ep, ec, parent, corners, u, n_n_child=n_nc)
        t1 = time.perf_counter()
        want_q = fep.transfer_points_np(t, parent, corners, q)
        t2 = time.perf_counter()
        r['twin_ms'] = {'nodes': 1e3 * (t1 - t0), 'points': 1e3 * (t2 - t1), 'corners': res['twin_corners_ms']}
        r['twin_plus_copies_ms'] = r['twin_ms']['nodes'] + r['twin_ms']['points'] + r['twin_ms']['corners'] + r['h2d_d2h']['median_ms']
        r['bit_equal'] = {'nodes': got_u.tobytes() == want_u.tobytes(), 'points': got_q.tobytes() == want_q.tobytes()}
        r['speedup_over_twin_plus_copies'] = r['twin_plus_copies_ms'] / r['resident_total_ms']
        res[t] = r
        del ep_d, ec_d, u_d, q_d, out_u, out_q, copies, want_u, want_q, got_u, got_q
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
