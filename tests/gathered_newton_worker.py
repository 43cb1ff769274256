"""
One rank of the gathered-solve tests (tests/test_gathered_solve_gpu.py):
`python tests/gathered_newton_worker.py RANK WORLD PORT OUTDIR JOB`, every rank on cuda:0, gloo rendezvous on 127.0.0.1.
JOB is a JSON object: {"job": "footing", ...arguments of solve_strip_footing_sharded},
{"job": "tsx", "refine": 0 | 1} (the golden TSX mesh, P1) or {"job": "cap"} (one solve capped at max_iter = 1).
Every solve is the multigrid one on K gathered to rank 0 (dist_newton.GatheredSolver).  Writes OUTDIR/rank<r>.npz.
"""
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    rank, world, port, outdir = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    job = json.loads(sys.argv[5])
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=port, RANK=str(rank), WORLD_SIZE=str(world))
    os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    import torch
    import torch.distributed as dist
    dist.init_process_group('gloo', rank=rank, world_size=world)
    torch.cuda.set_device(0)
    fep = importlib.import_module('fem-elastoplasticity_amd')
    kind = job.pop('job')
    out = os.path.join(outdir, f'rank{rank}.npz')
    if kind == 'footing':
        h = fep.solve_strip_footing_sharded('P1', device=0, linear_solver='amg', **job)
        np.savez(out, zeta=np.array(h['zeta']), pressure=np.array(h['pressure']), U=np.array(h['U']),
                 n_calls=np.array(h['n_calls']), counts=np.array(h['counts']), pcg_iters=np.array(h['pcg_iters']),
                 n_local_points=np.array(h['Ep'].shape[1]))
    elif kind == 'tsx':
        g = np.load(os.path.join(ROOT, 'tests', 'golden', 'tsx.npz'), allow_pickle=False)
        h = fep.solve_tsx_tunnel_sharded(g['coord'], g['elem'], 'P1', device=0, linear_solver='amg', **job)
        np.savez(out, zeta=np.array(h['zeta']), n_plast=np.array(h['n_plast']), displ=np.array(h['displ']),
                 U_final=h['U'][-1], pcg_iters=np.array(h['pcg_iters']), n_calls=np.array(h['n_calls']))
    elif kind == 'cap':
        dn = importlib.import_module('fem-elastoplasticity_amd.dist_newton')
        mesh = fep.square_mesh(20, 'P1', 10)
        sc = fep.ShardedContext(mesh['elements'], mesh['coordinates'], rank, world, device=0)
        sc.set_materials(*[v[0] for v in _materials(1)])
        qf = mesh['Q'].flatten(order='F')
        ops = dn._ShardOps(sc, qf, max_iter=1, linear_solver='amg', elements_global=mesh['elements'])
        K = ops.step(ops.zeros(), want=('K',), keep_K=True)['K']
        ops.setup_amg(K, mesh['coordinates'])
        b = np.random.default_rng(5).normal(size=qf.size)
        x = ops.solve(K, ops.vec(b))
        capped = dict(ops.solver.last)
        ops.max_iter = 200000
        y = ops.solve(K, ops.vec(b))
        np.savez(out, x=x.cpu().numpy(), last=np.array([capped['iters'], capped['relres'], capped['state']]),
                 y_finite=np.array(bool(torch.isfinite(y).all())), last_full=np.array([ops.solver.last['iters'],
                                                                                      ops.solver.last['state']]))
        ops.close()
        sc.close()
    else:
        raise ValueError(kind)
    dist.barrier()
    dist.destroy_process_group()


def _materials(n):
    young, poisson, c0, phi = 1e7, 0.48, 450, np.pi / 9
    one = np.ones(n)
    return (young / (2 * (1 + poisson)) * one, young / (3 * (1 - 2 * poisson)) * one,
            3 * np.tan(phi) / np.sqrt(9 + 12 * np.tan(phi) ** 2) * one, 3 * c0 / np.sqrt(9 + 12 * np.tan(phi) ** 2) * one)


if __name__ == '__main__':
    main()
