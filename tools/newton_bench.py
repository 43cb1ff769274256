#!/usr/bin/env python3
"""End-to-end run of BASELINE configs[3]: strip footing, N x N cells of P1 elements, `--steps` accepted
load steps, Newton iterate resident on the device (linear_solver='pcg').  Prints wall time, the share of the hot
path, and the PCG iteration counts.  Not the bench metric (bench.py times the hot path alone).

`--ranks N` with N > 1 runs the element-sharded driver (solve_strip_footing_sharded with `--solver`; 'amg' is the multigrid
solve on K gathered to rank 0): without WORLD_SIZE in the environment this process starts the N ranks as a CHILD
(`python -m torch.distributed.run ...`, as bench.py does, before anything here touches the GPU) and returns its exit code;
under torch.distributed.run it is one rank, and rank 0 prints the JSON line with `ranks`, `backend` and the mean
milliseconds per solve spent in send + merge + broadcast.  `--backend gloo --single-device` rehearses on one GPU."""
import argparse
import importlib
import json
import os
import sys
import time

t_proc = time.perf_counter()

ap = argparse.ArgumentParser()
ap.add_argument('--n', type=int, default=708)
ap.add_argument('--steps', type=int, default=10)
ap.add_argument('--element', default='P1')
ap.add_argument('--rtol', type=float, default=1e-10)
ap.add_argument('--forcing', type=float, default=0.0, help='inexact Newton: linear rtol = forcing * previous Newton criterion (0 = fixed rtol)')
ap.add_argument('--inexact', type=float, default=0.0, help='constant relative tolerance of every linear solve inside the Newton loop (0 = off)')
ap.add_argument('--cap', type=float, default=1e-4, help='loosest linear tolerance the forcing term may ask for')
ap.add_argument('--solver', default='amg', help='pcg (block-Jacobi CG) | amg (multigrid-preconditioned CG) | direct')

ap.add_argument('--cold', action='store_true', help='leave the library load (with `import torch`) and the HIP runtime start inside the timed call, as the runs before round 3\'s last session did')
ap.add_argument('--ranks', type=int, default=1, help='number of processes, one per GPU (1 = the single-GPU driver)')
ap.add_argument('--backend', default='nccl', help='torch.distributed backend for --ranks > 1 (nccl = RCCL; gloo only to rehearse on one GPU)')
ap.add_argument('--single-device', action='store_true', help='--ranks > 1: every rank on GPU 0 (rehearsal, with --backend gloo)')
# (the ranks get their arguments through the environment: torch.distributed.run reads `--n` as an abbreviation of its own options)
a = ap.parse_args(json.loads(os.environ['FEP_NEWTON_BENCH_ARGV']) if 'FEP_NEWTON_BENCH_ARGV' in os.environ else None)
if a.ranks > 1 and 'WORLD_SIZE' not in os.environ:
    import socket
    import subprocess
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, FEP_NEWTON_BENCH_ARGV=json.dumps(sys.argv[1:]))
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    env.setdefault('OMP_NUM_THREADS', str(max(1, (os.cpu_count() or 8) // a.ranks)))
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', f'--nproc-per-node={a.ranks}',
           '--master-addr', '127.0.0.1', '--master-port', str(port), os.path.abspath(__file__)]
    sys.exit(subprocess.run(cmd, env=env).returncode)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
fep = importlib.import_module('fem-elastoplasticity_amd')
rank = 0
if a.ranks > 1:
    import torch
    import torch.distributed as dist
    if int(os.environ['WORLD_SIZE']) != a.ranks:
        raise SystemExit(f'--ranks {a.ranks} but WORLD_SIZE={os.environ["WORLD_SIZE"]}')
    if a.solver not in ('pcg', 'amg') or a.forcing:
        raise SystemExit('--ranks > 1 offers --solver pcg | amg and --inexact, not --forcing')
    local = 0 if a.single_device else int(os.environ.get('LOCAL_RANK', '0'))
    torch.cuda.set_device(local)
    os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    if a.backend == 'nccl':
        dist.init_process_group('nccl', device_id=torch.device('cuda', local))
    else:
        dist.init_process_group(a.backend)
    rank = dist.get_rank()
if not a.cold:
    # what a process pays once, whatever it goes on to compute: loading the library (which imports torch first, for its HIP
    # runtime) and starting the HIP runtime on the device.  Reported as `startup_s`, not part of `wall_s`.
    import torch
    fep.lib()
    torch.zeros(1, device='cuda')
    torch.cuda.synchronize()
t_start = time.perf_counter() - t_proc

lines = []
t0 = time.perf_counter()


def log(s):
    lines.append(s)
    print(f'[{time.perf_counter() - t0:8.2f}s] {s}', flush=True)


if a.ranks > 1:
    h = fep.solve_strip_footing_sharded(a.element, n_cells=a.n, max_steps=a.steps, linear_solver=a.solver, pcg_rtol=a.rtol,
                                        pcg_inexact_rtol=a.inexact or None, keep_U=False, device=torch.cuda.current_device(),
                                        timed=a.solver == 'amg', log=log if rank == 0 else None)
else:
    h = fep.solve_strip_footing(a.element, n_cells=a.n, max_steps=a.steps, linear_solver=a.solver, pcg_rtol=a.rtol,
                                pcg_forcing=a.forcing or None, pcg_forcing_cap=a.cap, pcg_inexact_rtol=a.inexact or None,
                                keep_U=False, log=log)
t = time.perf_counter() - t0
it = h['pcg_iters'] or []
extra = {}
if a.ranks > 1:
    gs = h.get('gathered_solve')
    extra = {'ranks': a.ranks, 'backend': a.backend, 'solver': a.solver,
             'gather_ms_per_solve': None if not gs else 1e3 * (gs['send'] + gs['merge'] + gs['broadcast']) / max(1, gs['n_solves']),
             'gather_phases_ms_per_solve': None if not gs else {k: 1e3 * gs[k] / max(1, gs['n_solves']) for k in ('send', 'merge', 'solve', 'broadcast')}}
    dist.barrier()
    dist.destroy_process_group()
    if rank != 0:
        sys.exit(0)
print(json.dumps({'n_cells': a.n, 'element': a.element, 'elements': int(h['mesh']['elements'].shape[1]),
                  'accepted_steps': len(h['zeta']), 'hot_path_calls': h['n_calls'], 'newton_its': h['newton_its'],
                  'wall_s': t, 'startup_s': t_start, 'cold': bool(a.cold), 'linear_solves': len(it), 'pcg_iters_total': int(sum(it)),
                  'pcg_iters_max': int(max(it)) if it else None, 'pcg_iters': [int(v) for v in it], 'zeta': h['zeta'], 'pressure': h['pressure'],
                  'counts': h['counts'], **extra}))
