"""Shared by test_vm_ref_host.py and test_vm_gpu.py: the materials of the cyclic benchmark, the top-side load of the cut-out
square built on the host, and the CPU runs of the cyclic driver (computed once per session and never modified)."""
import functools
from importlib import import_module

import numpy as np

from conftest import ROOT  # noqa: F401  (puts the repository root on sys.path)
import loads_ref
from vm_ref import VMRefContext

fep = import_module('fem-elastoplasticity_amd')

YOUNG, POISSON, SIGMA_Y, HARDENING = 206900.0, 0.29, 450.0, 10000.0
SHEAR = YOUNG / (2 * (1 + POISSON))
BULK = YOUNG / (3 * (1 - 2 * POISSON))
YIELD = np.sqrt(2 / 3) * SIGMA_Y


def top_load(element_type, level, traction):
    """(2, n_n) load vector of the uniform `traction` on the top side of the cut-out square, summed on the host
    (tests/loads_ref.py; for P1 this is half an edge per end node)."""
    t = fep.LagrangeElementType[element_type]
    mesh = fep.assemble_mesh_el(level, t)
    edges = mesh['neumann_nodes'].astype(np.int64)
    hatp_s, dhatp1_s, wf_s = fep.surface_tables(t)
    t_int = np.repeat(np.asarray(traction, dtype=float).reshape(2, 1), edges.shape[1] * np.size(wf_s), axis=1)
    return loads_ref.traction(edges, mesh['coordinates'], t_int, hatp_s, dhatp1_s, wf_s)[0]


@functools.lru_cache(maxsize=None)
def cpu_cycle(element_type, peak):
    """solve_cutout_cyclic at level 0 on the CPU restatement with the sparse direct solve."""
    return fep.solve_cutout_cyclic(element_type, level=0, context_factory=VMRefContext, linear_solver='direct',
                                   f_ext=top_load(element_type, 0, (0, peak)))
