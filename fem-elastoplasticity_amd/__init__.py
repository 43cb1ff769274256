"""
MI355X-native implementation of the hot path of MartinBeseda/FEM-ElastoPlasticity:
Drucker-Prager return map + tangent-stiffness / internal-force assembly, as hand-written
HIP kernels behind a C ABI (include/fep.h), with a Python host layer that keeps the
reference's function names and signatures.

The directory name contains a hyphen; import it with
    fep = importlib.import_module('fem-elastoplasticity_amd')

Flavours of the reference's three `pythonFEM.py` copies:
    fep.plasticity2d_dp   Plasticity2D_DP/pythonFEM.py   (P1, P2, Q1, Q2)
    fep.tsx_tunnel        tsx-tunnel/pythonFEM.py        (adds e0 and P4)
    fep.elasticity2d      Elasticity2D/pythonFEM.py      (P1, Q1, Q2; external loads)
"""
from .tables import (ELEMENT_SHAPE, LagrangeElementType, element_tables, get_local_basis_surface,
                     get_local_basis_volume, get_quadrature_surface, get_quadrature_volume, surface_tables)
from .mesh import assemble_mesh, assemble_mesh_el, rect_mesh, renumber_for_locality, square_mesh
from .hotpath import (MeshContext, assemble_tangent, construct_constitutive_problem,
                      construct_constitutive_problem_tsx, construct_constitutive_problem_vm, construct_constitutive_problem_mc,
                      construct_constitutive_problem_vmps, construct_constitutive_problem_vmi,
                      construct_constitutive_problem_field, in_situ_strain, linear_in_situ, default_device, get_elastic_stiffness_matrix,
                      get_elastic_stiffness_matrix_el, get_vector_traction, get_vector_volume, load_traction)
from .elastic import solve_elasticity2d
from .vonmises import solve_cutout_cyclic
from .hardening import hardening_curve, voce_curve
from ._lib import FepError, lib, lib_path
from .build import build
from .sharding import GatherPlan, Partition, ShardedContext, element_ranges, global_pattern, merge_host
from .newton import solve_strip_footing, solve_tsx_tunnel, transform
from .solver import KrylovSolver, build_amg_hierarchy
from .dist_newton import DistributedPCG, GatheredSolver, solve_strip_footing_sharded, solve_tsx_tunnel_sharded
from .midpoints import (DeviceMesh, Ellipse, area_stats, area_stats_dev, create_midpoints, create_midpoints_P2, create_midpoints_P4,
                        mark_plastic, refine_marked, refine_uniform)
from .estimate import estimate_np, indicator_stats, mark_bulk, recover_stress_np, tree_sum
from .midpoints import child_corners
from .transfer import (transfer_nodes, transfer_nodes_dev, transfer_nodes_np, transfer_points, transfer_points_dev,
                       transfer_points_np, transfer_tables, uniform_corners)
from .meshio import dump_free_dof_csv, load_tsx_mesh, prepare_tsx_mesh
from . import plasticity2d_dp, tsx_tunnel, elasticity2d, vonmises, transfer

__all__ = ['LagrangeElementType', 'ELEMENT_SHAPE', 'get_quadrature_volume', 'get_local_basis_volume',
           'element_tables', 'assemble_mesh', 'square_mesh', 'rect_mesh', 'renumber_for_locality', 'Partition', 'ShardedContext', 'element_ranges', 'GatherPlan', 'global_pattern', 'merge_host', 'MeshContext', 'construct_constitutive_problem',
           'construct_constitutive_problem_tsx', 'get_elastic_stiffness_matrix', 'get_elastic_stiffness_matrix_el',
           'assemble_tangent', 'default_device', 'FepError', 'lib', 'lib_path', 'build',
           'solve_strip_footing', 'solve_tsx_tunnel', 'transform', 'KrylovSolver', 'DistributedPCG', 'solve_strip_footing_sharded', 'GatheredSolver', 'solve_tsx_tunnel_sharded', 'build_amg_hierarchy', 'create_midpoints', 'create_midpoints_P2',
           'create_midpoints_P4', 'refine_uniform', 'refine_marked', 'mark_plastic', 'DeviceMesh', 'Ellipse', 'area_stats', 'area_stats_dev', 'load_tsx_mesh', 'prepare_tsx_mesh', 'dump_free_dof_csv',
           'get_quadrature_surface', 'get_local_basis_surface', 'surface_tables', 'assemble_mesh_el', 'get_vector_volume',
           'get_vector_traction', 'load_traction', 'solve_elasticity2d',
           'construct_constitutive_problem_vm', 'construct_constitutive_problem_mc', 'construct_constitutive_problem_vmps',
           'construct_constitutive_problem_vmi', 'hardening_curve', 'voce_curve',
           'solve_cutout_cyclic',
           'construct_constitutive_problem_field', 'in_situ_strain', 'linear_in_situ',
           'tree_sum', 'recover_stress_np', 'estimate_np', 'indicator_stats', 'mark_bulk',
           'child_corners', 'uniform_corners', 'transfer_tables', 'transfer_nodes_np', 'transfer_points_np', 'transfer_nodes',
           'transfer_points', 'transfer_nodes_dev', 'transfer_points_dev',
           'plasticity2d_dp', 'tsx_tunnel', 'elasticity2d', 'vonmises', 'transfer']
