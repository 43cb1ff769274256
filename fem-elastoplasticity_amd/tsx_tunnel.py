"""Names of tsx-tunnel/pythonFEM.py that sit on the hot path, with identical signatures
(the return map takes the initial strain `e0` as second argument, TSX:990-991)."""
from .tables import LagrangeElementType, get_local_basis_volume, get_quadrature_volume   # noqa: F401  TSX:57-274
from .hotpath import assemble_tangent, get_elastic_stiffness_matrix                      # noqa: F401  TSX:432-542
from .hotpath import construct_constitutive_problem_tsx as construct_constitutive_problem  # noqa: F401  TSX:990-1157
from .midpoints import create_midpoints, create_midpoints_P2, create_midpoints_P4                 # noqa: F401  TSX:1354-1633
from .midpoints import DeviceMesh, Ellipse, refine_uniform                               # noqa: F401  uniform refinement: no counterpart
from .meshio import load_tsx_mesh, prepare_tsx_mesh                                      # noqa: F401  TSX:1687-1690
from .newton import solve_tsx_tunnel                                                     # noqa: F401  TSX:1637-1832

# The tunnel wall of the reference's mesh (coord.csv): its 25 nodes lie on this ellipse to |g - 1| <= 2.0e-5 (a least-squares
# fit gives the semi-axes 2.187505 / 1.749993).  Pass `curves=[TSX_HOLE]` to refine / enrich onto the wall, not its 25-gon.
TSX_HOLE = Ellipse(0.0, 0.0, 2.1875, 1.75, 1e-3)
