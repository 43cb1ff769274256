"""Names of Elasticity2D/pythonFEM.py, the whole flavour: tables, cut-out mesh, `get_elastic_stiffness_matrix` (returns
(K, weight) and shifts the 1-based `elements` in place, EL:389, EL:477), both load vectors and the driver.  The flavour is
plane strain, as the reference's; an elastic plane-stress stiffness is the K at U = 0 of a context with `set_model('vmps')`."""
from .tables import (LagrangeElementType, get_local_basis_surface, get_local_basis_volume,       # noqa: F401  EL:49-243
                     get_quadrature_surface, get_quadrature_volume)
from .mesh import assemble_mesh_el as assemble_mesh                                               # noqa: F401  EL:481-942
from .hotpath import get_elastic_stiffness_matrix_el as get_elastic_stiffness_matrix             # noqa: F401  EL:368-477
from .hotpath import get_vector_traction, get_vector_volume                                       # noqa: F401  EL:246-364
from .elastic import elasticity_fem                                                               # noqa: F401  EL:1052-1179
