"""
What a context runs on each route, named as fep_ctx_kernel_names prints it: the tests that select a route with FEP_ROUTE
assert it on every context they create, so that a switch the library ignores fails the test instead of running the
default route twice.
  node    P1 only (default): p1_point_kernel + p1_node_lds_kernel<256, rng, 1, true>; the K,F-only step p1_fused_kernel<...>
  patch   the element route's patch form (default for P2, Q1, Q2, P4; FEP_ROUTE=patch for P1): element_kernel + fixup_kernel
  coo     FEP_ROUTE=coo: element_kernel without the patch plan + csr_reduce_pk_kernel (K_e through HBM)
"""
NPQ = {'P1': (3, 1), 'P2': (6, 7), 'Q1': (4, 4), 'Q2': (8, 9), 'P4': (15, 12)}
# element_kernel's geometry from the coordinates (true) or from the dphi arrays (false), fixed per type and form
# (fep_api.hip: elem_geo_default)
GEO = {'patch': {'P1': 'false', 'P2': 'true', 'Q1': 'true', 'Q2': 'true', 'P4': 'true'},
       'coo': {'P1': 'false', 'P2': 'false', 'Q1': 'true', 'Q2': 'true', 'P4': 'false'}}
PATCH_TPB = {'P2': 512}                                 # threads per workgroup of the patch form (others: 256)


def route_kernels(t, route):
    """The exact kernel names of a full-output step of element type t on the element route's `route` form."""
    n_p, n_q = NPQ[t]
    if route == 'patch':
        return f'element_kernel<{n_p}, {n_q}, true, {GEO[route][t]}, true, {PATCH_TPB.get(t, 256)}, 1> + fixup_kernel'
    if route == 'coo':
        return f'element_kernel<{n_p}, {n_q}, true, {GEO[route][t]}, false, 256, 1> + csr_reduce_pk_kernel'
    raise ValueError(route)


def assert_route(ctx, route):
    """ctx runs `route` (node | patch | coo); for the node route, its K,F-only step is the one-kernel step."""
    t = ctx.element_type.name
    got = ctx.kernel_names(0)
    if route == 'node':
        assert t == 'P1' and got.startswith('p1_point_kernel + p1_node_lds_kernel<256, ') and got.endswith(', 1, true>'), got
        kf = ctx.kernel_names(1)
        assert kf.startswith('p1_fused_kernel<false, 256, '), kf
    else:
        assert got == route_kernels(t, route), (route, got)
        assert ctx.kernel_names(1) == got
