/*
 * fep.h — C ABI of libfep_hip.so: the MI355X (gfx950) implementation of the
 * reference's per-integration-point Drucker–Prager return map and per-element
 * tangent-stiffness / internal-force assembly.
 *
 * The reference (MartinBeseda/FEM-ElastoPlasticity) is pure Python and has no FFI;
 * its "operator interface" for this path is a set of module-level functions.
 * Each entry point below names the reference lines it replaces
 * (DP = Plasticity2D_DP/pythonFEM.py, TSX = tsx-tunnel/pythonFEM.py,
 *  EL = Elasticity2D/pythonFEM.py).  INTEGRATION.md shows the ctypes stubs.
 *
 * Conventions
 *   - every function returns 0 (FEP_OK) or a negative FEP_E* code; nothing throws or aborts;
 *   - `double` is IEEE fp64; node/element indices are int32_t, 0-based; sizes are int64_t;
 *   - integration point id  k = e*n_q + q  (q fastest)                       DP:510-511,526-527
 *   - DOF id = 2*node + comp (U, F are the column-major flattening of (2,n_n)) DP:560-565, DP:1043
 *   - strain/stress 3-vectors [11,22,12(engineering)], 4-vectors [11,22,12,33] DP:651
 *   - per-point arrays are "rows x n_int", C-contiguous (component-major, SoA),
 *     exactly the reference's (4,n_int)/(9,n_int) NumPy arrays;
 *   - `ds` holds the 3x3 consistent tangent row-major, m = 3*i + j            DP:703
 *   - pointers named *_h are host memory, *_d are device (HBM) memory of the
 *     context's GPU; the caller owns every pointer for the duration of the call;
 *   - device vectors indexed by DOF or by CSR position (U, F, k_data, the solver's x, b, y) must be 16-byte
 *     aligned (hipMalloc and every tensor library deliver that; checked, FEP_EINVAL otherwise): the kernels move
 *     them as (x, y) pairs;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); *_dev
 *     calls only enqueue work and return, *_host calls are synchronous (all but fep_load_traction_host run on a stream of
 *     the library's own, with pinned staging; the context and return-map forms keep their device buffers, so they allocate
 *     nothing per call after the first, the mesh forms use device blocks of the call);
 *   - calls on one context are not re-entrant; one context per (host thread, GPU).
 *
 * Stream contract of the *_host entry points that move the caller's arrays through the staging engine
 * (fep_return_map_host / _vm_host / _mc_host / _vmps_host / _vmi_host / _field_host, fep_step_host / _host_planar / _field_host, fep_assemble_host,
 * fep_transform_host, fep_load_volume_host, fep_ctx_point_coords_host, fep_recover_stress_host, fep_estimate_host,
 * fep_mesh_enrich_host, fep_mesh_refine_host, fep_mesh_refine_marked_host, fep_mesh_surf_curve_host, fep_mesh_area_stats_host,
 * fep_mark_bulk_host; not fep_load_traction_host, which allocates per call and copies on the default stream):
 *   - each call runs its copies and its kernels on ONE non-blocking stream per device that belongs to the library; that stream
 *     is ordered against nothing else: not the default stream, not a stream the caller passed to a *_dev call;
 *   - calls of all host threads on one device are serialised by a lock, and a call returns only after synchronising that
 *     stream: on return every output is complete in the caller's memory, every input may be reused or freed, and nothing of
 *     the call is in flight;
 *   - a host array may lie anywhere and needs no more than its element's alignment: a block from fep_host_alloc, or a view
 *     into one, is DMA-ed from / to directly, every other pointer goes through the engine's ring of pinned slots in chunks of
 *     8 MiB, whatever its length;
 *   - the context forms launch the same kernels as the *_dev forms and share the context's scratch with them (the ds / s scratch
 *     of the assembly, the branch counters' per-workgroup partials, a von Mises / Mohr-Coulomb context's point scratch), next
 *     to device buffers of their own that persist in the context (the first call that needs a larger one waits for the whole
 *     device before it frees the smaller).
 *   So: BEFORE a *_host call on a context, every *_dev call issued on that context must have COMPLETED: synchronise the
 *   stream(s) they were enqueued on (fep_sync, hipStreamSynchronize, an event the host waited for).  Being enqueued earlier
 *   is not enough, since the library's stream waits for no other.  AFTER a *_host call has returned, a *_dev call on the same
 *   context may be enqueued at once on any stream.  tests/test_host_staging_gpu.py runs exactly this alternation.
 *   The mesh-free fep_return_map_*_host calls use the engine's own device buffers and the counter scratch of the engine's
 *   stream only: they need no synchronisation against *_dev calls of any kind.
 *   The mesh forms (the last six of the list) use device blocks of the call: their outputs are as large as the
 *   mesh and a driver makes one mesh per level, so every call allocates its blocks and frees them before it returns, and
 *   nothing persists.  No *_dev call needs synchronising against them either: they only read the mesh, and what writes it
 *   (fep_mesh_create, fep_mesh_mark) synchronises before it returns.  Their kernel scratch (area statistics, the indicator's
 *   partials) is that of the engine's stream.  fep_mesh_child_corners_host, fep_transfer_nodes_host and
 *   fep_transfer_points_host follow the mesh forms in all of this (the owners of the node transfer are such kernel scratch).
 */
#ifndef FEP_H
#define FEP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FEP_OK            0
#define FEP_EINVAL       -1   /* bad argument (NULL pointer, negative size, unknown element type) */
#define FEP_ENODEV       -2   /* no usable HIP device / hipSetDevice failed */
#define FEP_ENOMEM       -3   /* host or device allocation failed */
#define FEP_EHIP         -4   /* a HIP runtime call or kernel launch failed (see fep_last_hip_error) */
#define FEP_ERANGE       -5   /* an index is out of range (element -> node id, 32-bit offset overflow, a node row of
                                 * more than 256 blocks: fep_ctx_create) */
#define FEP_ESTATE       -6   /* call order violated (e.g. materials not set) */

/* LagrangeElementType values of the reference (DP:55-60, TSX:57-63) */
#define FEP_P1 1
#define FEP_P2 2
#define FEP_Q1 3
#define FEP_Q2 4
#define FEP_P4 5

/* material models of a mesh context (fep_ctx_set_model) */
#define FEP_MODEL_DP 0        /* perfectly plastic Drucker-Prager (the reference's law; the default) */
#define FEP_MODEL_VM 1        /* von Mises with linear kinematic hardening (no reference counterpart) */
#define FEP_MODEL_MC 2        /* associative, perfectly plastic Mohr-Coulomb (no reference counterpart) */
#define FEP_MODEL_VMPS 3      /* von Mises with linear kinematic hardening in plane stress (no reference counterpart) */
#define FEP_MODEL_VMI 5       /* von Mises with isotropic hardening on a piecewise-linear curve next to the kinematic one, plane
                                * strain (no reference counterpart).  4 is not a model and is refused */
#define FEP_MAX_HARDENING_SEGMENTS 8   /* segments of a hardening curve (fep_return_map_vmi_*, fep_ctx_set_hardening) */

typedef struct fep_ctx fep_ctx;

/* ---- library ------------------------------------------------------------------------ */
int         fep_version(void);                 /* ABI version, currently 1 */
int         fep_build_is_ablation(void);       /* 1: built with -DFEP_ABLATION (measurement switches by environment variable, phase
                                                * clocks; tools/ only), 0: the product library, which reads FEP_ROUTE,
                                                * FEP_VALIDATE_PLAN, FEP_VERBOSE, FEP_HOST_THREADS, FEP_COPY_THREADS and nothing else */
const char* fep_strerror(int code);
int         fep_last_hip_error(void);          /* raw hipError_t of the last FEP_EHIP on this thread */
int         fep_device_count(int* n_out);
/* (n_p, n_q) of an element type; FEP_EINVAL if unknown.  Tables: DP:364-488, TSX:67-274. */
int         fep_element_shape(int elem_type, int* n_p, int* n_q);

/* ---- device memory helpers (for callers that do not bring their own allocator) ------- */
int fep_malloc(int device_id, void** ptr_d, int64_t bytes);
int fep_free(int device_id, void* ptr_d);
int fep_memcpy_h2d(int device_id, void* dst_d, const void* src_h, int64_t bytes);
int fep_memcpy_d2h(int device_id, void* dst_h, const void* src_d, int64_t bytes);
int fep_sync(int device_id, void* stream);
/* Page-locked host memory from a size-keyed cache (a returned block is reused by the next request of the same size;
 * up to 4 GiB stay cached).  The *_host entry points DMA straight from / into such blocks; any other host pointer is
 * staged through a ring of pinned slots filled by copy threads (FEP_COPY_THREADS, default 8).  The Python layer
 * places every output array it hands to the caller (s, ds, ind_p, K data, F: DP:1044-1058) in such blocks. */
int fep_host_alloc(void** ptr_h, int64_t bytes);
int fep_host_free(void* ptr_h);     /* FEP_EINVAL for a pointer that is not a live block of the cache (e.g. freed twice) */
/* Unpins and frees every cached (idle) block.  fep_host_alloc does this by itself, once, before it reports FEP_ENOMEM. */
int fep_host_trim(void);

/* ---- a2: return map, mesh-free (pointwise) --------------------------------------------
 * Replaces construct_constitutive_problem, DP:604-757 (e0_h == NULL) and TSX:990-1157
 * (e0_h = the broadcast (4,1) initial strain).
 *
 *   e          strain, component i of point k at e[k*e_pt_stride + i*e_comp_stride]
 *              ((3,n_int) C-order: (1, n_int); the driver's F-ordered array DP:1043: (3, 1)); never modified
 *   ep_prev    (4,n_int) or NULL (= zeros, DP:667).  If `accept` != 0 it is UPDATED IN PLACE
 *              (the reference returns the mutated `ep_prev` as 'ep', DP:751-755)
 *   shear,bulk,eta,c   (n_int) each
 *   s          out (4,n_int)   ds  out (9,n_int)   ind_p  out (n_int) 0/1 bytes
 *   counts     out [2] = {n_smooth, n_apex} (the numbers the reference logs at DP:730); may be NULL
 *
 * Non-finite inputs (all fep_return_map_* and, through them, fep_step_* and fep_assemble_*; tests/test_nonfinite_gpu.py).
 * A NaN or an infinity in a DATA array is legal input; indices, tables and sizes must always be valid.
 *   1. It is never hidden.  Von Mises (plane strain and plane stress) and Mohr-Coulomb: a point whose trial strain (e + e0) - ep_prev has a NaN component
 *      comes back with ind_p = 0, the elastic tangent, at least one NaN in s, its ep_prev untouched, and is counted nowhere
 *      (every branch test is written so that a NaN fails it: crit > 0, !(f > 0)).  Drucker-Prager does what the reference
 *      does: its products with the zeros of vol carry a non-finite shear strain into the trace, so a NaN in any strain
 *      component gives an elastic point with a NaN stress, while +Inf in a normal strain passes crit1 > 0 and crit2 > 0 and
 *      returns the apex's finite c / eta (DP:699): the reference's behaviour, kept.  A NaN in a material parameter is
 *      outside this rule: it shows in s or ds only where the formulas of the point's branch read that parameter.
 *   2. It is contained.  An output with no poisoned contributor (another point; in fep_step_*: a point of an element
 *      without the poisoned node, an F entry or a K block no such element contributes to) is bit for bit what the same
 *      call without the poison returns.  ds stays finite (the elastic tangent), so all of K does.
 *   3. The solvers report it promptly: fep_solver_pcg_dev / fep_solver_amg_pcg_dev (below).
 *   4. It leaves no trace: the same clean call on the same context, solver and hierarchy afterwards returns the same bits
 *      as before (the ds / s scratch, the counters' scratch and the refreshed coarse operators are overwritten whole).
 */
int fep_return_map_host(int device_id, int64_t n_int,
                        const double* e_h, int64_t e_pt_stride, int64_t e_comp_stride,
                        const double* e0_h, double* ep_prev_h,
                        const double* shear_h, const double* bulk_h, const double* eta_h, const double* c_h,
                        int accept,
                        double* s_h, double* ds_h, uint8_t* ind_p_h, int64_t* counts_h);

/* Same on device-resident arrays.  `counts_d` (2 x int64, device) is zeroed and filled by the call.  With counts_d the
 * call uses a per-(device, stream) scratch of 8 bytes per 256 points that grows on demand (FEP_ESTATE if it would have to
 * grow while the stream is being captured: run the call once outside the capture first); a block handed out is never
 * freed, so a HIP graph captured from this call stays valid for calls of up to the captured n_int. */
int fep_return_map_dev(int device_id, void* stream, int64_t n_int,
                       const double* e_d, int64_t e_pt_stride, int64_t e_comp_stride,
                       const double* e0_h, double* ep_prev_d,
                       const double* shear_d, const double* bulk_d, const double* eta_d, const double* c_d,
                       int accept,
                       double* s_d, double* ds_d, uint8_t* ind_p_d, int64_t* counts_d);

/* ---- second material model: von Mises with linear kinematic hardening, mesh-free -------
 * No reference counterpart.  Plane strain, radial return with the symmetric consistent tangent; layout, strides, e0_h,
 * ep_prev (NULL = zeros; updated in place when `accept`), outputs and the scratch rule of counts_d exactly as
 * fep_return_map_*, with the parameters
 *   a   (n_int) kinematic hardening modulus, >= 0        Y   (n_int) yield radius sqrt(2/3)*sigma_y, > 0
 * in the places of eta and c.  Per point, with p = ep_prev (engineering shear in p[2]) and z = e0:
 *     Et = (e, 0) + z - p                    tr = Et0 + Et1 + Et3
 *     dv = (Et0 - tr/3, Et1 - tr/3, Et2/2, Et3 - tr/3)
 *     s_tr = 2G*dv + K*tr*(1,1,0,1)
 *     xi = 2G*dv - a*(p0, p1, p2/2, p3)      nrm = sqrt(xi0^2 + xi1^2 + 2 xi2^2 + xi3^2)      crit = nrm - Y
 *     crit <= 0:  s = s_tr,  ds = 2G*Dev + K*Vol (the elastic tangent of the Drucker-Prager map)
 *     crit >  0:  lambda = crit/(2G + a),  N = xi/nrm,  s = s_tr - 2G*lambda*N,
 *                 ds = 2G*Dev + K*Vol - (2G)^2/(2G+a) N(x)N - (2G)^2*lambda/nrm (Dev - N(x)N)     (rows / columns 11, 22, 12)
 *                 accept:  p += lambda*(N0, N1, 2 N2, N3)
 * ind_p = (crit > 0); counts = {number of plastic points, 0}.  The back stress is a*p: the plastic strain is the only
 * state.  ds is symmetric, so fep_assemble_* takes it as it is. */
int fep_return_map_vm_host(int device_id, int64_t n_int,
                           const double* e_h, int64_t e_pt_stride, int64_t e_comp_stride,
                           const double* e0_h, double* ep_prev_h,
                           const double* shear_h, const double* bulk_h, const double* a_h, const double* y_h,
                           int accept,
                           double* s_h, double* ds_h, uint8_t* ind_p_h, int64_t* counts_h);
int fep_return_map_vm_dev(int device_id, void* stream, int64_t n_int,
                          const double* e_d, int64_t e_pt_stride, int64_t e_comp_stride,
                          const double* e0_h, double* ep_prev_d,
                          const double* shear_d, const double* bulk_d, const double* a_d, const double* y_d,
                          int accept,
                          double* s_d, double* ds_d, uint8_t* ind_p_d, int64_t* counts_d);

/* ---- third material model: associative, perfectly plastic Mohr-Coulomb, mesh-free ------
 * No reference counterpart.  Plane strain, the closest-point return map in principal stresses (elastic, smooth face, two
 * edges, apex) with its spectral tangent; layout, strides, e0_h, ep_prev, outputs and the scratch rule of counts_d
 * exactly as fep_return_map_*, with the parameters
 *   sin_phi (n_int) sine of the friction angle, in (0, 1)        c (n_int) cohesion, > 0
 * in the places of eta and c (the bounds are a precondition, as eta > 0 is for Drucker-Prager).  Yield function,
 * tension positive, sig1 >= sig2 >= sig3:  (1+s) sig1 - (1-s) sig3 - 2 c cos(phi) <= 0,  s = sin_phi, cos = sqrt(1-s^2).
 * Per point, with lam = K - 2G/3:
 *     Et = (e, 0) + z - p                    tr = Et0 + Et1 + Et3
 *     m = (Et0+Et1)/2, dd = (Et0-Et1)/2, h = Et2/2, r = sqrt(dd^2 + h^2)      ea = m + r, eb = m - r, ez = Et3
 *     (where max(|dd|, |h|) < 2^-500, dd and h are scaled by 2^600 for r, ca and sa: the squares stay out of the denormal range)
 *     ca = dd/r, sa = h/r (1, 0 at r = 0)    Pa = ((1+ca)/2, (1-ca)/2, sa/2), Pb = ((1-ca)/2, (1+ca)/2, -sa/2)
 *     (e1, e2, e3) = (ea, eb, ez) sorted descending and stable
 *     f = 2G[(1+s)e1 - (1-s)e3] + 2 lam s tr - 2c cos;          not f > 0 (f <= 0 or NaN): elastic (branch 0), L = 0
 *     g_sl = (e1-e2)/(1+s), g_sr = (e2-e3)/(1-s), g_la = (e1+e2-2e3)/(3-s), g_ra = (2e1-e2-e3)/(3+s)
 *   Every plastic branch but the apex is one formula on its normal n and its strains t:
 *     A n = 2G n + 2 lam s,  den = n.A n = 2G|n|^2 + 4 lam s^2,  L = (2G n.e + 2 lam s tr - 2c cos)/den,
 *     sig = lam tr + 2G t - L A n,        dsig/deps = lam + G M - (A n)(A n)^T/den
 *     1 smooth      L <= min(g_sl, g_sr):             n = (1+s, 0, -(1-s)),          t = e,  M = 2I
 *     2 left edge   g_sl < g_sr,  L <= g_la:           n = ((1+s)/2, (1+s)/2, -(1-s)), t = ((e1+e2)/2, (e1+e2)/2, e3),
 *                                                     M = [[1,1,0],[1,1,0],[0,0,2]]                      (sig1 = sig2)
 *     3 right edge  g_sl >= g_sr, L <= g_ra:           n = (1+s, -(1-s)/2, -(1-s)/2),  t = (e1, (e2+e3)/2, (e2+e3)/2),
 *                                                     M = [[2,0,0],[0,1,1],[0,1,1]]                      (sig2 = sig3)
 *     4 apex        otherwise:                        sig_i = c cos/s,  dsig/deps = 0
 *   Back through the permutation to (sig_a, sig_b, sig_z) and D over (a, b, z):
 *     (s11, s22, s12) = sig_a Pa + sig_b Pb,  s33 = sig_z
 *     ds = D_aa Pa Pa^T + D_ab (Pa Pb^T + Pb Pa^T) + D_bb Pb Pb^T + theta (diag(1, 1, 1/2) - Pa Pa^T - Pb Pb^T),
 *     theta = (sig_a - sig_b)/(2r) = G [(t_a - t_b) - L (n_a - n_b)]/r  (D_aa - D_ab at r = 0, 0 at the apex), formed from the
 *     difference itself: t_a - t_b is 2r unless the branch is an edge, so an elastic point has theta = 2G exactly and an edge
 *     that merges a and b theta = 0 exactly, whatever r                                  (rows / columns 11, 22, 12)
 *   accept, plastic points:  th = (sig_a+sig_b+sig_z)/(3K),  dp_i = e_i - (sig_i - lam th)/(2G) over (a, b, z),
 *     p += (dp_a Pa0 + dp_b Pb0,  dp_a Pa1 + dp_b Pb1,  2 (dp_a Pa2 + dp_b Pb2),  dp_z)
 * (An edge's L >= g_sl resp. g_sr needs no test: den (L - g) of the edge equals den (L - g) of the failed smooth test.)
 * ind_p = (branch != 0); counts = {smooth face + both edges, apex}.  ds is symmetric.  On the smooth face theta loses the
 * digits of max|Et| / r as r -> 0 (2r - L (n_a - n_b) is then a difference of two rounded numbers; nowhere else), and a point
 * within rounding of a branch boundary may take either side (s is continuous there). */
int fep_return_map_mc_host(int device_id, int64_t n_int,
                           const double* e_h, int64_t e_pt_stride, int64_t e_comp_stride,
                           const double* e0_h, double* ep_prev_h,
                           const double* shear_h, const double* bulk_h, const double* sin_phi_h, const double* c_h,
                           int accept,
                           double* s_h, double* ds_h, uint8_t* ind_p_h, int64_t* counts_h);
int fep_return_map_mc_dev(int device_id, void* stream, int64_t n_int,
                          const double* e_d, int64_t e_pt_stride, int64_t e_comp_stride,
                          const double* e0_h, double* ep_prev_d,
                          const double* shear_d, const double* bulk_d, const double* sin_phi_d, const double* c_d,
                          int accept,
                          double* s_d, double* ds_d, uint8_t* ind_p_d, int64_t* counts_d);

/* ---- fourth material model: von Mises with linear kinematic hardening in PLANE STRESS, mesh-free ------
 * No reference counterpart.  The law of fep_return_map_vm_* with the out-of-plane strain left free (s33 = 0) instead of
 * prescribed: for a traceless ep_prev, fep_return_map_vm_* at the e0[3] that makes its s[3] vanish returns the same
 * in-plane stress and the same new ep_prev.  Layout, strides, e0_h, ep_prev, outputs, the parameters a >= 0 and
 * Y = sqrt(2/3)*sigma_y > 0 and the scratch rule of counts_d exactly as fep_return_map_vm_*.  Per point, with p = ep_prev
 * (engineering shear in p[2]) and z = e0:
 *     ee_i = (e_i + z_i) - p_i, i = 0..2     lam = K - 2G/3,  lb = 2G lam/(lam + 2G)
 *     C = [[lb+2G, lb, 0], [lb, lb+2G, 0], [0, 0, G]]      st = C ee  (trial stress; C is the elastic tangent)
 *     ab = a (2 p0 + p1, 2 p1 + p0, p2/2)                  (plane-stress image of the deviatoric back stress a p)
 *     eta = st - ab,   hs = eta0 + eta1,  hd = eta0 - eta1,  h12 = eta2
 *     P = (1/3) [[2,-1,0],[-1,2,0],[0,0,6]]:   eta^T P eta = hs^2/6 + hd^2/2 + 2 h12^2  (= |dev xi|^2)
 *     cs = (2 lb + 2G)/3 + a,   cd = 2G + a
 *     phi(g) = hs^2/(6 (1 + cs g)^2) + (hd^2/2 + 2 h12^2)/(1 + cd g)^2 - Y^2
 *   not phi(0) > 0 (phi(0) <= 0 or NaN): elastic, g = 0, s = (st, 0), ds = C.
 *   phi(0) > 0: g is the root of phi (convex and decreasing on g >= 0), by Newton's iteration from
 *     g0 = (sqrt(eta^T P eta)/Y - 1)/max(cs, cd), which lies left of the root, so the iterates increase monotonically;
 *     stopped when |dg| cd <= 2^-51 (1 + cd g) and after 16 iterations at the latest (8 is the most any tested point takes).
 *     hs' = hs/(1 + cs g),  hd' = hd/(1 + cd g),  eta' = ((hs' + hd')/2, (hs' - hd')/2, h12/(1 + cd g))
 *     dp = g P eta'  (engineering shear in row 2),    s = (st - C dp, 0), formed as ((1 + a g) eta' + ab, 0): the same
 *          stress (M P = I for ab = a M p, so the image of a (p + dp) is ab + a g eta'), without the cancellation of st - C dp,
 *          which loses the digits of the overshoot
 *     th = g/(1 + a g),  Xi = (C^-1 + th P)^-1: diagonal in the (sum, difference, shear) modes with the entries
 *          1/(1/(2 lb + 2G) + th/3),  1/(1/(2G) + th),  1/(1/G + 2 th)
 *     n = Xi P eta',   ds = Xi - n n^T/(eta'^T P n + a Y^2 (1 + a g))              (rows / columns 11, 22, 12; symmetric)
 *     accept:  p += (dp0, dp1, dp2, -(dp0 + dp1))
 * ind_p = (phi(0) > 0); counts = {number of plastic points, 0}.  s[3] is +0.0.  e0[3] and ep_prev[3] enter the law only
 * through the propagation of non-finite values: eta^T P eta and s[3] carry the term -|0 * (|ee0| + |ee1| + |ee2| + |z3 - p3|)|,
 * which is -0.0 and changes no bit of a finite result, and NaN when one of the four components of the trial strain is a NaN
 * or an infinity, so that rule 1 above holds for all four components, and an infinite strain leaves a NaN in s too. */
int fep_return_map_vmps_host(int device_id, int64_t n_int,
                             const double* e_h, int64_t e_pt_stride, int64_t e_comp_stride,
                             const double* e0_h, double* ep_prev_h,
                             const double* shear_h, const double* bulk_h, const double* a_h, const double* y_h,
                             int accept,
                             double* s_h, double* ds_h, uint8_t* ind_p_h, int64_t* counts_h);
int fep_return_map_vmps_dev(int device_id, void* stream, int64_t n_int,
                            const double* e_d, int64_t e_pt_stride, int64_t e_comp_stride,
                            const double* e0_h, double* ep_prev_d,
                            const double* shear_d, const double* bulk_d, const double* a_d, const double* y_d,
                            int accept,
                            double* s_d, double* ds_d, uint8_t* ind_p_d, int64_t* counts_d);

/* ---- fifth material model: von Mises with isotropic hardening on a piecewise-linear curve, mesh-free ------
 * No reference counterpart.  The law of fep_return_map_vm_* (plane strain, radial return, symmetric consistent tangent, the
 * kinematic back stress a*p) with a yield radius Y + R(kappa) that follows the accumulated plastic multiplier kappa along a
 * curve the caller enters, e.g. from a tensile test.  Layout, strides, e0_h, outputs, the parameters a >= 0 and
 * Y = sqrt(2/3)*sigma_y0 > 0 (the INITIAL radius) and the scratch rule of counts_d exactly as fep_return_map_vm_*.
 *
 * State.  ep_prev keeps its shape (4,n_int), with the rows (p11, p22, gamma12, kappa).  Plane-strain von Mises flow is
 * traceless, so p33 = -(p11 + p22) is implied and row 3 is free for kappa, the sum of the multipliers lambda (the equivalent
 * plastic strain is sqrt(2/3)*kappa).  NULL = zeros; updated in place when `accept`.
 *
 * Curve, uniform over the points of a call, in host memory in both forms (as e0_h):
 *   n_seg      1 .. FEP_MAX_HARDENING_SEGMENTS
 *   kappa_h    [n_seg] breakpoints: kappa[0] == 0, strictly increasing, finite
 *   slope_h    [n_seg] dR/dkappa of segment j = [kappa[j], kappa[j+1]), finite; the last segment extends to +infinity
 * The library forms R[0] = 0, R[j+1] = R[j] + slope[j]*(kappa[j+1] - kappa[j]) in double, in this order, without fused
 * multiply-add, and the kernel reads kappa, R and slope.  FEP_EINVAL for a curve that is not as stated.  Preconditions on the
 * caller (as eta > 0 is for Drucker-Prager):  2G + a + slope[j] > 0 for every j and every point (softening is allowed within
 * that), and Y + R(kappa) > 0 wherever the state gets.
 *
 * Per point, with p = ep_prev, k0 = p[3], p3 = -(p[0] + p[1]) and z = e0:
 *     Et, tr, dv, s_tr, xi, nrm    the formulas of fep_return_map_vm_* with p3 in the place of p[3]
 *     j0 = the largest j with kappa[j] <= k0 (0 when no comparison holds: a point on a breakpoint starts in the segment to
 *          its right, a negative k0 on the first segment extended to the left)
 *     crit = nrm - (Y + (R[j0] + slope[j0]*(k0 - kappa[j0])))
 *     not crit > 0:  s = s_tr,  ds = 2G*Dev + K*Vol,  the state untouched
 *     crit > 0:  for j = j0, j0+1, ...:  H_j = (2G + a) + slope[j],
 *                    lambda_j = (nrm - (Y + (R[j] + slope[j]*(k0 - kappa[j])))) / H_j,
 *                the first j that is the last segment or has k0 + lambda_j <= kappa[j+1] is taken (the residual
 *                nrm - H lambda - Y - R(k0 + lambda) decreases monotonically under the precondition, so this j exists and is
 *                the segment of its root);  lambda = lambda_j, H = H_j,  N = xi/nrm,  s = s_tr - 2G*lambda*N,
 *                ds = 2G*Dev + K*Vol - (2G)^2/H N(x)N - (2G)^2*lambda/nrm (Dev - N(x)N)           (rows / columns 11, 22, 12)
 *                accept:  p0 += lambda*N0,  p1 += lambda*N1,  p2 += 2*lambda*N2,  p[3] = k0 + lambda
 * ind_p = (crit > 0); counts = {number of plastic points, 0}.  ds is symmetric.  No product is fused into a sum, in any
 * kernel of the model, so tests/vmi_ref.py follows the map operation by operation.  A point whose return lands within
 * rounding of a breakpoint may take either of the two segments: s is continuous there, ds is not (H jumps with the slope).
 * With one segment of slope 0 the map is fep_return_map_vm_* on p = (p0, p1, p2, -(p0 + p1)).
 * Non-finite values: the four rules above hold with k0 counted as a fifth component of the trial state.  K*tr and nrm carry
 * the term -|0*k0|, which is -0.0 and changes no bit of a finite result, and NaN for a NaN or an infinite k0 (whose infinite
 * yield radius would otherwise give an elastic point with a finite stress): such a point, like one with a NaN strain, comes
 * back with ind_p = 0, the elastic tangent, a NaN in s and its state untouched, and is counted nowhere. */
int fep_return_map_vmi_host(int device_id, int64_t n_int,
                            const double* e_h, int64_t e_pt_stride, int64_t e_comp_stride,
                            const double* e0_h, double* ep_prev_h,
                            const double* shear_h, const double* bulk_h, const double* a_h, const double* y_h,
                            int n_seg, const double* kappa_h, const double* slope_h,
                            int accept,
                            double* s_h, double* ds_h, uint8_t* ind_p_h, int64_t* counts_h);
/* (kappa_h and slope_h are read during the call and travel as a kernel argument: a hipGraph captured from this call has the
 * curve baked into the launch, as it has e0_h) */
int fep_return_map_vmi_dev(int device_id, void* stream, int64_t n_int,
                           const double* e_d, int64_t e_pt_stride, int64_t e_comp_stride,
                           const double* e0_h, double* ep_prev_d,
                           const double* shear_d, const double* bulk_d, const double* a_d, const double* y_d,
                           int n_seg, const double* kappa_h, const double* slope_h,
                           int accept,
                           double* s_d, double* ds_d, uint8_t* ind_p_d, int64_t* counts_d);

/* ---- initial strain per point, mesh-free: one pair for every model ----------------------
 * No reference counterpart (its demo holds one s0 for the whole mesh, TSX:1675-1681).  `model` = FEP_MODEL_DP, _VM or _MC (the
 * plane-stress model and the model with a hardening curve are not offered mesh-free with a field: FEP_EINVAL; fep_step_field_*
 * of a FEP_MODEL_VMPS or FEP_MODEL_VMI context take one);
 * every other argument as in fep_return_map_* of that model (the third and fourth parameter arrays are the model's), plus
 *   e0_field   (4, n_int) C-order like ep_prev, rows 11, 22, 12 (engineering shear), 33; never modified, borrowed for the call
 *   e0_scale   one factor for the whole field
 * The initial strain of point k is
 *     z_i(k) = e0u_i + e0_scale * e0_field[i * n_int + k],     e0u_i = e0_h[i], or 0.0 when e0_h is NULL,
 * the product rounded before the sum (no fused multiply-add), and the point's return map then runs on z(k) exactly as the
 * plain entry point runs on e0: a field whose columns all equal z with e0_scale = 1 and e0_h = NULL gives the bits of the
 * plain call with e0_h = z.  The four non-finite rules above hold for the field as for e0: a NaN or an infinity at one
 * point of the field is that point's and nobody else's.  One thing is stricter than for e0: an infinite z_i(k) counts as a NaN
 * (it is replaced by one before the return map), so for every model the point comes back elastic, with the finite elastic
 * tangent and a NaN in s, and ds and K stay finite whatever the field holds.
 * FEP_EINVAL: e0_field == NULL (the plain entry points are the way to run without a field) or an unknown model. */
int fep_return_map_field_host(int model, int device_id, int64_t n_int,
                              const double* e_h, int64_t e_pt_stride, int64_t e_comp_stride,
                              const double* e0_h, const double* e0_field_h, double e0_scale, double* ep_prev_h,
                              const double* shear_h, const double* bulk_h, const double* m3_h, const double* m4_h,
                              int accept,
                              double* s_h, double* ds_h, uint8_t* ind_p_h, int64_t* counts_h);
int fep_return_map_field_dev(int model, int device_id, void* stream, int64_t n_int,
                             const double* e_d, int64_t e_pt_stride, int64_t e_comp_stride,
                             const double* e0_h, const double* e0_field_d, double e0_scale, double* ep_prev_d,
                             const double* shear_d, const double* bulk_d, const double* m3_d, const double* m4_d,
                             int accept,
                             double* s_d, double* ds_d, uint8_t* ind_p_d, int64_t* counts_d);

/* ---- a6/a7: mesh context (static operands of the hot path) ----------------------------
 * Replaces the geometry / index part of get_elastic_stiffness_matrix
 * (DP:491-601, TSX:432-542, EL:368-477): Jacobians, dphi_1/dphi_2, weight = |det|*wf,
 * and the symbolic pattern of K = B^T D B.
 *
 *   elements   (n_p, n_e) C-order, 0-based node ids (the reference's `elements`; EL passes 1-based
 *              and shifts in place, EL:389 — shift before calling)
 *   coords     (2, n_n) C-order
 *   dhatp1/2   (n_p, n_q) C-order reference-element derivative tables, wf (n_q) weight factors
 *
 * At most 256 node-pair blocks per node row of K, i.e. at most 255 neighbours of any node (the nodes it shares an
 * element with): a larger row fits no tile of the assembly and FEP_ERANGE is returned, whatever the route.  P1: a node
 * in 256 triangles; P2: 86 triangles around a vertex; P4: 26.  The library's switches FEP_ROUTE, FEP_VALIDATE_PLAN and
 * FEP_VERBOSE (fep_build_is_ablation) are read by every call and hold for the context it creates.
 */
int fep_ctx_create(fep_ctx** ctx_out, int device_id, int elem_type,
                   int64_t n_e, int64_t n_n,
                   const int32_t* elements_h, const double* coords_h,
                   const double* dhatp1_h, const double* dhatp2_h, const double* wf_h);
int fep_ctx_destroy(fep_ctx* ctx);

/* sizes[0..7] = n_e, n_n, n_p, n_q, n_int, n_dof (=2*n_n), nnz (CSR entries of K), n_blk (node-pair blocks) */
int fep_ctx_sizes(const fep_ctx* ctx, int64_t sizes[8]);
/* The kernels one step of this context launches, named as rocprofv3 prints them and joined by " + " (which = 0: a step with
 * every output, 1: the K,F-only step of a Newton iterate).  `buf` receives a NUL-terminated string of at most cap - 1
 * characters.  No reference counterpart (measurement support: bench.py's roofline label). */
int fep_ctx_kernel_names(const fep_ctx* ctx, int which, char* buf, int64_t cap);

/* dphi1, dphi2: (n_p, n_int); weight: (n_int); det: (n_int) or NULL.       DP:530-546, 585 */
int fep_ctx_geometry_host(fep_ctx* ctx, double* dphi1_h, double* dphi2_h, double* weight_h, double* det_h);

/* Symbolic CSR pattern of K (rows = DOFs, sorted columns, every structural entry of B^T D B kept,
 * also those that are numerically zero — the reference's SciPy product drops them). */
int fep_ctx_pattern_host(const fep_ctx* ctx, int32_t* indptr_h /* n_dof+1 */, int32_t* indices_h /* nnz */);

/* Per-point material parameters (n_int each): shear, bulk (DP:972-973), eta, c (DP:983-984).  When each of the four
 * arrays is constant over the mesh (the reference's demos) the kernels take the constants as arguments and do not
 * read the arrays; results are bitwise the same either way. */
int fep_ctx_set_materials_host(fep_ctx* ctx, const double* shear_h, const double* bulk_h,
                               const double* eta_h, const double* c_h);
/* The material model of the context's steps: FEP_MODEL_DP (the default), FEP_MODEL_VM, FEP_MODEL_MC, FEP_MODEL_VMPS or FEP_MODEL_VMI (below); may be called
 * before or after fep_ctx_set_materials_host.  On a von Mises context the third and fourth arrays of
 * fep_ctx_set_materials_host are a and Y (fep_return_map_vm_*), on a Mohr-Coulomb context sin_phi and c
 * (fep_return_map_mc_*; counts = {smooth face + both edges, apex}), on a plane-stress von Mises context a and Y again
 * (fep_return_map_vmps_*; the elastic plane-stress stiffness is such a context's K at U = 0).  What follows holds for all alike.  The
 * constant-parameter shortcut applies as for Drucker-Prager, and fep_step_* keep their
 * signature and every output: they run the model's point kernel (geometry from the node coordinates, strain, return map;
 * s / ds to the caller's arrays or a scratch of the context) and then what fep_assemble_dev launches for the context.
 * counts = {number of plastic points, 0}.  The call allocates that scratch itself, so fep_step_dev on a von Mises
 * context never allocates and can be captured into a hipGraph.  Drucker-Prager steps of any context are not affected.
 * FEP_EINVAL: NULL context or unknown model; FEP_ESTATE: the scratch would have to be allocated while a stream capture
 * is in progress. */
int fep_ctx_set_model(fep_ctx* ctx, int model);
int fep_ctx_model(const fep_ctx* ctx, int* model);
/* FEP_MODEL_VMI is a model of fep_ctx_set_model too (4 is none: FEP_EINVAL): the third and fourth arrays of
 * fep_ctx_set_materials_host are a and Y as for von Mises, row 3 of ep_prev is kappa (fep_return_map_vmi_*), and the steps run
 * on the hardening curve of the context, one segment of slope 0 until this call sets another (n_seg, kappa_h, slope_h as in
 * fep_return_map_vmi_*; copied, so the arrays may be freed).  Before or after the materials.  fep_step_* and fep_step_field_* of
 * such a context run as for von Mises (the model's point kernel, then the context's own assembly), allocate nothing and can be
 * captured; the curve travels as a kernel argument, so it is baked into a captured launch as e0_h is: a replay runs on the
 * curve of the capture, whatever has been set since.
 * FEP_EINVAL: NULL context or a curve that is not as stated; FEP_ESTATE: the context's model is not FEP_MODEL_VMI.  A refused
 * call changes nothing. */
int fep_ctx_set_hardening(fep_ctx* ctx, int n_seg, const double* kappa_h, const double* slope_h);

/* Device pointers of the context's static per-point arrays (for the mesh-free entry points):
 * which = 0 shear, 1 bulk, 2 eta, 3 c, 4 weight, 5 dphi1, 6 dphi2. */
int fep_ctx_device_ptr(const fep_ctx* ctx, int which, void** ptr_d);

/* ---- a1..a5 fused: one pass of the hot path ------------------------------------------
 * Replaces, for one Newton iterate (DP:1043-1058 / TSX:1771-1778):
 *     E = B*U                                   (a1)
 *     construct_constitutive_problem(E, ...)     (a2)
 *     vD = w*ds ; D_p ; K_tangent = K_elast + B^T (D_p - D_elast) B   (a3, a4)
 *     F = B^T (w * s[0:3])                       (a5)
 * K_tangent is produced as the `data` array of the context's CSR pattern, computed as
 * B^T D_p B directly (equal to the reference's expression up to fp64 rounding).
 *
 *   U          (n_dof) displacement, DOF order
 *   e0_h       4 host doubles (TSX initial strain zeta*e_init, TSX:1765) or NULL
 *   ep_prev    (4,n_int) or NULL; updated in place when accept != 0
 *   e_out      (3,n_int) C-order strain or NULL (not needed by the path itself)
 *   s, ds, ind_p   as in fep_return_map_*; any of them may be NULL when not wanted (non-finite values in U, e0, ep_prev: the
 *                  four rules stated there)
 *   k_data     out (nnz)     f_out  out (n_dof)
 *   counts     out [2] {n_smooth, n_apex} or NULL
 *
 * fep_step_dev neither allocates nor synchronises, so the call can be captured into a hipGraph.  (One exception: a P1
 * context asked for k_data / f_out on an ACCEPTING call without ds / s allocates its ds / s scratch on the first such
 * call; make that call once outside a capture.  P1 non-accepting calls without point outputs run as one kernel and need
 * no scratch; the other routes get theirs in fep_ctx_set_materials_host.)  Results are bitwise reproducible run to run
 * (fixed summation order, no floating-point atomics).
 */
int fep_step_dev(fep_ctx* ctx, void* stream, const double* u_d, const double* e0_h,
                 double* ep_prev_d, int accept,
                 double* e_out_d, double* s_d, double* ds_d, uint8_t* ind_p_d,
                 double* k_data_d, double* f_out_d, int64_t* counts_d);
int fep_step_host(fep_ctx* ctx, const double* u_h, const double* e0_h,
                  double* ep_prev_h, int accept,
                  double* e_out_h, double* s_h, double* ds_h, uint8_t* ind_p_h,
                  double* k_data_h, double* f_out_h, int64_t* counts_h);

/* The same with the displacement as the reference holds it: `u2_h` = the (2, n_n) C-ordered array `U` (DP:1043
 * flattens it column-major on every iterate); the reordering into DOF order happens inside the staging copy. */
int fep_step_host_planar(fep_ctx* ctx, const double* u2_h, const double* e0_h,
                         double* ep_prev_h, int accept,
                         double* e_out_h, double* s_h, double* ds_h, uint8_t* ind_p_h,
                         double* k_data_h, double* f_out_h, int64_t* counts_h);

/* ---- the same step with an initial strain per integration point -------------------------
 * fep_step_dev / fep_step_host with `e0_field` ((4, n_int), device resp. host, borrowed for the call) and `e0_scale` after
 * e0_h: the initial strain of point k is z(k) of fep_return_map_field_* (in-situ stress that varies over the mesh; a load
 * factor goes into e0_scale, the array stays as it is).  Such a step always runs staged, for every model and on every
 * route: the model's point kernel with the field (geometry from the node coordinates, strain, return map; s / ds to the
 * caller's arrays or the context's scratch), then what fep_assemble_dev launches for the context, then the COO form's
 * force gather.  The one-kernel P1 step and the fused element kernel do not read a field.  Outputs, counts and the four
 * non-finite rules as fep_step_*: a NaN at one point of the field is that point's NaN and nobody else's.
 * fep_step_field_dev neither allocates nor synchronises and can be captured into a hipGraph; e0_scale and e0_h are then
 * baked into the captured launch (a replay reads the field's current contents with the captured factor).  One exception:
 * a Drucker-Prager context gets its ds / s scratch and the point kernel's counters on the first such call; make that call
 * once outside a capture (FEP_ESTATE inside one).
 * FEP_EINVAL: e0_field == NULL; the plain entry points remain the way to step without a field. */
int fep_step_field_dev(fep_ctx* ctx, void* stream, const double* u_d, const double* e0_h,
                       const double* e0_field_d, double e0_scale,
                       double* ep_prev_d, int accept,
                       double* e_out_d, double* s_d, double* ds_d, uint8_t* ind_p_d,
                       double* k_data_d, double* f_out_d, int64_t* counts_d);
int fep_step_field_host(fep_ctx* ctx, const double* u_h, const double* e0_h,
                        const double* e0_field_h, double e0_scale,
                        double* ep_prev_h, int accept,
                        double* e_out_h, double* s_h, double* ds_h, uint8_t* ind_p_h,
                        double* k_data_h, double* f_out_h, int64_t* counts_h);

/* Coordinates of the context's integration points, what such a field is evaluated at: xq (2, n_int) C-order,
 *     xq[c, e*n_q + q] = sum over a ascending of hatp[a, q] * coords[c, elements[a, e]]      (no fused multiply-add)
 * with `hatp_h` the (n_p, n_q) C-order table of basis-function VALUES on the host, as in fep_load_volume_* (it travels as a
 * kernel argument).  Neither allocates nor synchronises in the _dev form.  FEP_EINVAL: a NULL argument. */
int fep_ctx_point_coords_dev(fep_ctx* ctx, void* stream, const double* hatp_h, double* xq_d);
int fep_ctx_point_coords_host(fep_ctx* ctx, const double* hatp_h, double* xq_h);

/* ---- a3..a5 only: assembly from given ds / s ------------------------------------------
 * Replaces DP:1047-1050 + DP:1058 when the caller already holds `ds` (9,n_int) and `s` (>=3 rows
 * used, (4,n_int) layout).  Either output may be NULL.  With ds = the elastic tensor this is the
 * K_elast = B^T D B of DP:595.
 * `ds` must be symmetric per point (every tangent the return map produces is): only its upper triangle,
 * rows m = 0, 1, 2, 4, 5, 8, is read, and rows 3, 6, 7 are taken to equal rows 1, 2, 5.  A non-symmetric
 * ds is assembled as its upper triangle mirrored, without an error (a check would cost as much as the
 * assembly). */
int fep_assemble_dev(fep_ctx* ctx, void* stream, const double* ds_d, const double* s_d,
                     double* k_data_d, double* f_out_d);
int fep_assemble_host(fep_ctx* ctx, const double* ds_h, const double* s_h,
                      double* k_data_h, double* f_out_h);

/* ---- multi-GPU interface exchange helpers (no reference counterpart: the reference is single-process) ----
 * Pack / unpack of the interface DOFs around the RCCL all-reduce of the internal force (sharding.py):
 *   fep_gather_f64   dst[i] = idx[i] >= 0 ? src[idx[i]] : 0      (i < n)
 *   fep_scatter_f64  dst[dst_idx[i]] = src[src_idx[i]]            (i < n; dst_idx must be unique) */
int fep_gather_f64(int device_id, void* stream, int64_t n, const double* src_d, const int32_t* idx_d, double* dst_d);
int fep_scatter_f64(int device_id, void* stream, int64_t n, const double* src_d, const int32_t* src_idx_d,
                    const int32_t* dst_idx_d, double* dst_d);
/* Neighbour-only form of the same exchange (sharding.py, exchange='p2p'): after the send / receive batch, interface DOF i
 * (local DOF loc[i]) becomes 0 + c_0 + c_1 + ... over its holders in ascending rank order; contribution k of DOF i is
 * src[ptr[i] + k] < 0 ? this rank's own f[loc[i]] : recv[src[ptr[i] + k]].  Replaces nothing in the reference (DP:1058
 * is the quantity exchanged). */
int fep_iface_sum_f64(int device_id, void* stream, int64_t n, const int32_t* loc_d, const int32_t* ptr_d,
                      const int32_t* src_d, const double* recv_d, double* f_d);

/* Gathered solve (sharding.GatherPlan, dist_newton.GatheredSolver): the sub-assembled K_r of all ranks, lying in the receive
 * buffer `recv` of the solve rank, summed onto the global CSR pattern, K = sum_r P_r^T K_r P_r.  Tables count in PAIRS of
 * doubles (one row of a 2x2 node-pair block; recv and k_global 16-byte aligned): for q < 2 n_blocks, pair q of k_global is
 * pair first[q] of recv where first[q] >= 0, else 0.0 + the pairs multi_src[multi_ptr[k] .. multi_ptr[k+1]) of recv in the
 * listed (ascending rank) order, k = -1 - first[q].  One pass, every value written exactly once: no zero fill, no atomics,
 * the same bits for any launch geometry.  Entries of the tables are not checked against the length of recv.  n_blocks
 * beyond the 32-bit pattern: FEP_ERANGE.  Replaces nothing in the reference. */
int fep_csr_merge_f64(int device_id, void* stream, int64_t n_blocks, const int32_t* first_d, const int32_t* multi_ptr_d,
                      const int32_t* multi_src_d, const double* recv_d, double* k_global_d);

/* ---- callers of the hot path ----------------------------------------------------------------
 * transform (DP:760-816): integration-point values (n_int) -> nodal values (n_n), mean over the points of the
 * adjacent elements weighted with quadrature weight * |det J| (the footing pressure that steers the load step,
 * DP:1105).  A node that belongs to no element gets 0/0 = NaN, as the reference's F1 / F2 (DP:812) gives. */
int fep_transform_dev(fep_ctx* ctx, void* stream, const double* q_int_d, double* q_node_d);
int fep_transform_host(fep_ctx* ctx, const double* q_int_h, double* q_node_h);

/* ---- external loads (EL:246-364; the same two functions at TSX:546-988) ---------------------------------
 * Volume (body-force) vector, get_vector_volume EL:246-292:
 *     f_V[c, n] = sum over the (element e, local node a) with elements[a, e] == n, over the points q of e, of
 *                 hatp[a, q] * weight[e * n_q + q] * f_v[c, e * n_q + q]
 *
 *   hatp_h     (n_p, n_q) C-order basis-function VALUES at the quadrature points (get_local_basis_volume's first
 *              result, EL:136-209); host memory, read during the call and passed on as a kernel argument
 *   f_v        (2, n_int) planar, or NULL: the uniform body force (fx, fy) at every point (self-weight), without a field
 *              in memory; fx, fy are ignored when f_v is given
 *   weight     (n_int) or NULL = the context's own |det J| * wf (EL:441); a caller's modified weights are honoured as the
 *              reference honours its `weight` argument
 *   f_out      (n_dof) interleaved (x, y) per node, DOF order like F of fep_step_dev; every node is written, a node that
 *              belongs to no element gets 0 (the reference's sparse sum has no entry there)
 *
 * One lane per node over the node -> (element, local node) lists; no floating-point atomics, terms added in the fixed
 * order (e, a) ascending then q, products formed as hatp * (weight * f) without contraction: two calls give the same
 * bits, and so do the uniform form and a field holding the same two numbers.  fep_load_volume_dev neither allocates nor
 * copies nor synchronises: it can be captured into a hipGraph (the table is baked into the captured launch). */
int fep_load_volume_dev(fep_ctx* ctx, void* stream, const double* hatp_h, const double* f_v_d, double fx, double fy,
                        const double* weight_d, double* f_out_d);
int fep_load_volume_host(fep_ctx* ctx, const double* hatp_h, const double* f_v_h, double fx, double fy,
                         const double* weight_h, double* f_out_h);

/* Traction (surface-load) vector over boundary edges, get_vector_traction EL:295-364, context-free (edges are not
 * elements of a context):
 *     f_t[c, n] = sum over the (edge e, local node a) with edges[a, e] == n, over the surface points q, of
 *                 hatp_s[a, q] * |J(e, q)| * wf_s[q] * t_int[c, e * n_q_s + q]
 *     |J| = sqrt(j1^2 + j2^2),  j_c = sum_a coords[c, edges[a, e]] * dhatp1_s[a, q]
 * Two departures from EL:344-353, both supersets of it: the Jacobian is the full arc length (the reference takes |j1|,
 * right on horizontal edges only), and t_int holds a value PER surface point (the reference applies the last point's
 * value everywhere; the Python wrapper get_vector_traction broadcasts it to keep that quirk).
 *
 *   edges_h    (n_p_s, n_e_s) C-order, 0-based node ids, HOST memory in both forms (FEP_ERANGE for an id outside [0, n_n));
 *              n_p_s = 2 (P1, Q1), 3 (P2, Q2: end, end, middle), up to 5; n_q_s up to 8
 *   xy         (2, n_n) planar node coordinates       hatp_s_h, dhatp1_s_h (n_p_s, n_q_s), wf_s_h (n_q_s): host
 *   t_int      (2, n_e_s * n_q_s) planar              f_out (2 n_n) interleaved, zero off the loaded edges
 *
 * The node -> (edge, local node) lists of the loaded nodes are built on the host and uploaded by every call, so BOTH forms
 * allocate scratch and synchronise `stream` before they return (not capturable; n_e_s is of the order of sqrt(n_e)).  No
 * floating-point atomics, fixed order (e, a) ascending then q. */
int fep_load_traction_dev(int device_id, void* stream, int64_t n_n, int64_t n_e_s, int n_p_s, int n_q_s,
                          const int32_t* edges_h, const double* xy_d, const double* hatp_s_h, const double* dhatp1_s_h,
                          const double* wf_s_h, const double* t_int_d, double* f_out_d);
int fep_load_traction_host(int device_id, int64_t n_n, int64_t n_e_s, int n_p_s, int n_q_s,
                           const int32_t* edges_h, const double* xy_h, const double* hatp_s_h, const double* dhatp1_s_h,
                           const double* wf_s_h, const double* t_int_h, double* f_out_h);

/* ---- mesh: P1 -> P2 / P4 enrichment and uniform refinement of triangle meshes ------------
 * Replaces create_midpoints_P2 (TSX:1508-1626) and create_midpoints_P4 (TSX:1354-1505) — a sequential loop over
 * elements in which the first element to see an edge creates its nodes — by the order-free form of the same numbering,
 * and adds uniform (red) refinement, which the reference does not have.  Context-free: the mesh exists before any context.
 *
 * Edge k of a triangle runs from vertex k to vertex (k + 1) % 3.  A half-edge (element i, edge k) OWNS its edge iff no
 * other element holds both ends or the one that does has the higher id.  With c_i = number of owned edges of i and
 * base = the exclusive prefix sum of c:
 *   P2  slots in visit order (V2V3, V3V1, V1V2: TSX:1530, 1561, 1591); the r-th owned slot of i has index base_i + r;
 *       its node is n_n + index at (cA + cB) / 2.  elem_ext rows (V1, V2, V3, m23, m31, m12).
 *   P4  slots (V1V2, V2V3, V3V1: TSX:1386, 1424, 1463); interior nodes 3 i + 3 base_i + {0, 1, 2} (nearest V1, V2, V3,
 *       TSX:1374-1381); the r-th owned slot has its midpoint at m = 3 i + 3 base_i + 3 + 3 r, the quarter point nearer
 *       its start A at m + 1 (3 cA / 4 + cB / 4), nearer its end B at m + 2; the neighbour, which walks the edge
 *       backwards, takes them swapped (TSX:1405-1416).  elem_ext rows: 3 vertices, 3 midpoints, 6 quarter points (two per
 *       slot), 3 interior nodes.
 *   surf  the owned boundary half-edges in (element, visit slot) order: rows (B, A, node) for P2 and
 *       (B, A, mid, mid + 1, mid + 2) for P4.   elem_ed (3, n_e): index of the edge in each P2 slot;
 *       edge_el (2, n_edges): owner element, neighbour element (0 on a boundary edge: the reference leaves its zero there).
 *   refinement  new vertices = the P2 midside nodes (old nodes keep their ids); children 4 i .. 4 i + 3 of element i =
 *       (V1, m12, m31), (m12, V2, m23), (m31, m23, V3), (m12, m23, m31); orientation is preserved and boundary edges are
 *       halved as straight segments unless curves are set (fep_mesh_set_curves below).
 * Coordinates are computed without contraction into fused multiply-adds, so every array equals the host functions' bit for
 * bit.  No floating-point atomics; two calls give the same bytes.
 *
 *   fep_mesh_create     elem (3, n_e) int32 C-order, coord (2, n_n), both host pointers (on_device == 0) or both device
 *                       pointers of device_id; copies them, builds node -> element lists, matches the half-edges (one
 *                       lane per element, a loop of the start vertex's degree per edge), owners and both prefix sums on
 *                       `stream`, then synchronises it.  Nodes of no element are legal.  FEP_EINVAL: n_e < 1, NULL
 *                       pointers; FEP_ERANGE: a vertex id outside [0, n_n), n_n or 4 n_e beyond int32 (no mesh is made).
 *   fep_mesh_info       info = {n_e, n_n, n_edges, n_boundary_edges, n_nonmanifold (edges of more than two elements),
 *                       n_inconsistent (interior edges whose two elements walk them the same way), n_degenerate
 *                       (triangles naming a vertex twice)}.  Output sizes follow from it: P2 adds n_edges nodes,
 *                       P4 3 n_e + 3 n_edges.
 *   fep_mesh_enrich_*   elem_type FEP_P2 / FEP_P4 (FEP_EINVAL otherwise).  elem_ext (6 | 15, n_e), coord_ext (2, n_n + new),
 *                       surf (3 | 5, n_boundary_edges) (may be NULL when there is no boundary edge); P2 only, each may be
 *                       NULL: elem_ed (3, n_e), edge_el (2, n_edges); ignored for P4.  ids are int32.
 *   fep_mesh_refine_*   elem_child (3, 4 n_e), coord_ext (2, n_n + n_edges)
 *                       Both: FEP_ESTATE, and nothing written, when n_nonmanifold, n_inconsistent or n_degenerate > 0 (on
 *                       such meshes the reference's result depends on its visit order and has no parallel form);
 *                       FEP_ERANGE when n_n + new nodes exceeds int32.  _dev forms enqueue on `stream` and leave
 *                       everything on the device, so levels chain without a host round trip; _host forms are synchronous. */
typedef struct fep_mesh fep_mesh;
int fep_mesh_create(fep_mesh** mesh_out, int device_id, void* stream, int64_t n_e, int64_t n_n, const int32_t* elem,
                    const double* coord, int on_device);
int fep_mesh_destroy(fep_mesh* mesh);
int fep_mesh_info(const fep_mesh* mesh, int64_t info[7]);
int fep_mesh_enrich_dev(const fep_mesh* mesh, void* stream, int elem_type, int32_t* elem_ext_d, double* coord_ext_d,
                        int32_t* surf_d, int32_t* elem_ed_d, int32_t* edge_el_d);
int fep_mesh_enrich_host(const fep_mesh* mesh, int elem_type, int32_t* elem_ext_h, double* coord_ext_h, int32_t* surf_h,
                         int32_t* elem_ed_h, int32_t* edge_el_h);
int fep_mesh_refine_dev(const fep_mesh* mesh, void* stream, int32_t* elem_child_d, double* coord_ext_d);
int fep_mesh_refine_host(const fep_mesh* mesh, int32_t* elem_child_h, double* coord_ext_h);

/* Curved boundaries (opt-in; without curves every output above is byte for byte what it was).  A curve is an axis-aligned
 * ellipse, five doubles (cx, cy, a, b, tol); a circle has a == b.  For a point p: dx = x - cx, dy = y - cy, u = dx / a,
 * v = dy / b, g = sqrt(u u + v v), evaluated in this order without fused multiply-adds.  A vertex is ON the curve iff
 * |g - 1| <= tol.  An edge is CURVED iff it is a boundary edge (exactly one element holds it) and both its ends are on
 * the same curve; the lowest curve index wins; an interior edge is never curved.  Every node the library creates on a
 * curved edge (the refinement / P2 midpoint, the P4 midpoint and its two quarter points) is computed as a straight point
 * exactly as above and then moved to (cx + dx / g, cy + dy / g), with dx, dy, g of that straight point; for g == 0 (a
 * chord through the centre) it stays.  Existing vertices never move; ids, elem_ext, elem_ed, edge_el, surf and the child
 * table do not depend on the curves.  The three interior nodes of a P4 element follow its curved edges, so that the
 * element's map stays smooth enough for a quartic.  With d_m, d_a, d_b the offsets (moved minus straight) of the midpoint of
 * a curved edge a -> b and of its quarter points nearer a and nearer b, and with every interior node starting at its
 * straight position, for each curved edge of the element in the order V1V2, V2V3, V3V1 and per component:
 *     node nearest a:         p = p + ((w_m d_m + w_n d_a) + w_f d_b)         w_m = 5 / 18, w_n = 10 / 27, w_f = -2 / 27,
 *     node nearest b:         p = p + ((w_m d_m + w_f d_a) + w_n d_b)         w_o = 1 / 4 (each the double nearest to it),
 *     node nearest the third: p = p + w_o d_m
 * which is (l_a + l_b)^2 sum_k L_k(t) d_k at the node's barycentric coordinates l, t = l_b / (l_a + l_b), L_k the quartic
 * Lagrange basis on {0, 1/4, 1/2, 3/4, 1}.  A boundary edge is owned by its element, so no other element's nodes are
 * needed.  The host functions apply the same rules with the same operations in the same order.
 *
 *   fep_mesh_set_curves   curves_h: n_curves x 5 HOST doubles, copied; they travel to the enrichment / refinement kernels as
 *                         a by-value argument (no allocation: the _dev forms stay capturable).  n_curves = 0 clears them.
 *                         FEP_EINVAL, and the mesh keeps the curves it had: n_curves < 0 or > FEP_MAX_CURVES, a <= 0,
 *                         b <= 0, tol < 0, any value not finite.
 *   fep_mesh_surf_curve_* curve_of_surf (n_boundary_edges): for every boundary edge in the `surf` order of elem_type
 *                         (FEP_P2 / FEP_P4) the index of its curve, -1 for a straight one: what a caller needs to put a
 *                         traction on one curved boundary with fep_load_traction_*.  FEP_ESTATE as fep_mesh_enrich_*.
 *   fep_mesh_area_stats_* Context-free: P1 vertex rows elem (3, n_e) int32, coord (2, n_n); both device pointers of
 *                         device_id (_dev, enqueued on `stream`, out: 4 device doubles) or all host pointers (_host,
 *                         synchronous).  With the doubled signed area d = (x2 - x1)(y3 - y1) - (x3 - x1)(y2 - y1):
 *                         out = {min d, sum of d / 2, number of triangles with d <= 0, n_e}; min d = +inf for n_e = 0.  A
 *                         triangle with a vertex id outside [0, n_n) counts as d = 0.  Per-workgroup partials and a
 *                         one-workgroup final pass in a fixed order: two calls give the same bytes; no floating-point
 *                         atomics.  The partials live in one fixed block per (device, stream) made by the first call on
 *                         that stream (FEP_ESTATE if that first call comes while the stream is being captured).  The check
 *                         that a projected level folded no element, without leaving the device. */
#define FEP_MAX_CURVES 4
int fep_mesh_set_curves(fep_mesh* mesh, int n_curves, const double* curves_h);
int fep_mesh_surf_curve_dev(const fep_mesh* mesh, void* stream, int elem_type, int32_t* curve_of_surf_d);
int fep_mesh_surf_curve_host(const fep_mesh* mesh, int elem_type, int32_t* curve_of_surf_h);
int fep_mesh_area_stats_dev(int device_id, void* stream, int64_t n_e, int64_t n_n, const int32_t* elem_d, const double* coord_d,
                            double* out_d);
int fep_mesh_area_stats_host(int device_id, int64_t n_e, int64_t n_n, const int32_t* elem_h, const double* coord_h,
                             double* out_h);

/* Refinement of MARKED elements: one level of conforming longest-edge bisection (Rivara's 4T-LE), which the reference does
 * not have.  Opt-in: without these calls every output above is byte for byte what it was.
 *   reference edge  r of an element = its longest edge: squared length dx dx + dy dy with dx = x[B] - x[A], dy = y[B] - y[A]
 *       of the vertex chord (also on a curved edge) in the element's own walking direction, without fused multiply-adds;
 *       slots compared in the order 0, 1, 2 with a strict >, so the lowest slot wins a tie.  Both elements of an edge get
 *       the same squared length (the signs cancel exactly).
 *   closure  a marked element marks its three edges; an edge is marked if either half-edge says so; an element with any
 *       marked edge must have its reference edge marked.  The least fixpoint of a monotone rule: unique, finite and
 *       independent of the order of evaluation, so kernels and a sequential loop reach the same marks.
 *   nodes  every marked edge gets one node, n_n + the rank of the edge among the marked edges in the P2 edge order (elem_ed),
 *       at the coordinates fep_mesh_refine_* gives that edge's midside node (computed by the owner; moved onto the curves of
 *       fep_mesh_set_curves by the same rule).  With every element marked coord_ext equals fep_mesh_refine_*'s bit for bit.
 *   children  with a = V[r], b = V[(r + 1) % 3], c = V[(r + 2) % 3] and m, p, q the nodes of ab, bc, ca: an element without
 *       a marked edge is one child, its row unchanged; any other is (a, m, q), (q, m, c) — or (a, m, c) when ca is not
 *       marked — followed by (m, b, p), (m, p, c) — or (m, b, c) when bc is not.  1 + (marked edges) children per element,
 *       from the exclusive prefix sum of these counts on; parent[child] = element.  Orientation is preserved.
 *
 *   fep_mesh_mark   marked (n_e) bytes, non-zero = marked: a host pointer (on_device == 0) or a device pointer of the mesh's
 *                   device (FEP_EINVAL, and the mesh keeps the marks it had, when the pointer is NULL, on the other side
 *                   than on_device says, or memory of another device).  Closes the marks, ranks the edges and counts the children on `stream`, stores
 *                   the result in the mesh in place of any earlier one, and SYNCHRONISES `stream`, because the output sizes
 *                   depend on it: not capturable.  Its first call on a mesh allocates the scratch the mesh keeps.
 *                   out = {n_child, n_new_nodes, elements with a marked edge, n_sweeps}; n_sweeps (closure sweeps enqueued)
 *                   is informational: each sweep lets a workgroup iterate over its own marks in LDS until they stand still
 *                   and reads other workgroups' marks from memory; several sweeps are enqueued per read of the "changed"
 *                   word.  The stored marks do not depend on any of this.  No marks at all is legal: the identity
 *                   (n_child = n_e, no new node, parent = 0 .. n_e - 1).
 *   fep_mesh_refine_marked_*  elem_child (3, n_child), coord_ext (2, n_n + n_new_nodes), parent (n_child; may be NULL).
 *                   The _dev form enqueues on `stream` and allocates nothing; the _host form is synchronous.
 *                   FEP_ESTATE, and nothing written: n_nonmanifold, n_inconsistent or n_degenerate > 0 (both calls), or no
 *                   successful fep_mesh_mark before.  FEP_EINVAL: NULL pointers.  FEP_ERANGE (fep_mesh_mark): n_n +
 *                   n_new_nodes beyond int32 (n_child <= 4 n_e cannot be: fep_mesh_create refuses such a mesh).  No floating-point atomics; two calls give the same bytes. */
int fep_mesh_mark(fep_mesh* mesh, void* stream, const uint8_t* marked, int on_device, int64_t out[4]);
int fep_mesh_refine_marked_dev(const fep_mesh* mesh, void* stream, int32_t* elem_child_d, double* coord_ext_d, int32_t* parent_d);
int fep_mesh_refine_marked_host(const fep_mesh* mesh, int32_t* elem_child_h, double* coord_ext_h, int32_t* parent_h);

/* ---- state transfer across refinement: displacement and per-point state from parents to children --------------------
 * No reference counterpart.  Opt-in: without these calls every output above is byte for byte what it was.  Triangles only
 * (FEP_P1, FEP_P2, FEP_P4), the same element type on both meshes.
 *
 *   corner codes  parent[child] does not say WHICH part of the parent a child is; corners (3, n_child) uint8 does:
 *       corners[k, ch] describes vertex row k of child ch: 0, 1, 2 = the parent's vertex row 0, 1, 2; 3, 4, 5 = the node on the
 *       parent's edge 0, 1, 2 (edge k runs from vertex k to vertex (k + 1) % 3).  Marked refinement, in the names of
 *       fep_mesh_mark's "children" with a = r, b = (r + 1) % 3, c = (r + 2) % 3, m = 3 + r, p = 3 + (r + 1) % 3,
 *       q = 3 + (r + 2) % 3: the rows (a, m, q), (q, m, c) | (a, m, c) and (m, b, p), (m, p, c) | (m, b, c) hold exactly those
 *       codes; an element without a marked edge gets (0, 1, 2).  Uniform refinement (fep_mesh_refine_*): children 4 i .. 4 i + 3
 *       are (0, 3, 5), (3, 1, 4), (5, 4, 2), (3, 4, 5) with parent = child / 4: a constant table, no kernel.  The codes do not
 *       depend on curves: the reference edge is decided on vertex chords.
 *   fep_mesh_child_corners_*  corners (3, n_child) of the marks the mesh holds.  FEP_ESTATE on the conditions of
 *       fep_mesh_refine_marked_*; FEP_EINVAL: NULL pointers.  The _dev form enqueues one kernel (one lane per element, writing
 *       from the first child of the element on) and allocates nothing; the _host form is synchronous.
 *
 *   barycentrics of a code, in the order (V1, V2, V3):  B[0] = (1, 0, 0), B[1] = (0, 1, 0), B[2] = (0, 0, 1),
 *       B[3] = (1/2, 1/2, 0), B[4] = (0, 1/2, 1/2), B[5] = (1/2, 0, 1/2).  A point with barycentrics l in the child has
 *       L = l0 B[c0] + l1 B[c1] + l2 B[c2] in the parent, reference coordinates (x1, x2) = (L[1], L[2]).
 *   shape   a triple of codes.  FEP_TRANSFER_SHAPES = 21 occur (the identity, 18 of marked refinement, 4 uniform, 2 of them
 *       shared), numbered in ascending order of c0 + 6 c1 + 36 c2.  What depends on the shape alone is data, computed on the host
 *       in float64 (tables.py, transfer_tables) and handed over; the library knows no basis function:
 *         shape_of_code (216) int8   indexed c0 + 6 c1 + 36 c2; -1 for a triple that is no shape
 *         w    (FEP_TRANSFER_SHAPES, n_p, n_p)   w[s, j, a] = basis function a of the parent at the parent coordinates of the
 *                                                child's node j
 *         near (FEP_TRANSFER_SHAPES, n_q) uint8  the parent's integration point nearest (in reference coordinates, the lowest
 *                                                index on a tie) to the child's point k
 *   nodes   u (n_n_parent, n_comp) row-major, n_comp in 1..4 (the interleaved U of the drivers is n_comp = 2), u_child
 *       (n_n_child, n_comp).  For child ch with e = parent[ch], s = shape_of_code[corners[:, ch]], local node j, component i:
 *       acc = 0.0, then for a = 0 .. n_p - 1:  acc = acc + w[s, j, a] * u[elem_parent[a, e], i]  — one IEEE double product and
 *       one addition per term, terms with a zero weight like any other, nothing contracted.  A child node is written once, by
 *       the lowest pair index ch n_p + j among the (child element, local node) pairs that hold it: an integer minimum, the
 *       only atomic.  A node of no child element gets NaN (fep_transform_*).  So an old vertex keeps its value: == the input
 *       and bit-equal to it, except that -0.0 becomes +0.0.
 *   points  q (n_rows, n_e n_q) planar (a plastic strain is 4 rows, a material 1), q_child (n_rows, n_child n_q):
 *       q_child[:, ch n_q + k] = q[:, e n_q + near[s, k]], a bitwise copy: a copied value is one the model has produced or
 *       accepted, an extrapolated one can leave the yield surface or turn a modulus negative.
 *   bad input never reads out of bounds: a child whose parent is outside [0, n_e), whose triple has a code above 5 or is no
 *       shape, or whose parent element names a node outside [0, n_n_parent), gets NaN in all its point values and in the nodes
 *       it owns; a child node id outside [0, n_n_child) is skipped.  Nothing else changes.
 *   non-finite values (the four rules of fep_return_map_*): a NaN at a parent node reaches exactly the nodes owned by children of
 *       the elements that hold it (0 * NaN is NaN: also where its weight is 0), a NaN at a parent point exactly the child
 *       points that copy it; a clean call afterwards gives the clean bytes.
 *
 * The _dev forms only enqueue: no read-back, no synchronisation.  The owners (8 bytes per child node) live in one grow-only
 * block per (device, stream), by the rule of counts_d (fep_return_map_dev): FEP_ESTATE if it would have to grow while the stream
 * is being captured (run the call once outside the capture first).  The _host forms are synchronous, on the library's stream
 * with device blocks of the call, as the mesh forms.  FEP_EINVAL: NULL pointers (of arrays that are not empty), elem_type not
 * P1 / P2 / P4, n_comp outside 1..4, n_rows < 1, negative counts, an output that shares bytes with an input; FEP_ERANGE: a count
 * of 2^31 - 1 or more.  n_child = 0 is legal (every child node is then a node of no element).  A refused call writes nothing. */
#define FEP_TRANSFER_SHAPES 21
int fep_mesh_child_corners_dev(const fep_mesh* mesh, void* stream, uint8_t* corners_d);
int fep_mesh_child_corners_host(const fep_mesh* mesh, uint8_t* corners_h);
int fep_transfer_nodes_dev(int device_id, void* stream, int elem_type, int n_comp, int64_t n_e, int64_t n_n_parent, int64_t n_child,
                           int64_t n_n_child, const int32_t* elem_parent_d, const int32_t* elem_child_d, const int32_t* parent_d,
                           const uint8_t* corners_d, const int8_t* shape_of_code_d, const double* w_d, const double* u_d,
                           double* u_child_d);
int fep_transfer_nodes_host(int device_id, int elem_type, int n_comp, int64_t n_e, int64_t n_n_parent, int64_t n_child,
                            int64_t n_n_child, const int32_t* elem_parent_h, const int32_t* elem_child_h, const int32_t* parent_h,
                            const uint8_t* corners_h, const int8_t* shape_of_code_h, const double* w_h, const double* u_h,
                            double* u_child_h);
int fep_transfer_points_dev(int device_id, void* stream, int elem_type, int n_rows, int64_t n_e, int64_t n_child,
                            const int32_t* parent_d, const uint8_t* corners_d, const int8_t* shape_of_code_d, const uint8_t* near_d,
                            const double* q_d, double* q_child_d);
int fep_transfer_points_host(int device_id, int elem_type, int n_rows, int64_t n_e, int64_t n_child, const int32_t* parent_h,
                             const uint8_t* corners_h, const int8_t* shape_of_code_h, const uint8_t* near_h, const double* q_h,
                             double* q_child_h);

/* ---- recovered-stress error indicator and bulk marking: what decides the marks of fep_mesh_mark ----------------------
 * No reference counterpart.  Opt-in: without these calls every output above is byte for byte what it was.  Zienkiewicz-Zhu:
 * the step's stress s ((4, n_int), rows 11, 22, 12, 33) is averaged to the nodes, and the indicator of an element is the
 * complementary-energy norm of (recovered - computed) over it.  Every operation below is one IEEE double operation in the
 * order written (parentheses bind, otherwise left to right), nothing is contracted into a fused multiply-add, and there are no
 * floating-point atomics: two calls give the same bytes, and so does the NumPy twin estimate.py.
 *
 *   recovery    s_node (4, n_n) planar.  For node n, with a0..a3 = ws = 0.0: for each entry of the node's incidence list in
 *               ascending (element, local node) order, for q = 0 .. n_q - 1, k = e n_q + q, w = weight[k] (the context's
 *               |det J| * wf, as in fep_transform_*):  a_i = a_i + w * s[i, k] (i = 0..3),  ws = ws + w.
 *               s_node[i, n] = a_i / ws.  A node of no element gets 0/0 = NaN, as fep_transform_* gives (a NaN is a NaN: its
 *               sign bit is the machine's, the one thing in which the twin's bytes may differ).
 *   norm        for a 4-vector d and moduli G, K:  tr = (d0 + d1) + d3,  m = tr / 3,  e_i = d_i - m (i = 0, 1, 3),
 *               c(d) = (((e0 e0 + e1 e1) + e3 e3) + 2 (d2 d2)) / (2 G) + (tr tr) / (9 K)        (= d : C^-1 : d)
 *               It serves plane strain and plane stress (s33 = 0) alike: the indicator does not depend on the context's
 *               model.  G, K are the context's shear and bulk at the point (or its constants: the same bits).
 *   P1          one point per element, s constant, weight[e] the area; V_a the vertices, i = 0..3:
 *               d_a[i] = s_node[i, V_a] - s[i, e],   b[i] = ((d_0[i] + d_1[i]) + d_2[i]) / 3,
 *               eta2[e] = weight[e] * (c(b) + ((c(d_0 - b) + c(d_1 - b)) + c(d_2 - b)) / 12)
 *               — the exact integral of the linear difference, not the one-point rule.
 *   P2 Q1 Q2 P4 r_q[i] = 0.0, then for a = 0 .. n_p - 1:  r_q[i] = r_q[i] + hatp[a, q] * s_node[i, elements[a, e]];
 *               acc = 0.0, then for q = 0 .. n_q - 1, k = e n_q + q:  acc = acc + weight[k] * c(r_q - s[:, k]);  eta2[e] = acc.
 *               hatp_h: the (n_p, n_q) basis-function VALUES on the host, as in fep_load_volume_* (a kernel argument).
 *   T(v)        the fixed-order sum of n values: pad v with +0.0 to a multiple of 256; in every block of 256 consecutive values,
 *               for s = 128, 64, ..., 1:  x[i] = x[i] + x[i + s] for i < s; the block's sum is x[0]; T(v) = T(block sums), until
 *               one value is left (T of nothing is +0.0).  One launch per level.
 *   stats       v_e = eta2[e] where that is finite, else +0.0.  stats = {T(v), the largest positive v_e (+0.0 if there is
 *               none), the number of non-finite eta2[e], n_e}.
 *   marking     for eta2 (n) and theta in (0, 1]:  total = T(v),  goal = theta * total,
 *               tail(t) = T(v_e where eta2[e] is finite and >= t, else +0.0).  If total > 0, t* is the largest double
 *               t <= max (of stats) with tail(t) >= goal, else t* = +inf.  marked[e] = 1 iff eta2[e] is finite, > 0 and >= t*, else 0.
 *               Rounding is monotone and the tree is the same for every t, so tail never increases with t: t* exists, is one
 *               of the values and does not depend on how it is looked for, and all values tied at t* are marked, so the set
 *               depends on no ordering.  The library walks the 63 value bits of t from the top, one pass over eta2 per bit
 *               (a bit stays set if the candidate is <= max and its tail >= goal), every decision taken on the device.
 *               out = {t*, tail(t*), number marked, total}.
 * Non-finite values (the four rules of fep_return_map_*): a NaN or an infinity in s at one point makes eta2 non-finite for
 * exactly the elements that share a node with that point's element; it stays in eta2 and is counted in stats[2], enters no
 * sum and is never marked; every other eta2, and the marks among the finite values, are bit for bit those of the clean call
 * wherever the poisoned elements contribute nothing to them; a clean call afterwards returns the same bytes as before.
 *
 *   fep_recover_stress_*  s (4, n_int) -> s_node (4, n_n).  One lane per node.  The _dev form enqueues one kernel.
 *   fep_estimate_*        s, s_node (of fep_recover_stress_*; an input in both forms) -> eta2 (n_e); stats (4 doubles) may be
 *                         NULL; hatp_h is ignored for P1.  One lane per element.  FEP_ESTATE: materials not set.
 *   fep_mark_bulk_*       context-free.  marked (n bytes) is what fep_mesh_mark(..., on_device = 1) takes.  n = 0 is legal:
 *                         out = {+inf, 0, 0, 0}.  63 + 2 passes of 1 + (levels above the leaves) launches.
 * The _dev forms only enqueue: no read-back, no synchronisation.  The partials of the tree levels and the descent's state
 * live in one grow-only block per (device, stream), by the rule of counts_d (fep_return_map_dev): FEP_ESTATE if it would have
 * to grow while the stream is being captured (fep_estimate_dev with stats, fep_mark_bulk_dev; run the call once outside the
 * capture first).  FEP_EINVAL: NULL pointers (hatp_h for any type but P1), n < 0, theta outside (0, 1] or NaN; FEP_ERANGE:
 * n of 2^39 or more.  A refused call writes nothing.  The _host forms are synchronous; the two context forms follow the stream
 * contract of fep_transform_host. */
int fep_recover_stress_dev(fep_ctx* ctx, void* stream, const double* s_d, double* s_node_d);
int fep_recover_stress_host(fep_ctx* ctx, const double* s_h, double* s_node_h);
int fep_estimate_dev(fep_ctx* ctx, void* stream, const double* hatp_h, const double* s_d, const double* s_node_d,
                     double* eta2_d, double* stats_d);
int fep_estimate_host(fep_ctx* ctx, const double* hatp_h, const double* s_h, const double* s_node_h, double* eta2_h,
                      double* stats_h);
int fep_mark_bulk_dev(int device_id, void* stream, int64_t n, const double* eta2_d, double theta, uint8_t* marked_d,
                      double* out_d);
int fep_mark_bulk_host(int device_id, int64_t n, const double* eta2_h, double theta, uint8_t* marked_h, double* out_h);

/* Linear solve of a Newton iterate, K[Q][:,Q] dU[Q] = b[Q]  (np.linalg.solve on the dense boolean-masked block at
 * DP:1062-1066 / TSX:1781).  Preconditioned conjugate gradients (2x2 node-block Jacobi) entirely on
 * the device; K is the `data` array fep_step_dev wrote, on the context's CSR pattern.  The Jacobi blocks are the 2x2
 * diagonal blocks of K with constrained DOFs replaced by identity rows and columns and the off-diagonal symmetrised to
 * (K[2n,2n+1] + K[2n+1,2n]) / 2; a block that is not positive definite is replaced by the identity.
 *
 *   fep_solver_create   pattern = fep_ctx_pattern_host (checked: rows 2n, 2n+1 share their columns, which come in
 *                       pairs 2m, 2m+1 -> FEP_EINVAL otherwise); free_dof_h (2 n_n) is Q in DOF order, non-zero = free
 *   fep_solver_sizes    {n_n, n_dof, nnz, n_free}
 *   fep_solver_spmv_dev y = K x (masked != 0: y = Q K x, x must then be 0 on the constrained DOFs); x != y
 *   fep_solver_pcg_dev  x = 0 on entry is implied; iterates until |r| <= rtol |b[Q]| (recursive residual), at most
 *                       max_iter iterations; the host looks at the device-side state after at most check_every
 *                       iterations (<= 0: 50; sooner when the residual history says the test is about to be met) and the
 *                       iterate is frozen on the device at the iteration that met the test.
 *                       *state_out: 0 = max_iter reached, 1 = converged, 2 = breakdown (K[Q][:,Q] not positive
 *                       definite or non-finite values); x is 0 on constrained DOFs.  Synchronises `stream`.
 *                       A NaN in a K entry of a free row or in b at a free DOF is a breakdown at the FIRST read-back: the call
 *                       returns FEP_OK with state 2 and *iters_out <= check_every, and x is the zero vector the call starts
 *                       from, never a NaN.  b at constrained DOFs and K entries whose row and column are both constrained are
 *                       selected away, not multiplied by zero: a NaN there changes no bit of x, iters or relres. */
typedef struct fep_solver fep_solver;
int fep_solver_create(fep_solver** solver_out, int device_id, int64_t n_n, const int32_t* indptr_h,
                      const int32_t* indices_h, const uint8_t* free_dof_h);
int fep_solver_destroy(fep_solver* solver);
int fep_solver_sizes(const fep_solver* solver, int64_t sizes[4]);
int fep_solver_spmv_dev(fep_solver* solver, void* stream, const double* k_data_d, const double* x_d, double* y_d,
                        int masked);
int fep_solver_pcg_dev(fep_solver* solver, void* stream, const double* k_data_d, const double* b_d, double* x_d,
                       double rtol, int max_iter, int check_every, int* iters_out, double* relres_out,
                       int* state_out);

/* Multigrid preconditioner for the same solve (smoothed aggregation).  The hierarchy is built on the host (solver.py:
 * aggregates from fep_aggregate_host, rigid-body-mode prolongators, Galerkin products with SciPy) from a reference
 * matrix on the context's pattern — normally K_elast — and pushed level by level; the solver applies it as a V(2,2)
 * cycle in which level 0 is always the CURRENT tangent (k_data_d of the call) and the coarse operators are those of the
 * reference matrix unless the refresh re-projects them (fep_solver_amg_enable_refresh).  Smoother: degree-2 Chebyshev in
 * D^-1 A on [lmax/20, lmax], lmax = 1.2 x the value the smoothed level's omega encodes (omega = 4 / (3 * 1.05 * rho)),
 * D = the Jacobi blocks above on level 0 and the 3x3 block inverses below it.
 * The preconditioner reads single precision — K in the smoother's level-0 passes, the refreshed coarse operators
 * and the transfers, applied in node blocks —;
 * CG's own product, its vectors and the Galerkin products are double precision.
 *
 *   fep_solver_amg_push_level   transfer level k -> k+1 (k = number of levels pushed so far; level 0 = the mesh DOFs):
 *       P (n_fine x n_coarse) and R = P^T (n_coarse x n_fine) in CSR; A = operator of level k+1 (n_coarse^2, CSR) or,
 *       when last != 0, its INVERSE (dense rows in CSR); D = inverse of the block diagonal of A (CSR; NULL when last);
 *       omega_fine = damping of the smoother on level k.  Rows of P belonging to constrained DOFs must be zero.
 *   fep_solver_amg_clear        drops the hierarchy
 *   fep_solver_amg_pcg_dev      as fep_solver_pcg_dev, preconditioned with the V-cycle (FEP_ESTATE without a complete
 *                               hierarchy); check_every <= 0: 10
 *   fep_solver_amg_enable_refresh   after the last level: from now on every fep_solver_amg_pcg_dev first re-projects the
 *                               coarse operators from ITS k_data_d — A_1 = R_0 K P_0, A_2 = R_1 A_1 P_1, ... with the
 *                               transfers as pushed, block-Jacobi inverses and the coarsest inverse recomputed — instead of
 *                               keeping those of the reference matrix (numeric products on patterns fixed here by the host;
 *                               the terms of every output entry are listed on the device:
 *                               40 % fewer iterations on plastic tangents).  FEP_ERANGE: coarsest level > 256 DOFs (its inverse
 *                               is recomputed by one workgroup; checked first, the hierarchy is left as pushed) or a product
 *                               whose pattern / term list exceeds 32-bit counts (found while the plans are built: the
 *                               hierarchy is DROPPED, as after an allocation failure).  A caller that wants to go on with the
 *                               reference operators pushes the levels again after FEP_ERANGE (solver.py: setup_amg does).
 *   fep_solver_amg_refresh_dev  the re-projection alone, stream-ordered (FEP_ESTATE unless enabled)
 *   fep_aggregate_host          greedy aggregation of a node graph in CSR (a neighbour list may repeat ids, in any order):
 *                               agg_out[i] in [0, *n_agg_out) */
int fep_solver_amg_clear(fep_solver* solver);
int fep_solver_amg_enable_refresh(fep_solver* solver);
int fep_solver_amg_refresh_dev(fep_solver* solver, void* stream, const double* k_data_d);
int fep_solver_amg_push_level(fep_solver* solver, int64_t n_fine, int64_t n_coarse,
                              const int32_t* p_indptr, const int32_t* p_indices, const double* p_vals,
                              const int32_t* r_indptr, const int32_t* r_indices, const double* r_vals,
                              const int32_t* a_indptr, const int32_t* a_indices, const double* a_vals,
                              const int32_t* d_indptr, const int32_t* d_indices, const double* d_vals,
                              double omega_fine, int last);
int fep_solver_amg_pcg_dev(fep_solver* solver, void* stream, const double* k_data_d, const double* b_d, double* x_d,
                           double rtol, int max_iter, int check_every, int* iters_out, double* relres_out,
                           int* state_out);
int fep_aggregate_host(int64_t n, const int32_t* indptr, const int32_t* indices, int32_t* agg_out, int64_t* n_agg_out);
/* Host sparse product C = X * Y for the set-up's Galerkin products (P^T A P with SciPy in the first versions; the reference has
 * no multigrid: DP:1062-1066 is a dense solve), rows in parallel.  _count: structural row sizes into c_indptr_out (n_rows + 1);
 * _fill: column ids ascending per row and values on that structure (entries that cancel to zero are kept).  No GPU involved. */
int fep_spgemm_count_host(int64_t n_rows, int64_t n_mid, int64_t n_cols, const int32_t* x_indptr, const int32_t* x_indices,
                          const int32_t* y_indptr, const int32_t* y_indices, int32_t* c_indptr_out);
int fep_spgemm_fill_host(int64_t n_rows, int64_t n_mid, int64_t n_cols, const int32_t* x_indptr, const int32_t* x_indices,
                         const double* x_vals, const int32_t* y_indptr, const int32_t* y_indices, const double* y_vals,
                         const int32_t* c_indptr, int32_t* c_indices_out, double* c_vals_out);

/* ---- in-situ kernel timing (bench.py's roofline figure) --------------------------------
 * Between fep_ctx_profile_begin and fep_ctx_profile_end every fep_step_dev / fep_assemble_dev call
 * brackets each of its kernels with HIP events on the launch stream (the kernels run in their real
 * position inside the step, not replayed back to back).  _end synchronises the stream and returns
 * the average milliseconds per launch.  P1 (node route): ms_out[0] p1_point_kernel (strain + return map),
 * ms_out[1] p1_node_lds_kernel (tangent CSR values + force), ms_out[2] 0; a P1 step that runs as ONE kernel (no point
 * output wanted, not accepting): ms_out[0] = the gap between two event marks (~0.005), ms_out[1] p1_fused_kernel
 * (+ the one-workgroup counter sum).  Other element types / COO route:
 * ms_out[0] element_kernel (strain + return map + K_e, f_e), ms_out[1] csr_reduce_kernel, ms_out[2]
 * force_reduce_kernel.  *n_steps = steps averaged. */
int fep_ctx_profile_begin(fep_ctx* ctx);
int fep_ctx_profile_end(fep_ctx* ctx, void* stream, double ms_out[3], int* n_steps);

#ifdef __cplusplus
}
#endif
#endif /* FEP_H */
