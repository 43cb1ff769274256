// Triangle-mesh operations that run before any context exists (include/fep.h, "mesh"): edge matching, the P1 -> P2 / P4
// enrichment with the reference's node numbering (TSX:1354-1626) and uniform refinement.
//
// The sequential numbering of the reference (first element to see an edge creates its nodes) has an order-free form on
// edge-manifold, consistently oriented meshes: a half-edge owns its edge iff it has no neighbour or its element id is the
// lower one, and the k-th owned slot of element i (in the reference's visit order) gets index base_i + k, base = the
// exclusive prefix sum of the owned counts.  Everything below computes that form; nothing depends on the order in which
// lanes run (integer atomics only where the outcome is order-free: counts, cursors into lists whose order is not observed).
//
// Edge k of an element runs from vertex k to vertex (k + 1) % 3.  P2 visits the edges in the order 1, 2, 0 (slots V2V3, V3V1,
// V1V2: TSX:1530, 1561, 1591), P4 in the order 0, 1, 2 (TSX:1386, 1424, 1463).
//
// Also here, because it is context-free and produces what fep_mesh_mark reads: the fixed-order sums, the statistics and the
// bulk marking of the error indicator (include/fep.h, "recovered-stress error indicator"; ind_level_kernel, fep_mark_bulk_*).
#include "fep_common.h"
#include "fep_staging.h"

#include <cmath>
#include <new>

#pragma clang fp contract(off)

namespace {

constexpr int kBlock = 256;
constexpr int kScanItems = 4;
constexpr int kScanTile = kBlock * kScanItems;

inline unsigned grid_for(int64_t n, int per_block) { return (unsigned)((n + per_block - 1) / per_block); }

// counters of fep_mesh_create
enum { C_RANGE = 0, C_DEGENERATE, C_NONMANIFOLD, C_INCONSISTENT, C_COUNT };

__device__ __forceinline__ bool load_tri(const int32_t* __restrict__ elem, int64_t n_e, int64_t n_n, int64_t i, int32_t v[3]) {
    v[0] = elem[i];
    v[1] = elem[n_e + i];
    v[2] = elem[2 * n_e + i];
    const bool in_range = v[0] >= 0 && v[0] < n_n && v[1] >= 0 && v[1] < n_n && v[2] >= 0 && v[2] < n_n;
    return in_range && v[0] != v[1] && v[1] != v[2] && v[2] != v[0];
}

// elements per node; elements with an id outside [0, n_n) or a repeated vertex are counted and take no further part
__global__ void __launch_bounds__(kBlock) mesh_degree_kernel(int64_t n_e, int64_t n_n, const int32_t* __restrict__ elem,
                                                             int32_t* __restrict__ deg, int32_t* __restrict__ counters) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_e) return;
    int32_t v[3];
    if (!load_tri(elem, n_e, n_n, i, v)) {
        const bool in_range = v[0] >= 0 && v[0] < n_n && v[1] >= 0 && v[1] < n_n && v[2] >= 0 && v[2] < n_n;
        atomicAdd(&counters[in_range ? C_DEGENERATE : C_RANGE], 1);
        return;
    }
    for (int k = 0; k < 3; ++k) atomicAdd(&deg[v[k]], 1);
}

// list of node v = [ptr[v], ptr[v + 1]) holds 3 * element + position of v in it, in no particular order
__global__ void __launch_bounds__(kBlock) mesh_fill_kernel(int64_t n_e, int64_t n_n, const int32_t* __restrict__ elem,
                                                           const int32_t* __restrict__ ptr, int32_t* __restrict__ cursor,
                                                           int32_t* __restrict__ list) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_e) return;
    int32_t v[3];
    if (!load_tri(elem, n_e, n_n, i, v)) return;
    for (int k = 0; k < 3; ++k) {
        const int32_t at = atomicAdd(&cursor[v[k]], 1);
        const int32_t lo = ptr[v[k]], hi = ptr[v[k] + 1];
        if (at < hi - lo) list[lo + at] = (int32_t)(3 * i + k);
    }
}

// One lane per element, its three edges in turn: the other elements that hold both ends, found in the list of the start
// vertex (a loop of the node's degree).  mask: bit k = edge k is owned, bit 3 + k = edge k is a boundary edge.
// nbr[k * n_e + i] = 3 * j + (edge of j that is the same edge), -1 on the boundary.
__global__ void __launch_bounds__(kBlock) mesh_match_kernel(int64_t n_e, int64_t n_n, const int32_t* __restrict__ elem,
                                                            const int32_t* __restrict__ ptr, const int32_t* __restrict__ list,
                                                            int32_t* __restrict__ nbr, uint8_t* __restrict__ mask,
                                                            int32_t* __restrict__ n_own, int32_t* __restrict__ n_bnd,
                                                            int32_t* __restrict__ counters) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_e) return;
    int32_t v[3];
    const bool ok = load_tri(elem, n_e, n_n, i, v);
    int m = 0, c_own = 0, c_bnd = 0;
    for (int k = 0; k < 3; ++k) {
        int32_t found = -1;
        if (ok) {
            const int32_t A = v[k], B = v[(k + 1) % 3];
            int n_match = 0, n_same_way = 0;
            int64_t j_min = n_e;
            const int32_t lo = ptr[A], hi = ptr[A + 1];
            for (int32_t q = lo; q < hi; ++q) {
                const int32_t code = list[q];
                const int64_t j = code / 3;
                const int p = code % 3;
                if (j == i) continue;
                const int32_t before = elem[(int64_t)((p + 2) % 3) * n_e + j];      // j walks before -> A -> after
                const int32_t after = elem[(int64_t)((p + 1) % 3) * n_e + j];
                if (before == B) {
                    found = (int32_t)(3 * j + (p + 2) % 3);
                } else if (after == B) {
                    found = (int32_t)(3 * j + p);
                    ++n_same_way;
                } else {
                    continue;
                }
                ++n_match;
                j_min = j < j_min ? j : j_min;
            }
            if (n_match == 0) {
                m |= (1 << k) | (8 << k);
                ++c_own;
                ++c_bnd;
            } else if (n_match == 1) {
                if (i < j_min) {
                    m |= 1 << k;
                    ++c_own;
                    if (n_same_way) atomicAdd(&counters[C_INCONSISTENT], 1);
                }
            } else if (i < j_min) {
                atomicAdd(&counters[C_NONMANIFOLD], 1);                               // once per edge: by its lowest element
            }
        }
        nbr[(int64_t)k * n_e + i] = found;
    }
    mask[i] = (uint8_t)m;
    n_own[i] = c_own;
    n_bnd[i] = c_bnd;
}

// ---- exclusive prefix sum of int32, any length: block scan, scan of the block sums (recursively), add ---------------------
__global__ void __launch_bounds__(kBlock) scan_tile_kernel(int64_t n, int32_t* __restrict__ data, int32_t* __restrict__ sums) {
    __shared__ int32_t lds[kBlock];
    const int64_t first = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kScanItems;
    int32_t x[kScanItems];
    int32_t acc = 0;
    for (int r = 0; r < kScanItems; ++r) {
        x[r] = first + r < n ? data[first + r] : 0;
        acc += x[r];
    }
    lds[threadIdx.x] = acc;
    __syncthreads();
    for (int d = 1; d < kBlock; d *= 2) {
        const int32_t other = threadIdx.x >= (unsigned)d ? lds[threadIdx.x - d] : 0;
        __syncthreads();
        lds[threadIdx.x] += other;
        __syncthreads();
    }
    int32_t run = lds[threadIdx.x] - acc;
    for (int r = 0; r < kScanItems; ++r) {
        if (first + r < n) data[first + r] = run;
        run += x[r];
    }
    if (threadIdx.x == kBlock - 1) sums[blockIdx.x] = lds[kBlock - 1];
}

__global__ void __launch_bounds__(kBlock) scan_add_kernel(int64_t n, int32_t* __restrict__ data, const int32_t* __restrict__ sums) {
    const int64_t first = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kScanItems;
    const int32_t add = sums[blockIdx.x];
    for (int r = 0; r < kScanItems; ++r)
        if (first + r < n) data[first + r] += add;
}

// in place; `scratch` holds the block sums of every level (scan_scratch_len(n) entries)
int64_t scan_scratch_len(int64_t n) {
    int64_t total = 0;
    while (true) {
        n = (n + kScanTile - 1) / kScanTile;
        total += n;
        if (n <= 1) return total;
    }
}

int scan_exclusive(hipStream_t st, int64_t n, int32_t* data, int32_t* scratch) {
    const int64_t n_tiles = (n + kScanTile - 1) / kScanTile;
    hipLaunchKernelGGL(scan_tile_kernel, dim3((unsigned)n_tiles), dim3(kBlock), 0, st, n, data, scratch);
    HIP_TRY(hipGetLastError());
    if (n_tiles > 1) {
        FEP_TRY(scan_exclusive(st, n_tiles, scratch, scratch + n_tiles));
        hipLaunchKernelGGL(scan_add_kernel, dim3((unsigned)n_tiles), dim3(kBlock), 0, st, n, data, scratch);
        HIP_TRY(hipGetLastError());
    }
    return FEP_OK;
}

// ---- numbering ------------------------------------------------------------------------------------------------------------
// index of edge k of element e among the new nodes, the edge being OWNED by e (bit k of m set)
__device__ __forceinline__ int32_t p2_index(int32_t base_e, int m, int k) {
    const int rank = k == 1 ? 0 : (k == 2 ? ((m >> 1) & 1) : (((m >> 1) & 1) + ((m >> 2) & 1)));   // visit order 1, 2, 0
    return base_e + rank;
}
__device__ __forceinline__ int32_t p4_index(int64_t e, int32_t base_e, int m, int k) {
    return (int32_t)(3 * e + 3 * (int64_t)base_e + 3 + 3 * __popc(m & ((1 << k) - 1)));         // visit order 0, 1, 2
}
__device__ __forceinline__ int bnd_rank_p2(int m, int k) {
    return k == 1 ? 0 : (k == 2 ? ((m >> 4) & 1) : (((m >> 4) & 1) + ((m >> 5) & 1)));
}

struct MeshView {
    int64_t n_e, n_n, n_edges, n_bnd;
    const int32_t* elem;
    const double* coord;
    const int32_t* nbr;
    const uint8_t* mask;
    const int32_t* base;     // exclusive prefix sum of the owned counts
    const int32_t* bbase;    // ... of the boundary counts
};

// ---- curved boundaries (fep.h, fep_mesh_set_curves) -----------------------------------------------------------------------
// Axis-aligned ellipses (cx, cy, a, b, tol), passed to the kernels by value.  g(p) = sqrt(u u + v v), u = (x - cx) / a,
// v = (y - cy) / b; p is ON the curve iff |g - 1| <= tol.  The host functions (midpoints.py) do the same operations in the
// same order; contraction is off for this file, division and square root of doubles are correctly rounded.
struct CurveSet {
    int n;
    double v[FEP_MAX_CURVES][5];
};

__device__ __forceinline__ double curve_g(const double* __restrict__ c, double x, double y, double* dx, double* dy) {
    *dx = x - c[0];
    *dy = y - c[1];
    const double u = *dx / c[2], v = *dy / c[3];
    return sqrt(u * u + v * v);
}

__device__ __forceinline__ bool on_curve(const double* __restrict__ c, double x, double y) {
    double dx, dy;
    return fabs(curve_g(c, x, y, &dx, &dy) - 1) <= c[4];
}

// the curve a boundary edge with the ends a, b follows: the lowest one that holds both, -1 if none does
__device__ __forceinline__ int edge_curve(const CurveSet& S, double ax, double ay, double bx, double by) {
    for (int q = 0; q < S.n; ++q)
        if (on_curve(S.v[q], ax, ay) && on_curve(S.v[q], bx, by)) return q;
    return -1;
}

// the straight point moved along its ray from the centre onto the curve; a point AT the centre (g == 0) stays
__device__ __forceinline__ void project(const double* __restrict__ c, double* x, double* y) {
    double dx, dy;
    const double g = curve_g(c, *x, *y, &dx, &dy);
    if (g == 0) return;
    *x = c[0] + dx / g;
    *y = c[1] + dy / g;
}

// P2 index of edge k of element i, whoever owns it
__device__ __forceinline__ int32_t p2_edge(const MeshView& M, int64_t i, int k, int m, bool* owned, int64_t* j_out) {
    *owned = (m >> k) & 1;
    if (*owned) {
        const int32_t nb = M.nbr[(int64_t)k * M.n_e + i];
        *j_out = nb < 0 ? -1 : nb / 3;
        return p2_index(M.base[i], m, k);
    }
    const int32_t nb = M.nbr[(int64_t)k * M.n_e + i];
    const int64_t j = nb / 3;
    *j_out = j;
    return p2_index(M.base[j], M.mask[j], nb % 3);
}

// grid.y = slot s (edge k = (s + 1) % 3), one lane per element: coalesced rows of elem_ext / elem_ed
__global__ void __launch_bounds__(kBlock) enrich_p2_kernel(MeshView M, CurveSet S, int32_t* __restrict__ elem_ext, double* __restrict__ coord_ext,
                                                           int32_t* __restrict__ surf, int32_t* __restrict__ elem_ed,
                                                           int32_t* __restrict__ edge_el) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= M.n_e) return;
    const int s = blockIdx.y, k = (s + 1) % 3;
    const int m = M.mask[i];
    const int32_t A = M.elem[(int64_t)k * M.n_e + i], B = M.elem[(int64_t)((k + 1) % 3) * M.n_e + i];
    bool owned;
    int64_t j;
    const int32_t ind = p2_edge(M, i, k, m, &owned, &j);
    const int64_t n_tot = M.n_n + M.n_edges;
    elem_ext[(int64_t)s * M.n_e + i] = M.elem[(int64_t)s * M.n_e + i];
    elem_ext[(int64_t)(3 + s) * M.n_e + i] = (int32_t)(M.n_n + ind);
    if (elem_ed) elem_ed[(int64_t)s * M.n_e + i] = ind;
    if (!owned) return;
    const double ax = M.coord[A], ay = M.coord[M.n_n + A], bx = M.coord[B], by = M.coord[M.n_n + B];
    double mx = (ax + bx) / 2, my = (ay + by) / 2;
    if (j < 0 && S.n > 0) {
        const int q = edge_curve(S, ax, ay, bx, by);
        if (q >= 0) project(S.v[q], &mx, &my);
    }
    coord_ext[M.n_n + ind] = mx;
    coord_ext[n_tot + M.n_n + ind] = my;
    if (edge_el) {
        edge_el[ind] = (int32_t)i;
        edge_el[M.n_edges + ind] = j < 0 ? 0 : (int32_t)j;       // the reference leaves its zero on a boundary edge
    }
    if (j < 0) {
        const int64_t at = M.bbase[i] + bnd_rank_p2(m, k);
        surf[at] = B;
        surf[M.n_bnd + at] = A;
        surf[2 * M.n_bnd + at] = (int32_t)(M.n_n + ind);
    }
}

// the three new nodes of a P4 edge a -> b at their straight positions: midpoint, quarter point nearer a, nearer b
__device__ __forceinline__ void p4_edge_points(double ax, double ay, double bx, double by, double* px, double* py) {
    px[0] = (ax + bx) / 2; px[1] = 3 * ax / 4 + bx / 4; px[2] = ax / 4 + 3 * bx / 4;
    py[0] = (ay + by) / 2; py[1] = 3 * ay / 4 + by / 4; py[2] = ay / 4 + 3 * by / 4;
}

// Blending weights of a P4 element's interior nodes for one curved edge a -> b (fep.h, fep_mesh_set_curves):
// (l_a + l_b)^2 L_k(t) at t = l_b / (l_a + l_b) for the edge's midpoint and quarter points.
constexpr double kBlendMid = 5.0 / 18.0, kBlendNear = 10.0 / 27.0, kBlendFar = -2.0 / 27.0, kBlendOpp = 1.0 / 4.0;

// What the curved edge a -> b of an element adds to one of its interior nodes: `role` 0 = the node nearest a, 1 = the node
// nearest the third vertex, 2 = the node nearest b.  Nothing for an edge on no curve.
__device__ __forceinline__ void p4_blend(const CurveSet& S, int role, double ax, double ay, double bx, double by, double* ix, double* iy) {
    const int q = edge_curve(S, ax, ay, bx, by);
    if (q < 0) return;
    double sx[3], sy[3], dx[3], dy[3];
    p4_edge_points(ax, ay, bx, by, sx, sy);
    for (int r = 0; r < 3; ++r) {
        double px = sx[r], py = sy[r];
        project(S.v[q], &px, &py);
        dx[r] = px - sx[r];
        dy[r] = py - sy[r];
    }
    if (role == 0) {
        *ix = *ix + ((kBlendMid * dx[0] + kBlendNear * dx[1]) + kBlendFar * dx[2]);
        *iy = *iy + ((kBlendMid * dy[0] + kBlendNear * dy[1]) + kBlendFar * dy[2]);
    } else if (role == 2) {
        *ix = *ix + ((kBlendMid * dx[0] + kBlendFar * dx[1]) + kBlendNear * dx[2]);
        *iy = *iy + ((kBlendMid * dy[0] + kBlendFar * dy[1]) + kBlendNear * dy[2]);
    } else {
        *ix = *ix + kBlendOpp * dx[0];
        *iy = *iy + kBlendOpp * dy[0];
    }
}

// grid.y = edge k = slot; lane k of an element also writes its interior node k (nearest vertex k, TSX:1374-1381), moved by
// the blending rule for every curved edge of the element: boundary edges are owned by their element, so the lane has all it needs
__global__ void __launch_bounds__(kBlock) enrich_p4_kernel(MeshView M, CurveSet S, int32_t* __restrict__ elem_ext, double* __restrict__ coord_ext,
                                                           int32_t* __restrict__ surf) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= M.n_e) return;
    const int k = blockIdx.y;
    const int m = M.mask[i];
    const int64_t n_e = M.n_e, n_n = M.n_n;
    const int64_t n_tot = n_n + 3 * n_e + 3 * M.n_edges;
    const int32_t A = M.elem[(int64_t)k * n_e + i], B = M.elem[(int64_t)((k + 1) % 3) * n_e + i];
    const int32_t C = M.elem[(int64_t)((k + 2) % 3) * n_e + i];
    const int32_t base_i = M.base[i];
    const bool owned = (m >> k) & 1;
    const int32_t nb = M.nbr[(int64_t)k * n_e + i];
    int32_t mid;
    if (owned) {
        mid = p4_index(i, base_i, m, k);
    } else {
        const int64_t j = nb / 3;
        mid = p4_index(j, M.base[j], M.mask[j], nb % 3);
    }
    elem_ext[(int64_t)k * n_e + i] = A;
    elem_ext[(int64_t)(3 + k) * n_e + i] = (int32_t)(n_n + mid);
    elem_ext[(int64_t)(6 + 2 * k) * n_e + i] = (int32_t)(n_n + mid + (owned ? 1 : 2));     // the neighbour walks the edge backwards
    elem_ext[(int64_t)(7 + 2 * k) * n_e + i] = (int32_t)(n_n + mid + (owned ? 2 : 1));
    const int64_t inner = 3 * i + 3 * (int64_t)base_i + k;
    elem_ext[(int64_t)(12 + k) * n_e + i] = (int32_t)(n_n + inner);
    const double ax = M.coord[A], ay = M.coord[n_n + A], bx = M.coord[B], by = M.coord[n_n + B];
    const double cx = M.coord[C], cy = M.coord[n_n + C];
    // c1 / 2 + c2 / 4 + c3 / 4 and its permutations, summed in the order V1, V2, V3
    double ix, iy;
    if (k == 0) { ix = ax / 2 + bx / 4 + cx / 4; iy = ay / 2 + by / 4 + cy / 4; }            // A = V1, B = V2, C = V3
    else if (k == 1) { ix = cx / 4 + ax / 2 + bx / 4; iy = cy / 4 + ay / 2 + by / 4; }       // C = V1, A = V2, B = V3
    else { ix = bx / 4 + cx / 4 + ax / 2; iy = by / 4 + cy / 4 + ay / 2; }                   // B = V1, C = V2, A = V3
    if ((m >> 3) && S.n > 0) {
        // the element's edges in the order V1V2, V2V3, V3V1; edge e is this lane's (A, B), (B, C) or (C, A)
        for (int e = 0; e < 3; ++e) {
            if (!((m >> (3 + e)) & 1)) continue;
            const int rel = (e - k + 3) % 3;
            if (rel == 0) p4_blend(S, 0, ax, ay, bx, by, &ix, &iy);
            else if (rel == 1) p4_blend(S, 1, bx, by, cx, cy, &ix, &iy);
            else p4_blend(S, 2, cx, cy, ax, ay, &ix, &iy);
        }
    }
    coord_ext[n_n + inner] = ix;
    coord_ext[n_tot + n_n + inner] = iy;
    if (!owned) return;
    double px[3], py[3];
    p4_edge_points(ax, ay, bx, by, px, py);
    if (nb < 0 && S.n > 0) {
        const int q = edge_curve(S, ax, ay, bx, by);
        if (q >= 0)
            for (int r = 0; r < 3; ++r) project(S.v[q], &px[r], &py[r]);
    }
    for (int r = 0; r < 3; ++r) {
        coord_ext[n_n + mid + r] = px[r];
        coord_ext[n_tot + n_n + mid + r] = py[r];
    }
    if (nb < 0) {
        const int64_t at = M.bbase[i] + __popc((m >> 3) & ((1 << k) - 1));
        const int64_t n_b = M.n_bnd;
        surf[at] = B;
        surf[n_b + at] = A;
        surf[2 * n_b + at] = (int32_t)(n_n + mid);
        surf[3 * n_b + at] = (int32_t)(n_n + mid + 1);
        surf[4 * n_b + at] = (int32_t)(n_n + mid + 2);
    }
}

// one lane per element: its three P2 midside ids, the coordinates of those it owns, its four children
__global__ void __launch_bounds__(kBlock) refine_kernel(MeshView M, CurveSet S, int32_t* __restrict__ child, double* __restrict__ coord_ext) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= M.n_e) return;
    const int m = M.mask[i];
    const int64_t n_tot = M.n_n + M.n_edges;
    int32_t v[3], mid[3];
    for (int k = 0; k < 3; ++k) v[k] = M.elem[(int64_t)k * M.n_e + i];
    for (int k = 0; k < 3; ++k) {
        bool owned;
        int64_t j;
        const int32_t ind = p2_edge(M, i, k, m, &owned, &j);
        mid[k] = (int32_t)(M.n_n + ind);
        if (owned) {
            const int32_t A = v[k], B = v[(k + 1) % 3];
            const double ax = M.coord[A], ay = M.coord[M.n_n + A], bx = M.coord[B], by = M.coord[M.n_n + B];
            double mx = (ax + bx) / 2, my = (ay + by) / 2;
            if (j < 0 && S.n > 0) {
                const int q = edge_curve(S, ax, ay, bx, by);
                if (q >= 0) project(S.v[q], &mx, &my);
            }
            coord_ext[M.n_n + ind] = mx;
            coord_ext[n_tot + M.n_n + ind] = my;
        }
    }
    const int32_t m12 = mid[0], m23 = mid[1], m31 = mid[2];
    const int64_t n_c = 4 * M.n_e;
    int32_t* r0 = child + 4 * i;
    int32_t* r1 = child + n_c + 4 * i;
    int32_t* r2 = child + 2 * n_c + 4 * i;
    r0[0] = v[0]; r0[1] = m12;  r0[2] = m31;  r0[3] = m12;          // children (V1, m12, m31), (m12, V2, m23),
    r1[0] = m12;  r1[1] = v[1]; r1[2] = m23;  r1[3] = m23;          //          (m31, m23, V3), (m12, m23, m31)
    r2[0] = m31;  r2[1] = m23;  r2[2] = v[2]; r2[3] = m31;
}

// ---- refinement of marked elements: conforming longest-edge bisection (fep.h, fep_mesh_mark) -------------------------------
// bits[i]: bit k = half-edge k of element i says its edge is marked.  An edge IS marked iff either half-edge says so.
// ref[i]: the reference edge, the longest one (squared chord in the element's walking direction, slots compared 0, 1, 2
// with a strict >).  The closure — an element with any marked edge marks its reference edge — is the least fixpoint of a
// monotone rule on the bits, so it does not depend on the order in which lanes, workgroups or sweeps evaluate it.
__device__ __forceinline__ int edge_state(const int32_t* __restrict__ nbr, const uint8_t* bits, int64_t n_e, int64_t i, int k, int own) {
    const int32_t nb = nbr[(int64_t)k * n_e + i];
    return ((own >> k) & 1) | (nb < 0 ? 0 : ((bits[nb / 3] >> (nb % 3)) & 1));
}

__global__ void __launch_bounds__(kBlock) mark_init_kernel(MeshView M, const uint8_t* __restrict__ marked, uint8_t* __restrict__ bits,
                                                           uint8_t* __restrict__ ref) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= M.n_e) return;
    double x[3], y[3], len[3];
    for (int k = 0; k < 3; ++k) {
        const int32_t v = M.elem[(int64_t)k * M.n_e + i];
        x[k] = M.coord[v];
        y[k] = M.coord[M.n_n + v];
    }
    for (int k = 0; k < 3; ++k) {
        const double dx = x[(k + 1) % 3] - x[k], dy = y[(k + 1) % 3] - y[k];
        len[k] = dx * dx + dy * dy;
    }
    int r = 0;
    if (len[1] > len[r]) r = 1;
    if (len[2] > len[r]) r = 2;
    ref[i] = (uint8_t)r;
    bits[i] = marked[i] ? 7 : 0;
}

// One sweep.  A workgroup iterates over its own kBlock bytes in LDS until none of them changes — a chain of reference edges
// inside the workgroup closes in one launch — with the bits of neighbours in other workgroups read once, before the loop.
// Those may be older than what their workgroup writes in this launch; bits are only ever added, so an old value delays a
// mark and never loses one, and the workgroup that added it raises `changed`, which brings another launch.  A launch that
// leaves `changed` at zero has evaluated the rule of every element on the final bytes: the fixpoint.  A lane writes its
// own byte only.
__global__ void __launch_bounds__(kBlock) mark_sweep_kernel(int64_t n_e, const int32_t* __restrict__ nbr, const uint8_t* __restrict__ ref,
                                                            uint8_t* bits, int32_t* __restrict__ changed) {
    __shared__ int l_bits[kBlock];
    const int64_t first = (int64_t)blockIdx.x * kBlock, i = first + threadIdx.x;
    const bool active = i < n_e;
    int b = 0, r = 0, outside = 0, at[3] = {-1, -1, -1}, shift[3] = {0, 0, 0};
    if (active) {
        b = bits[i];
        r = ref[i];
        for (int k = 0; k < 3; ++k) {
            const int32_t nb = nbr[(int64_t)k * n_e + i];
            if (nb < 0) continue;
            const int64_t j = nb / 3;
            if (j >= first && j < first + kBlock) {
                at[k] = (int)(j - first);
                shift[k] = nb % 3;
            } else {
                outside |= (bits[j] >> (nb % 3)) & 1;
            }
        }
    }
    const int b_in = b;
    while (true) {
        l_bits[threadIdx.x] = b;
        __syncthreads();
        int any = b | outside;
        for (int k = 0; k < 3; ++k)
            if (at[k] >= 0) any |= (l_bits[at[k]] >> shift[k]) & 1;
        const int b_new = any ? (b | (1 << r)) : b;
        const int moved = active && b_new != b;
        if (active) b = b_new;
        if (!__syncthreads_or(moved)) break;               // also the barrier between these reads and the next writes
    }
    if (b != b_in) bits[i] = (uint8_t)b;
    if (__syncthreads_or(b != b_in) && threadIdx.x == 0) atomicOr(changed, 1);
}

// flag of every edge at its index (written by the owner), number of children per element, number of elements with a marked edge
__global__ void __launch_bounds__(kBlock) mark_count_kernel(MeshView M, const uint8_t* __restrict__ bits, int32_t* __restrict__ eflag,
                                                            int32_t* __restrict__ n_child, int32_t* __restrict__ n_touched) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    int n = 0;
    if (i < M.n_e) {
        const int m = M.mask[i], own = bits[i];
        for (int k = 0; k < 3; ++k) {
            const int st = edge_state(M.nbr, bits, M.n_e, i, k, own);
            n += st;
            if ((m >> k) & 1) eflag[p2_index(M.base[i], m, k)] = st;
        }
        n_child[i] = 1 + n;
    }
    const int c = __syncthreads_count(n > 0);
    if (threadIdx.x == 0 && c > 0) atomicAdd(n_touched, c);
}

// one lane per element: the nodes of its marked edges (coordinates by the owner, with refine_kernel's operations), its
// 1 + (number of marked edges) children from cbase[i] on, their parent ids
__global__ void __launch_bounds__(kBlock) refine_marked_kernel(MeshView M, CurveSet S, const uint8_t* __restrict__ bits,
                                                               const uint8_t* __restrict__ ref, const int32_t* __restrict__ erank,
                                                               const int32_t* __restrict__ cbase, int64_t n_tot, int64_t n_c,
                                                               int32_t* __restrict__ child, double* __restrict__ coord_ext,
                                                               int32_t* __restrict__ parent) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= M.n_e) return;
    const int m = M.mask[i], own = bits[i];
    int32_t v[3], node[3];
    for (int k = 0; k < 3; ++k) v[k] = M.elem[(int64_t)k * M.n_e + i];
    for (int k = 0; k < 3; ++k) {
        node[k] = -1;
        if (!edge_state(M.nbr, bits, M.n_e, i, k, own)) continue;
        bool owned;
        int64_t j;
        const int32_t ind = p2_edge(M, i, k, m, &owned, &j);
        node[k] = (int32_t)(M.n_n + erank[ind]);
        if (owned) {
            const int32_t A = v[k], B = v[(k + 1) % 3];
            const double ax = M.coord[A], ay = M.coord[M.n_n + A], bx = M.coord[B], by = M.coord[M.n_n + B];
            double mx = (ax + bx) / 2, my = (ay + by) / 2;
            if (j < 0 && S.n > 0) {
                const int q = edge_curve(S, ax, ay, bx, by);
                if (q >= 0) project(S.v[q], &mx, &my);
            }
            coord_ext[node[k]] = mx;
            coord_ext[n_tot + node[k]] = my;
        }
    }
    int64_t at = cbase[i];
    auto put = [&](int32_t a, int32_t b, int32_t c) {
        child[at] = a;
        child[n_c + at] = b;
        child[2 * n_c + at] = c;
        if (parent) parent[at] = (int32_t)i;
        ++at;
    };
    const int r = ref[i];
    const int32_t mm = node[r];
    if (mm < 0) {                                            // no marked edge (the closure marks r whenever one is)
        put(v[0], v[1], v[2]);
        return;
    }
    const int32_t a = v[r], b = v[(r + 1) % 3], c = v[(r + 2) % 3], p = node[(r + 1) % 3], q = node[(r + 2) % 3];
    if (q >= 0) { put(a, mm, q); put(q, mm, c); } else put(a, mm, c);
    if (p >= 0) { put(mm, b, p); put(mm, p, c); } else put(mm, b, c);
}

// refine_marked_kernel's child logic with the ids replaced by corner codes (fep.h, fep_mesh_child_corners_*): code k = the
// parent's vertex row k, code 3 + k = the node on its edge k.  One lane per element, from cbase[i] on.
__global__ void __launch_bounds__(kBlock) child_corners_kernel(MeshView M, const uint8_t* __restrict__ bits, const uint8_t* __restrict__ ref,
                                                               const int32_t* __restrict__ cbase, int64_t n_c, uint8_t* __restrict__ corners) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= M.n_e) return;
    const int own = bits[i];
    int st[3];
    for (int k = 0; k < 3; ++k) st[k] = edge_state(M.nbr, bits, M.n_e, i, k, own);
    int64_t at = cbase[i];
    auto put = [&](int a, int b, int c) {
        corners[at] = (uint8_t)a;
        corners[n_c + at] = (uint8_t)b;
        corners[2 * n_c + at] = (uint8_t)c;
        ++at;
    };
    const int r = ref[i];
    if (!st[r]) {                                            // no marked edge (the closure marks r whenever one is)
        put(0, 1, 2);
        return;
    }
    const int a = r, b = (r + 1) % 3, c = (r + 2) % 3, mm = 3 + r, p = 3 + (r + 1) % 3, q = 3 + (r + 2) % 3;
    if (st[(r + 2) % 3]) { put(a, mm, q); put(q, mm, c); } else put(a, mm, c);
    if (st[(r + 1) % 3]) { put(mm, b, p); put(mm, p, c); } else put(mm, b, c);
}

// curve index (-1: none) of every boundary edge, in the surf order of the element type (P2: visit order 1, 2, 0; P4: 0, 1, 2)
__global__ void __launch_bounds__(kBlock) surf_curve_kernel(MeshView M, CurveSet S, int p2, int32_t* __restrict__ curve_of_surf) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= M.n_e) return;
    const int m = M.mask[i];
    if (!(m >> 3)) return;
    for (int k = 0; k < 3; ++k) {
        if (!((m >> (3 + k)) & 1)) continue;
        const int32_t A = M.elem[(int64_t)k * M.n_e + i], B = M.elem[(int64_t)((k + 1) % 3) * M.n_e + i];
        const int64_t at = M.bbase[i] + (p2 ? bnd_rank_p2(m, k) : __popc((m >> 3) & ((1 << k) - 1)));
        curve_of_surf[at] = edge_curve(S, M.coord[A], M.coord[M.n_n + A], M.coord[B], M.coord[M.n_n + B]);
    }
}

// ---- area statistics: min doubled area, sum of areas, count of doubled areas <= 0 ------------------------------------------
// Doubled signed area d = (x2 - x1)(y3 - y1) - (x3 - x1)(y2 - y1).  A fixed grid (a function of n_e alone), a grid-stride
// loop per lane, a tree over the workgroup in LDS, one partial per workgroup, a second tree over the partials in one
// workgroup: the order of every sum is fixed, no atomics.  A triangle naming a node outside [0, n_n) reads nothing and
// counts as d = 0.
constexpr int kAreaMaxBlocks = 1024;

__device__ __forceinline__ void area_tree(double* __restrict__ l_min, double* __restrict__ l_sum, double* __restrict__ l_cnt) {
    for (int d = kBlock / 2; d > 0; d /= 2) {
        __syncthreads();
        if (threadIdx.x < (unsigned)d) {
            const double o = l_min[threadIdx.x + d];
            l_min[threadIdx.x] = o < l_min[threadIdx.x] ? o : l_min[threadIdx.x];
            l_sum[threadIdx.x] += l_sum[threadIdx.x + d];
            l_cnt[threadIdx.x] += l_cnt[threadIdx.x + d];
        }
    }
    __syncthreads();
}

__global__ void __launch_bounds__(kBlock) area_partial_kernel(int64_t n_e, int64_t n_n, const int32_t* __restrict__ elem,
                                                              const double* __restrict__ coord, double* __restrict__ part) {
    __shared__ double l_min[kBlock], l_sum[kBlock], l_cnt[kBlock];
    double mn = INFINITY, sum = 0, cnt = 0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n_e; i += (int64_t)gridDim.x * kBlock) {
        const int32_t a = elem[i], b = elem[n_e + i], c = elem[2 * n_e + i];
        double d = 0;
        if (a >= 0 && a < n_n && b >= 0 && b < n_n && c >= 0 && c < n_n) {
            const double x1 = coord[a], y1 = coord[n_n + a];
            d = (coord[b] - x1) * (coord[n_n + c] - y1) - (coord[c] - x1) * (coord[n_n + b] - y1);
        }
        mn = d < mn ? d : mn;
        sum += d / 2;
        cnt += d <= 0 ? 1 : 0;
    }
    l_min[threadIdx.x] = mn;
    l_sum[threadIdx.x] = sum;
    l_cnt[threadIdx.x] = cnt;
    area_tree(l_min, l_sum, l_cnt);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = l_min[0];
        part[gridDim.x + blockIdx.x] = l_sum[0];
        part[2 * gridDim.x + blockIdx.x] = l_cnt[0];
    }
}

__global__ void __launch_bounds__(kBlock) area_final_kernel(int n_part, const double* __restrict__ part, int64_t n_e,
                                                            double* __restrict__ out) {
    __shared__ double l_min[kBlock], l_sum[kBlock], l_cnt[kBlock];
    double mn = INFINITY, sum = 0, cnt = 0;
    for (int b = threadIdx.x; b < n_part; b += kBlock) {
        mn = part[b] < mn ? part[b] : mn;
        sum += part[n_part + b];
        cnt += part[2 * n_part + b];
    }
    l_min[threadIdx.x] = mn;
    l_sum[threadIdx.x] = sum;
    l_cnt[threadIdx.x] = cnt;
    area_tree(l_min, l_sum, l_cnt);
    if (threadIdx.x == 0) {
        out[0] = l_min[0];
        out[1] = l_sum[0];
        out[2] = l_cnt[0];
        out[3] = (double)n_e;
    }
}

// ---- error indicator: fixed-order sums, statistics and bulk marking (include/fep.h, "recovered-stress error indicator") ----
// T(v): in every block of kBlock consecutive values x[i] = x[i] + x[i + s] for s = 128, 64, ..., 1 (i < s), then T of the block
// sums.  One launch per level; the workgroup that finds itself alone on its level finishes the pass.  A pass carries three
// values per block: the tree sum, the maximum and a count (a tree sum of small integers, exact in any order).
struct IndState {                                            // one per (device, stream), at the head of the scratch
    unsigned long long cand;                                 // bits of the largest t found so far with tail(t) >= goal
    double total, vmax, goal;
};
enum { kIndStats = 0, kIndTrial = 1, kIndFinal = 2 };

__device__ __forceinline__ void ind_tree(double* __restrict__ l_sum, double* __restrict__ l_max, double* __restrict__ l_cnt) {
    for (int d = kBlock / 2; d > 0; d /= 2) {
        __syncthreads();
        if (threadIdx.x < (unsigned)d) {
            const double o = l_max[threadIdx.x + d];
            l_sum[threadIdx.x] = l_sum[threadIdx.x] + l_sum[threadIdx.x + d];
            l_max[threadIdx.x] = o > l_max[threadIdx.x] ? o : l_max[threadIdx.x];
            l_cnt[threadIdx.x] = l_cnt[threadIdx.x] + l_cnt[threadIdx.x + d];
        }
    }
    __syncthreads();
}

__device__ __forceinline__ double ind_threshold(const IndState* __restrict__ state, int mode, int bit) {
    if (mode == kIndTrial) return __longlong_as_double((long long)(state->cand | (1ull << bit)));
    return state->total > 0 ? __longlong_as_double((long long)state->cand) : INFINITY;        // kIndFinal: t*
}

// kLeaf: the values come from eta2 (filtered as the mode says); else from the partials of the level below.
template <bool kLeaf>
__global__ void __launch_bounds__(kBlock) ind_level_kernel(int64_t n, const double* __restrict__ eta2, const double* __restrict__ in,
                                                           int64_t n_in, int mode, int bit, double theta, IndState* __restrict__ state,
                                                           uint8_t* __restrict__ marked, double* __restrict__ part,
                                                           double* __restrict__ stats, double* __restrict__ out) {
    __shared__ double l_sum[kBlock], l_max[kBlock], l_cnt[kBlock];
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    double v = 0.0, mx = 0.0, cnt = 0.0;                     // the padding
    if (kLeaf) {
        if (i < n) {
            const double x = eta2[i];
            const bool fin = x - x == 0.0;                   // false for NaN and both infinities
            if (mode == kIndStats) {
                v = fin ? x : 0.0;
                mx = v > 0.0 ? v : 0.0;
                cnt = fin ? 0.0 : 1.0;
            } else {
                const bool keep = fin && x >= ind_threshold(state, mode, bit);
                v = keep ? x : 0.0;
                if (mode == kIndFinal) {
                    const bool mk = keep && x > 0.0;
                    marked[i] = mk ? 1 : 0;
                    cnt = mk ? 1.0 : 0.0;
                }
            }
        }
    } else if (i < n_in) {
        v = in[i];
        mx = in[n_in + i];
        cnt = in[2 * n_in + i];
    }
    l_sum[threadIdx.x] = v;
    l_max[threadIdx.x] = mx;
    l_cnt[threadIdx.x] = cnt;
    ind_tree(l_sum, l_max, l_cnt);
    if (threadIdx.x != 0) return;
    if (gridDim.x > 1) {
        part[blockIdx.x] = l_sum[0];
        part[gridDim.x + blockIdx.x] = l_max[0];
        part[2 * gridDim.x + blockIdx.x] = l_cnt[0];
        return;
    }
    const double sum = l_sum[0];
    if (mode == kIndStats) {
        if (stats) { stats[0] = sum; stats[1] = l_max[0]; stats[2] = l_cnt[0]; stats[3] = (double)n; }
        if (state) { state->cand = 0; state->total = sum; state->vmax = l_max[0]; state->goal = theta * sum; }
    } else if (mode == kIndTrial) {
        const unsigned long long t = state->cand | (1ull << bit);
        if (state->total > 0 && t <= (unsigned long long)__double_as_longlong(state->vmax) && sum >= state->goal) state->cand = t;
    } else {
        out[0] = ind_threshold(state, kIndFinal, 0);
        out[1] = sum;
        out[2] = l_cnt[0];
        out[3] = state->total;
    }
}

using fep_stage::reserve_as;
using fep_stage::ScopedStore;

// Device blocks of a mesh (fep_mesh::blocks: made once at their final size, released with the mesh), ...
enum MeshBuf { kMeshElem, kMeshCoord, kMeshNbr, kMeshMask, kMeshBase, kMeshBbase, kMeshMarkIn, kMeshMarkBits, kMeshMarkRef,
               kMeshMarkErank, kMeshMarkCbase, kMeshMarkScan, kMeshMarkWords };
// ... of the analysis in fep_mesh_create (released when it returns) ...
enum CreateBuf { kTmpPtr, kTmpCursor, kTmpList, kTmpCounters, kTmpScan };
// ... and of one host-form call (a store of the call: allocated by it, released when it returns; nothing persists)
enum CallBuf { kCallElem, kCallCoord, kCallSurf, kCallElemEd, kCallEdgeEl, kCallParent, kCallEta2, kCallMarked, kCallStats,
               kCallCorners };

}  // namespace

struct fep_mesh {
    int device = 0;
    int64_t n_e = 0, n_n = 0, n_edges = 0, n_bnd = 0, n_nonmanifold = 0, n_inconsistent = 0, n_degenerate = 0;
    int32_t* elem = nullptr;
    double* coord = nullptr;
    int32_t* nbr = nullptr;
    uint8_t* mask = nullptr;
    int32_t* base = nullptr;
    int32_t* bbase = nullptr;
    CurveSet curves{};
    // closed marks of fep_mesh_mark (scratch made by its first call, kept with the mesh)
    bool has_marks = false, m_ready = false;
    int64_t n_child = 0, n_new = 0;
    uint8_t* m_in = nullptr;      // the caller's marks, when they came from the host
    uint8_t* m_bits = nullptr;
    uint8_t* m_ref = nullptr;
    int32_t* m_erank = nullptr;   // (n_edges + 1) rank of every edge among the marked ones
    int32_t* m_cbase = nullptr;   // (n_e + 1) first child of every element
    int32_t* m_scan = nullptr;
    int32_t* m_words = nullptr;   // {changed, elements with a marked edge}
    ScopedStore blocks;

    bool refused() const { return n_nonmanifold > 0 || n_inconsistent > 0 || n_degenerate > 0; }
    MeshView view() const { return MeshView{n_e, n_n, n_edges, n_bnd, elem, coord, nbr, mask, base, bbase}; }
};

static int mesh_create_impl(fep_mesh** out, int device_id, hipStream_t st, int64_t n_e, int64_t n_n, const int32_t* elem,
                            const double* coord, int on_device) {
    if (!out) return FEP_EINVAL;
    *out = nullptr;
    if (n_e < 1 || n_n < 0 || !elem || (!coord && n_n > 0)) return FEP_EINVAL;
    if (n_n >= (int64_t)INT32_MAX || 4 * n_e >= (int64_t)INT32_MAX) return FEP_ERANGE;
    FEP_TRY(fep_set_device(device_id));
    fep_mesh* M = new fep_mesh();
    struct Guard {
        fep_mesh* m;
        ~Guard() { delete m; }
    } guard{M};
    M->device = device_id;
    M->n_e = n_e;
    M->n_n = n_n;
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    FEP_TRY(reserve_as(M->blocks, kMeshElem, 3 * n_e, st, &M->elem));
    FEP_TRY(reserve_as(M->blocks, kMeshCoord, 2 * n_n, st, &M->coord));
    FEP_TRY(reserve_as(M->blocks, kMeshNbr, 3 * n_e, st, &M->nbr));
    FEP_TRY(reserve_as(M->blocks, kMeshMask, n_e, st, &M->mask));
    FEP_TRY(reserve_as(M->blocks, kMeshBase, n_e + 1, st, &M->base));
    FEP_TRY(reserve_as(M->blocks, kMeshBbase, n_e + 1, st, &M->bbase));
    HIP_TRY(hipMemcpyAsync(M->elem, elem, (size_t)(3 * n_e) * sizeof(int32_t), kind, st));
    if (n_n > 0) HIP_TRY(hipMemcpyAsync(M->coord, coord, (size_t)(2 * n_n) * sizeof(double), kind, st));
    // scratch of the analysis: released when this function returns (it synchronises first)
    ScopedStore tmp;
    int32_t *ptr = nullptr, *cursor = nullptr, *list = nullptr, *counters = nullptr, *scan = nullptr;
    const int64_t n_longest = (n_n > n_e ? n_n : n_e) + 1;
    FEP_TRY(reserve_as(tmp, kTmpPtr, n_n + 1, st, &ptr));
    FEP_TRY(reserve_as(tmp, kTmpCursor, n_n, st, &cursor));
    FEP_TRY(reserve_as(tmp, kTmpList, 3 * n_e, st, &list));
    FEP_TRY(reserve_as(tmp, kTmpCounters, C_COUNT, st, &counters));
    FEP_TRY(reserve_as(tmp, kTmpScan, scan_scratch_len(n_longest), st, &scan));
    HIP_TRY(hipMemsetAsync(ptr, 0, (size_t)(n_n + 1) * sizeof(int32_t), st));
    HIP_TRY(hipMemsetAsync(cursor, 0, (size_t)(n_n > 0 ? n_n : 1) * sizeof(int32_t), st));
    HIP_TRY(hipMemsetAsync(counters, 0, C_COUNT * sizeof(int32_t), st));
    HIP_TRY(hipMemsetAsync(M->base + n_e, 0, sizeof(int32_t), st));
    HIP_TRY(hipMemsetAsync(M->bbase + n_e, 0, sizeof(int32_t), st));
    const dim3 grid(grid_for(n_e, kBlock)), block(kBlock);
    hipLaunchKernelGGL(mesh_degree_kernel, grid, block, 0, st, n_e, n_n, M->elem, ptr, counters);
    HIP_TRY(hipGetLastError());
    FEP_TRY(scan_exclusive(st, n_n + 1, ptr, scan));
    hipLaunchKernelGGL(mesh_fill_kernel, grid, block, 0, st, n_e, n_n, M->elem, ptr, cursor, list);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(mesh_match_kernel, grid, block, 0, st, n_e, n_n, M->elem, ptr, list, M->nbr, M->mask, M->base, M->bbase,
                       counters);
    HIP_TRY(hipGetLastError());
    FEP_TRY(scan_exclusive(st, n_e + 1, M->base, scan));
    FEP_TRY(scan_exclusive(st, n_e + 1, M->bbase, scan));
    int32_t h_counters[C_COUNT] = {0, 0, 0, 0}, h_edges = 0, h_bnd = 0;
    HIP_TRY(hipMemcpyAsync(h_counters, counters, sizeof(h_counters), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&h_edges, M->base + n_e, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&h_bnd, M->bbase + n_e, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (h_counters[C_RANGE] > 0) return FEP_ERANGE;
    M->n_edges = h_edges;
    M->n_bnd = h_bnd;
    M->n_degenerate = h_counters[C_DEGENERATE];
    M->n_nonmanifold = h_counters[C_NONMANIFOLD];
    M->n_inconsistent = h_counters[C_INCONSISTENT];
    guard.m = nullptr;
    *out = M;
    return FEP_OK;
}

static int64_t mesh_new_nodes(const fep_mesh* M, int elem_type) {
    return elem_type == FEP_P2 ? M->n_edges : 3 * M->n_e + 3 * M->n_edges;
}

// check_*: the arguments of an entry point's two forms, in one place (host or device pointers: only tested for NULL)
static int check_enrich(const fep_mesh* M, int elem_type, const int32_t* elem_ext, const double* coord_ext, const int32_t* surf) {
    if (!M || (elem_type != FEP_P2 && elem_type != FEP_P4) || !elem_ext || !coord_ext || (!surf && M->n_bnd > 0)) return FEP_EINVAL;
    if (M->refused()) return FEP_ESTATE;
    return M->n_n + mesh_new_nodes(M, elem_type) >= (int64_t)INT32_MAX ? FEP_ERANGE : FEP_OK;
}

static int mesh_enrich_impl(const fep_mesh* M, hipStream_t st, int elem_type, int32_t* elem_ext, double* coord_ext, int32_t* surf,
                            int32_t* elem_ed, int32_t* edge_el) {
    FEP_TRY(check_enrich(M, elem_type, elem_ext, coord_ext, surf));
    const int64_t n_tot = M->n_n + mesh_new_nodes(M, elem_type);
    FEP_TRY(fep_set_device(M->device));
    for (int r = 0; r < 2 && M->n_n > 0; ++r)
        HIP_TRY(hipMemcpyAsync(coord_ext + r * n_tot, M->coord + r * M->n_n, (size_t)M->n_n * sizeof(double), hipMemcpyDeviceToDevice, st));
    const dim3 grid(grid_for(M->n_e, kBlock), 3), block(kBlock);
    if (elem_type == FEP_P2)
        hipLaunchKernelGGL(enrich_p2_kernel, grid, block, 0, st, M->view(), M->curves, elem_ext, coord_ext, surf, elem_ed, edge_el);
    else
        hipLaunchKernelGGL(enrich_p4_kernel, grid, block, 0, st, M->view(), M->curves, elem_ext, coord_ext, surf);
    HIP_TRY(hipGetLastError());
    return FEP_OK;
}

static int check_refine(const fep_mesh* M, const int32_t* elem_child, const double* coord_ext) {
    if (!M || !elem_child || !coord_ext) return FEP_EINVAL;
    if (M->refused()) return FEP_ESTATE;
    return M->n_n + M->n_edges >= (int64_t)INT32_MAX ? FEP_ERANGE : FEP_OK;
}

static int mesh_refine_impl(const fep_mesh* M, hipStream_t st, int32_t* elem_child, double* coord_ext) {
    FEP_TRY(check_refine(M, elem_child, coord_ext));
    const int64_t n_tot = M->n_n + M->n_edges;
    FEP_TRY(fep_set_device(M->device));
    for (int r = 0; r < 2 && M->n_n > 0; ++r)
        HIP_TRY(hipMemcpyAsync(coord_ext + r * n_tot, M->coord + r * M->n_n, (size_t)M->n_n * sizeof(double), hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(refine_kernel, dim3(grid_for(M->n_e, kBlock)), dim3(kBlock), 0, st, M->view(), M->curves, elem_child, coord_ext);
    HIP_TRY(hipGetLastError());
    return FEP_OK;
}

// sweeps enqueued between two reads of the `changed` word: a chain of reference edges crosses at least one workgroup per sweep
constexpr int kSweepsPerRead = 4;

// 1 if p is memory of GPU `device` (or managed memory), 0 if it is host memory, pinned or not, -1 if it is another GPU's
static int pointer_on_device(const void* p, int device) {
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();                             // runtimes that do not know a plain host pointer say so this way
        return 0;
    }
    if (a.type == hipMemoryTypeManaged) return 1;
    if (a.type != hipMemoryTypeDevice) return 0;
    return a.device == device ? 1 : -1;
}

static int mesh_mark_impl(fep_mesh* M, hipStream_t st, const uint8_t* marked, int on_device, int64_t* out) {
    if (!M || !marked || !out) return FEP_EINVAL;
    if (M->refused()) return FEP_ESTATE;
    FEP_TRY(fep_set_device(M->device));
    if (pointer_on_device(marked, M->device) != (on_device ? 1 : 0)) return FEP_EINVAL;
    const int64_t n_e = M->n_e, n_edges = M->n_edges;
    if (!M->m_ready) {                                       // each block once (those an earlier call made before it ran out of memory are kept)
        const int64_t n_longest = (n_edges > n_e ? n_edges : n_e) + 1;
        FEP_TRY(reserve_as(M->blocks, kMeshMarkBits, n_e, st, &M->m_bits));
        FEP_TRY(reserve_as(M->blocks, kMeshMarkRef, n_e, st, &M->m_ref));
        FEP_TRY(reserve_as(M->blocks, kMeshMarkErank, n_edges + 1, st, &M->m_erank));
        FEP_TRY(reserve_as(M->blocks, kMeshMarkCbase, n_e + 1, st, &M->m_cbase));
        FEP_TRY(reserve_as(M->blocks, kMeshMarkScan, scan_scratch_len(n_longest), st, &M->m_scan));
        FEP_TRY(reserve_as(M->blocks, kMeshMarkWords, 2, st, &M->m_words));
        M->m_ready = true;
    }
    if (!on_device) FEP_TRY(reserve_as(M->blocks, kMeshMarkIn, n_e, st, &M->m_in));   // only meshes that are ever marked from the host
    M->has_marks = false;
    if (!on_device) {
        HIP_TRY(hipMemcpyAsync(M->m_in, marked, (size_t)n_e, hipMemcpyHostToDevice, st));
        marked = M->m_in;
    }
    const dim3 grid(grid_for(n_e, kBlock)), block(kBlock);
    hipLaunchKernelGGL(mark_init_kernel, grid, block, 0, st, M->view(), marked, M->m_bits, M->m_ref);
    HIP_TRY(hipGetLastError());
    int64_t n_sweeps = 0;
    int32_t h_words[2] = {1, 0};
    while (h_words[0]) {
        HIP_TRY(hipMemsetAsync(M->m_words, 0, 2 * sizeof(int32_t), st));
        for (int s = 0; s < kSweepsPerRead; ++s) {
            hipLaunchKernelGGL(mark_sweep_kernel, grid, block, 0, st, n_e, M->nbr, M->m_ref, M->m_bits, M->m_words);
            HIP_TRY(hipGetLastError());
        }
        n_sweeps += kSweepsPerRead;
        HIP_TRY(hipMemcpyAsync(h_words, M->m_words, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    HIP_TRY(hipMemsetAsync(M->m_erank + n_edges, 0, sizeof(int32_t), st));
    HIP_TRY(hipMemsetAsync(M->m_cbase + n_e, 0, sizeof(int32_t), st));
    hipLaunchKernelGGL(mark_count_kernel, grid, block, 0, st, M->view(), M->m_bits, M->m_erank, M->m_cbase, M->m_words + 1);
    HIP_TRY(hipGetLastError());
    FEP_TRY(scan_exclusive(st, n_edges + 1, M->m_erank, M->m_scan));
    FEP_TRY(scan_exclusive(st, n_e + 1, M->m_cbase, M->m_scan));
    int32_t h_new = 0, h_child = 0;
    HIP_TRY(hipMemcpyAsync(&h_new, M->m_erank + n_edges, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&h_child, M->m_cbase + n_e, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h_words, M->m_words, sizeof(h_words), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    out[0] = h_child;
    out[1] = h_new;
    out[2] = h_words[1];
    out[3] = n_sweeps;
    // n_child <= 4 n_e < 2^31 - 1 (fep_mesh_create refuses larger meshes) and n_new <= n_edges <= 3 n_e, so neither int32 scan
    // can wrap; only the sum with n_n can pass int32
    if (M->n_n + (int64_t)h_new >= (int64_t)INT32_MAX) return FEP_ERANGE;
    M->n_child = h_child;
    M->n_new = h_new;
    M->has_marks = true;
    return FEP_OK;
}

static int check_refine_marked(const fep_mesh* M, const int32_t* elem_child, const double* coord_ext) {
    if (!M || !elem_child || !coord_ext) return FEP_EINVAL;
    return M->refused() || !M->has_marks ? FEP_ESTATE : FEP_OK;
}

static int mesh_refine_marked_impl(const fep_mesh* M, hipStream_t st, int32_t* elem_child, double* coord_ext, int32_t* parent) {
    FEP_TRY(check_refine_marked(M, elem_child, coord_ext));
    const int64_t n_tot = M->n_n + M->n_new;
    FEP_TRY(fep_set_device(M->device));
    for (int r = 0; r < 2 && M->n_n > 0; ++r)
        HIP_TRY(hipMemcpyAsync(coord_ext + r * n_tot, M->coord + r * M->n_n, (size_t)M->n_n * sizeof(double), hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(refine_marked_kernel, dim3(grid_for(M->n_e, kBlock)), dim3(kBlock), 0, st, M->view(), M->curves, M->m_bits,
                       M->m_ref, M->m_erank, M->m_cbase, n_tot, M->n_child, elem_child, coord_ext, parent);
    HIP_TRY(hipGetLastError());
    return FEP_OK;
}

static int check_child_corners(const fep_mesh* M, const uint8_t* corners) {
    if (!M || !corners) return FEP_EINVAL;
    return M->refused() || !M->has_marks ? FEP_ESTATE : FEP_OK;
}

static int mesh_child_corners_impl(const fep_mesh* M, hipStream_t st, uint8_t* corners) {
    FEP_TRY(check_child_corners(M, corners));
    FEP_TRY(fep_set_device(M->device));
    hipLaunchKernelGGL(child_corners_kernel, dim3(grid_for(M->n_e, kBlock)), dim3(kBlock), 0, st, M->view(), M->m_bits, M->m_ref, M->m_cbase,
                       M->n_child, corners);
    HIP_TRY(hipGetLastError());
    return FEP_OK;
}

static int mesh_set_curves_impl(fep_mesh* M, int n_curves, const double* curves_h) {
    if (!M || n_curves < 0 || n_curves > FEP_MAX_CURVES || (n_curves > 0 && !curves_h)) return FEP_EINVAL;
    CurveSet S{};
    for (int q = 0; q < n_curves; ++q) {
        const double* c = curves_h + 5 * q;
        for (int r = 0; r < 5; ++r)
            if (!std::isfinite(c[r])) return FEP_EINVAL;
        if (!(c[2] > 0) || !(c[3] > 0) || !(c[4] >= 0)) return FEP_EINVAL;
        for (int r = 0; r < 5; ++r) S.v[q][r] = c[r];
    }
    S.n = n_curves;
    M->curves = S;
    return FEP_OK;
}

static int check_surf_curve(const fep_mesh* M, int elem_type, const int32_t* curve_of_surf) {
    if (!M || (elem_type != FEP_P2 && elem_type != FEP_P4) || (!curve_of_surf && M->n_bnd > 0)) return FEP_EINVAL;
    return M->refused() ? FEP_ESTATE : FEP_OK;
}

static int mesh_surf_curve_impl(const fep_mesh* M, hipStream_t st, int elem_type, int32_t* curve_of_surf) {
    FEP_TRY(check_surf_curve(M, elem_type, curve_of_surf));
    FEP_TRY(fep_set_device(M->device));
    if (M->n_bnd == 0) return FEP_OK;
    hipLaunchKernelGGL(surf_curve_kernel, dim3(grid_for(M->n_e, kBlock)), dim3(kBlock), 0, st, M->view(), M->curves,
                       elem_type == FEP_P2 ? 1 : 0, curve_of_surf);
    HIP_TRY(hipGetLastError());
    return FEP_OK;
}

// the arguments of both forms (host or device pointers: only tested for NULL)
static int check_area_stats(int64_t n_e, int64_t n_n, const int32_t* elem, const double* coord, const double* out) {
    return n_e < 0 || n_n < 0 || !out || (n_e > 0 && (!elem || (!coord && n_n > 0))) ? FEP_EINVAL : FEP_OK;
}

static int area_stats_impl(int device_id, hipStream_t st, int64_t n_e, int64_t n_n, const int32_t* elem, const double* coord,
                           double* out) {
    FEP_TRY(check_area_stats(n_e, n_n, elem, coord, out));
    FEP_TRY(fep_set_device(device_id));
    // the partials: the fixed-size scratch of (device, stream), made by the first call on it (an allocation: refused,
    // FEP_ESTATE, while that stream is being captured) and kept
    double* part = nullptr;
    const size_t part_bytes = 3 * kAreaMaxBlocks * sizeof(double);
    FEP_TRY(stream_scratch(kScratchArea, device_id, st, part_bytes, part_bytes, (void**)&part));
    int64_t n_part = (n_e + kBlock - 1) / kBlock;
    n_part = n_part < 1 ? 1 : (n_part > kAreaMaxBlocks ? kAreaMaxBlocks : n_part);
    hipLaunchKernelGGL(area_partial_kernel, dim3((unsigned)n_part), dim3(kBlock), 0, st, n_e, n_n, elem, coord, part);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(area_final_kernel, dim3(1), dim3(kBlock), 0, st, (int)n_part, part, n_e, out);
    HIP_TRY(hipGetLastError());
    return FEP_OK;
}

// Scratch of the indicator's passes: IndState, then three partials per block of every level above the leaves.  The grow-only
// scratch of its (device, stream) (stream_scratch, fep_staging.h): growing is an allocation, refused (FEP_ESTATE) while the
// stream is being captured, and a block handed out is never freed.
constexpr int64_t kIndHead = 8;                             // doubles reserved for IndState
static int64_t ind_scratch_len(int64_t n) {
    int64_t len = kIndHead;
    for (int64_t nb = (n + kBlock - 1) / kBlock; nb > 1; nb = (nb + kBlock - 1) / kBlock) len += 3 * nb;
    return len;
}

static int ind_scratch(int device, hipStream_t st, int64_t n, double** out) {
    const size_t len = (size_t)ind_scratch_len(n);
    return stream_scratch(kScratchIndicator, device, st, len * sizeof(double), (len + len / 4) * sizeof(double), (void**)out);
}

// One pass over eta2: the leaves, then one launch per level until a single workgroup is left, which finishes the pass.
static int ind_pass(hipStream_t st, int64_t n, const double* eta2, int mode, int bit, double theta, double* scratch, bool use_state,
                    uint8_t* marked, double* stats, double* out) {
    IndState* state = use_state ? (IndState*)scratch : nullptr;
    double* part = scratch + kIndHead;
    int64_t nb = (n + kBlock - 1) / kBlock;
    if (nb < 1) nb = 1;
    hipLaunchKernelGGL(ind_level_kernel<true>, dim3((unsigned)nb), dim3(kBlock), 0, st, n, eta2, (const double*)nullptr, (int64_t)0,
                       mode, bit, theta, state, marked, part, stats, out);
    HIP_TRY(hipGetLastError());
    while (nb > 1) {
        const int64_t nb_up = (nb + kBlock - 1) / kBlock;
        double* part_up = part + 3 * nb;
        hipLaunchKernelGGL(ind_level_kernel<false>, dim3((unsigned)nb_up), dim3(kBlock), 0, st, n, (const double*)nullptr,
                           (const double*)part, nb, mode, bit, theta, state, (uint8_t*)nullptr, part_up, stats, out);
        HIP_TRY(hipGetLastError());
        part = part_up;
        nb = nb_up;
    }
    return FEP_OK;
}

// fep_api.hip's fep_estimate_dev: `reserve` before its own kernel (a refusal writes nothing), `stats` after it
__attribute__((visibility("hidden"))) int fep_indicator_reserve(int device, hipStream_t st, int64_t n) {
    double* scratch = nullptr;
    return ind_scratch(device, st, n, &scratch);
}

__attribute__((visibility("hidden"))) int fep_indicator_stats(int device, hipStream_t st, int64_t n, const double* eta2_d,
                                                              double* stats_d) {
    double* scratch = nullptr;
    FEP_TRY(ind_scratch(device, st, n, &scratch));
    return ind_pass(st, n, eta2_d, kIndStats, 0, 0.0, scratch, false, nullptr, stats_d, nullptr);
}

constexpr int kIndValueBits = 63;                           // trial passes of the descent: the bits of a non-negative double

static int check_mark_bulk(int64_t n, const double* eta2, double theta, const uint8_t* marked, const double* out) {
    return n < 0 || !out || (n > 0 && (!eta2 || !marked)) || !(theta > 0.0 && theta <= 1.0) ? FEP_EINVAL : FEP_OK;
}

static int mark_bulk_impl(int device_id, hipStream_t st, int64_t n, const double* eta2, double theta, uint8_t* marked, double* out) {
    FEP_TRY(check_mark_bulk(n, eta2, theta, marked, out));
    if (n >= (int64_t)INT32_MAX * kBlock) return FEP_ERANGE;
    FEP_TRY(fep_set_device(device_id));
    double* scratch = nullptr;
    FEP_TRY(ind_scratch(device_id, st, n, &scratch));
    FEP_TRY(ind_pass(st, n, eta2, kIndStats, 0, theta, scratch, true, nullptr, nullptr, nullptr));
    if (n > 0)
        for (int bit = kIndValueBits - 1; bit >= 0; --bit)
            FEP_TRY(ind_pass(st, n, eta2, kIndTrial, bit, theta, scratch, true, nullptr, nullptr, nullptr));
    return ind_pass(st, n, eta2, kIndFinal, 0, theta, scratch, true, marked, nullptr, out);
}

// Host forms: the caller's arrays staged through the device's engine (fep_stage::HostCall) into device blocks of this call
// (`store`, declared before the call: released after its scope has finished or drained the engine).  Outputs are as large as
// the mesh and a driver makes one mesh per level, so nothing is kept.  A NULL optional array gives a NULL device pointer.
static int mark_bulk_host_impl(int device_id, int64_t n, const double* eta2_h, double theta, uint8_t* marked_h, double* out_h) {
    FEP_TRY(check_mark_bulk(n, eta2_h, theta, marked_h, out_h));
    ScopedStore store;
    fep_stage::HostCall call(device_id, &store);
    const double* eta2 = call.in(kCallEta2, eta2_h, (size_t)n);
    uint8_t* marked = call.out(kCallMarked, marked_h, (size_t)n);
    double* out = call.out(kCallStats, out_h, 4);
    return call.run([&] { return mark_bulk_impl(device_id, call.stream(), n, eta2, theta, marked, out); });
}

static int mesh_enrich_host_impl(const fep_mesh* M, int elem_type, int32_t* elem_ext_h, double* coord_ext_h, int32_t* surf_h,
                                 int32_t* elem_ed_h, int32_t* edge_el_h) {
    FEP_TRY(check_enrich(M, elem_type, elem_ext_h, coord_ext_h, surf_h));
    const bool p2 = elem_type == FEP_P2;
    const int64_t n_tot = M->n_n + mesh_new_nodes(M, elem_type), n_p = p2 ? 6 : 15, n_s = p2 ? 3 : 5;
    ScopedStore store;
    fep_stage::HostCall call(M->device, &store);
    int32_t* elem_ext = call.out(kCallElem, elem_ext_h, (size_t)(n_p * M->n_e));
    double* coord_ext = call.out(kCallCoord, coord_ext_h, (size_t)(2 * n_tot));
    int32_t* surf = call.out(kCallSurf, surf_h, (size_t)(n_s * M->n_bnd));
    int32_t* elem_ed = call.out(kCallElemEd, p2 ? elem_ed_h : nullptr, (size_t)(3 * M->n_e));
    int32_t* edge_el = call.out(kCallEdgeEl, p2 ? edge_el_h : nullptr, (size_t)(2 * M->n_edges));
    return call.run([&] { return mesh_enrich_impl(M, call.stream(), elem_type, elem_ext, coord_ext, surf, elem_ed, edge_el); });
}

static int mesh_refine_host_impl(const fep_mesh* M, int32_t* elem_child_h, double* coord_ext_h) {
    FEP_TRY(check_refine(M, elem_child_h, coord_ext_h));
    ScopedStore store;
    fep_stage::HostCall call(M->device, &store);
    int32_t* child = call.out(kCallElem, elem_child_h, (size_t)(12 * M->n_e));
    double* coord_ext = call.out(kCallCoord, coord_ext_h, (size_t)(2 * (M->n_n + M->n_edges)));
    return call.run([&] { return mesh_refine_impl(M, call.stream(), child, coord_ext); });
}

static int mesh_refine_marked_host_impl(const fep_mesh* M, int32_t* elem_child_h, double* coord_ext_h, int32_t* parent_h) {
    FEP_TRY(check_refine_marked(M, elem_child_h, coord_ext_h));
    ScopedStore store;
    fep_stage::HostCall call(M->device, &store);
    int32_t* child = call.out(kCallElem, elem_child_h, (size_t)(3 * M->n_child));
    double* coord_ext = call.out(kCallCoord, coord_ext_h, (size_t)(2 * (M->n_n + M->n_new)));
    int32_t* parent = call.out(kCallParent, parent_h, (size_t)M->n_child);
    return call.run([&] { return mesh_refine_marked_impl(M, call.stream(), child, coord_ext, parent); });
}

static int mesh_child_corners_host_impl(const fep_mesh* M, uint8_t* corners_h) {
    FEP_TRY(check_child_corners(M, corners_h));
    ScopedStore store;
    fep_stage::HostCall call(M->device, &store);
    uint8_t* corners = call.out(kCallCorners, corners_h, (size_t)(3 * M->n_child));
    return call.run([&] { return mesh_child_corners_impl(M, call.stream(), corners); });
}

static int mesh_surf_curve_host_impl(const fep_mesh* M, int elem_type, int32_t* curve_of_surf_h) {
    FEP_TRY(check_surf_curve(M, elem_type, curve_of_surf_h));
    ScopedStore store;
    fep_stage::HostCall call(M->device, &store);
    int32_t* out = call.out(kCallSurf, curve_of_surf_h, (size_t)M->n_bnd);
    return call.run([&] { return mesh_surf_curve_impl(M, call.stream(), elem_type, out); });
}

static int area_stats_host_impl(int device_id, int64_t n_e, int64_t n_n, const int32_t* elem_h, const double* coord_h,
                                double* out_h) {
    FEP_TRY(check_area_stats(n_e, n_n, elem_h, coord_h, out_h));
    ScopedStore store;
    fep_stage::HostCall call(device_id, &store);
    const int32_t* elem = call.in(kCallElem, elem_h, (size_t)(3 * n_e));
    const double* coord = call.in(kCallCoord, coord_h, (size_t)(2 * n_n));
    double* out = call.out(kCallStats, out_h, 4);
    return call.run([&] { return area_stats_impl(device_id, call.stream(), n_e, n_n, elem, coord, out); });
}

extern "C" int fep_mesh_create(fep_mesh** mesh_out, int device_id, void* stream, int64_t n_e, int64_t n_n, const int32_t* elem,
                               const double* coord, int on_device) {
    FEP_GUARD(mesh_create_impl(mesh_out, device_id, (hipStream_t)stream, n_e, n_n, elem, coord, on_device))
}

extern "C" int fep_mesh_destroy(fep_mesh* mesh) {
    if (!mesh) return FEP_OK;
    (void)fep_set_device(mesh->device);
    delete mesh;
    return FEP_OK;
}

extern "C" int fep_mesh_info(const fep_mesh* mesh, int64_t info[7]) {
    if (!mesh || !info) return FEP_EINVAL;
    info[0] = mesh->n_e;
    info[1] = mesh->n_n;
    info[2] = mesh->n_edges;
    info[3] = mesh->n_bnd;
    info[4] = mesh->n_nonmanifold;
    info[5] = mesh->n_inconsistent;
    info[6] = mesh->n_degenerate;
    return FEP_OK;
}

extern "C" int fep_mesh_enrich_dev(const fep_mesh* mesh, void* stream, int elem_type, int32_t* elem_ext_d, double* coord_ext_d,
                                   int32_t* surf_d, int32_t* elem_ed_d, int32_t* edge_el_d) {
    FEP_GUARD(mesh_enrich_impl(mesh, (hipStream_t)stream, elem_type, elem_ext_d, coord_ext_d, surf_d, elem_ed_d, edge_el_d))
}

extern "C" int fep_mesh_enrich_host(const fep_mesh* mesh, int elem_type, int32_t* elem_ext_h, double* coord_ext_h, int32_t* surf_h,
                                    int32_t* elem_ed_h, int32_t* edge_el_h) {
    FEP_GUARD(mesh_enrich_host_impl(mesh, elem_type, elem_ext_h, coord_ext_h, surf_h, elem_ed_h, edge_el_h))
}

extern "C" int fep_mesh_refine_dev(const fep_mesh* mesh, void* stream, int32_t* elem_child_d, double* coord_ext_d) {
    FEP_GUARD(mesh_refine_impl(mesh, (hipStream_t)stream, elem_child_d, coord_ext_d))
}

extern "C" int fep_mesh_refine_host(const fep_mesh* mesh, int32_t* elem_child_h, double* coord_ext_h) {
    FEP_GUARD(mesh_refine_host_impl(mesh, elem_child_h, coord_ext_h))
}

extern "C" int fep_mesh_mark(fep_mesh* mesh, void* stream, const uint8_t* marked, int on_device, int64_t out[4]) {
    FEP_GUARD(mesh_mark_impl(mesh, (hipStream_t)stream, marked, on_device, out))
}

extern "C" int fep_mesh_refine_marked_dev(const fep_mesh* mesh, void* stream, int32_t* elem_child_d, double* coord_ext_d, int32_t* parent_d) {
    FEP_GUARD(mesh_refine_marked_impl(mesh, (hipStream_t)stream, elem_child_d, coord_ext_d, parent_d))
}

extern "C" int fep_mesh_refine_marked_host(const fep_mesh* mesh, int32_t* elem_child_h, double* coord_ext_h, int32_t* parent_h) {
    FEP_GUARD(mesh_refine_marked_host_impl(mesh, elem_child_h, coord_ext_h, parent_h))
}

extern "C" int fep_mesh_child_corners_dev(const fep_mesh* mesh, void* stream, uint8_t* corners_d) {
    FEP_GUARD(mesh_child_corners_impl(mesh, (hipStream_t)stream, corners_d))
}

extern "C" int fep_mesh_child_corners_host(const fep_mesh* mesh, uint8_t* corners_h) {
    FEP_GUARD(mesh_child_corners_host_impl(mesh, corners_h))
}

extern "C" int fep_mesh_set_curves(fep_mesh* mesh, int n_curves, const double* curves_h) {
    FEP_GUARD(mesh_set_curves_impl(mesh, n_curves, curves_h))
}

extern "C" int fep_mesh_surf_curve_dev(const fep_mesh* mesh, void* stream, int elem_type, int32_t* curve_of_surf_d) {
    FEP_GUARD(mesh_surf_curve_impl(mesh, (hipStream_t)stream, elem_type, curve_of_surf_d))
}

extern "C" int fep_mesh_surf_curve_host(const fep_mesh* mesh, int elem_type, int32_t* curve_of_surf_h) {
    FEP_GUARD(mesh_surf_curve_host_impl(mesh, elem_type, curve_of_surf_h))
}

extern "C" int fep_mesh_area_stats_dev(int device_id, void* stream, int64_t n_e, int64_t n_n, const int32_t* elem_d,
                                       const double* coord_d, double* out_d) {
    FEP_GUARD(area_stats_impl(device_id, (hipStream_t)stream, n_e, n_n, elem_d, coord_d, out_d))
}

extern "C" int fep_mesh_area_stats_host(int device_id, int64_t n_e, int64_t n_n, const int32_t* elem_h, const double* coord_h,
                                        double* out_h) {
    FEP_GUARD(area_stats_host_impl(device_id, n_e, n_n, elem_h, coord_h, out_h))
}

extern "C" int fep_mark_bulk_dev(int device_id, void* stream, int64_t n, const double* eta2_d, double theta, uint8_t* marked_d,
                                 double* out_d) {
    FEP_GUARD(mark_bulk_impl(device_id, (hipStream_t)stream, n, eta2_d, theta, marked_d, out_d))
}

extern "C" int fep_mark_bulk_host(int device_id, int64_t n, const double* eta2_h, double theta, uint8_t* marked_h, double* out_h) {
    FEP_GUARD(mark_bulk_host_impl(device_id, n, eta2_h, theta, marked_h, out_h))
}
