// State transfer across refinement (include/fep.h, "state transfer across refinement"): nodal fields through the parent's
// basis, per-point fields by the nearest parent point.  Context-free, triangle types only.  The library knows no basis
// function: the weights W and the nearest-point table come from the host (tables.py, transfer_tables), per SHAPE = the triple
// of corner codes that says where a child sits in its parent.
//
// Every sum is one IEEE double product and one addition per term in the order of the header, nothing is contracted, and the
// only atomics are integer minima whose result does not depend on the order (the owner of a child node), so two calls give
// the same bytes and so does the NumPy twin transfer.py.
#include "fep_common.h"
#include "fep_staging.h"

#pragma clang fp contract(off)

namespace {

constexpr int kBlock = 256;
constexpr int kMaxComp = 4;
constexpr unsigned long long kNoOwner = ~0ull;
constexpr unsigned long long kNanBits = 0x7ff8000000000000ull;   // the quiet NaN of 0.0 / 0.0 with a clear sign bit

inline unsigned grid_for(int64_t n, int per_block) { return (unsigned)((n + per_block - 1) / per_block); }

// shape index of child `ch` and its parent element; -1 for a child with a parent outside [0, n_e), a code above 5, or a
// triple that is no shape.  Reads nothing out of bounds whatever the arrays hold.
__device__ __forceinline__ int child_shape(const int32_t* __restrict__ parent, const uint8_t* __restrict__ corners,
                                           const int8_t* __restrict__ shape_of_code, int64_t n_e, int64_t n_child, int64_t ch,
                                           int64_t* e_out) {
    const int64_t e = parent[ch];
    const unsigned c0 = corners[ch], c1 = corners[n_child + ch], c2 = corners[2 * n_child + ch];
    *e_out = 0;
    if (e < 0 || e >= n_e || c0 > 5 || c1 > 5 || c2 > 5) return -1;
    const int s = shape_of_code[c0 + 6 * c1 + 36 * c2];
    if (s < 0 || s >= FEP_TRANSFER_SHAPES) return -1;
    *e_out = e;
    return s;
}

// owner[node] = the lowest pair index ch * N_P + j among the (child element, local node) pairs that hold the node: an
// integer minimum, so the order of the lanes does not matter.  Lanes run along ch (the rows of elem_child are contiguous).
template <int N_P>
__global__ void __launch_bounds__(kBlock) transfer_owner_kernel(int64_t n_child, int64_t n_n_child, const int32_t* __restrict__ elem_child,
                                                                unsigned long long* __restrict__ owner) {
    const int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (idx >= n_child * N_P) return;
    const int64_t j = idx / n_child, ch = idx % n_child;
    const int64_t node = elem_child[idx];
    if (node < 0 || node >= n_n_child) return;
    atomicMin(&owner[node], (unsigned long long)(ch * N_P + j));
}

// LPC lanes per child (the power of two that holds N_P), kBlock / LPC children per workgroup.  Lane a of a child stages the
// n_comp values of the parent's node a in LDS, once per child; after the barrier lane j sums row j of W[s] against them, if
// its pair owns the node.
template <int N_P, int LPC>
__global__ void __launch_bounds__(kBlock) transfer_nodes_kernel(int n_comp, int64_t n_e, int64_t n_n_parent, int64_t n_child,
                                                                int64_t n_n_child, const int32_t* __restrict__ elem_parent,
                                                                const int32_t* __restrict__ elem_child, const int32_t* __restrict__ parent,
                                                                const uint8_t* __restrict__ corners, const int8_t* __restrict__ shape_of_code,
                                                                const double* __restrict__ W, const double* __restrict__ u,
                                                                const unsigned long long* __restrict__ owner, double* __restrict__ u_child) {
    constexpr int kChildren = kBlock / LPC;
    __shared__ double l_u[kChildren][N_P][kMaxComp];
    __shared__ int l_bad[kChildren];
    const int g = threadIdx.x / LPC, j = threadIdx.x % LPC;
    const int64_t ch = (int64_t)blockIdx.x * kChildren + g;
    const bool active = ch < n_child && j < N_P;
    if (j == 0) l_bad[g] = 0;
    __syncthreads();
    int s = -1;
    if (active) {
        int64_t e;
        s = child_shape(parent, corners, shape_of_code, n_e, n_child, ch, &e);
        int64_t v = -1;
        if (s >= 0) v = elem_parent[(int64_t)j * n_e + e];
        if (v < 0 || v >= n_n_parent) {
            l_bad[g] = 1;                                      // every lane that finds fault writes the same value
            for (int i = 0; i < kMaxComp; ++i) l_u[g][j][i] = 0.0;
        } else {
            for (int i = 0; i < kMaxComp; ++i) l_u[g][j][i] = i < n_comp ? u[v * n_comp + i] : 0.0;
        }
    }
    __syncthreads();
    if (!active) return;
    const int64_t node = elem_child[(int64_t)j * n_child + ch];
    if (node < 0 || node >= n_n_child || owner[node] != (unsigned long long)(ch * N_P + j)) return;
    double* out = u_child + node * n_comp;
    if (l_bad[g]) {
        for (int i = 0; i < n_comp; ++i) out[i] = __longlong_as_double((long long)kNanBits);
        return;
    }
    const double* w = W + ((int64_t)s * N_P + j) * N_P;
    double acc[kMaxComp] = {0.0, 0.0, 0.0, 0.0};
    for (int a = 0; a < N_P; ++a) {
        const double wa = w[a];
        for (int i = 0; i < kMaxComp; ++i) acc[i] = acc[i] + wa * l_u[g][a][i];
    }
    for (int i = 0; i < n_comp; ++i) out[i] = acc[i];
}

// a node of no child element: NaN, the rule of fep_transform_*
__global__ void __launch_bounds__(kBlock) transfer_orphans_kernel(int n_comp, int64_t n_n_child, const unsigned long long* __restrict__ owner,
                                                                  double* __restrict__ u_child) {
    const int64_t n = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (n >= n_n_child || owner[n] != kNoOwner) return;
    for (int i = 0; i < n_comp; ++i) u_child[n * n_comp + i] = __longlong_as_double((long long)kNanBits);
}

// One lane per child point; the child's parent, codes and shape are looked up once, the rows copied in an inner loop as
// 64-bit words (a bitwise copy), stores contiguous along the point index.
template <int N_Q>
__global__ void __launch_bounds__(kBlock) transfer_points_kernel(int n_rows, int64_t n_e, int64_t n_child, const int32_t* __restrict__ parent,
                                                                 const uint8_t* __restrict__ corners, const int8_t* __restrict__ shape_of_code,
                                                                 const uint8_t* __restrict__ near, const unsigned long long* __restrict__ q,
                                                                 unsigned long long* __restrict__ q_child) {
    const int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x, n_cq = n_child * N_Q, n_eq = n_e * N_Q;
    if (idx >= n_cq) return;
    const int64_t ch = idx / N_Q;
    const int k = (int)(idx % N_Q);
    int64_t e;
    const int s = child_shape(parent, corners, shape_of_code, n_e, n_child, ch, &e);
    int64_t src = -1;
    if (s >= 0) {
        const int from = near[s * N_Q + k];
        if (from < N_Q) src = e * N_Q + from;
    }
    for (int r = 0; r < n_rows; ++r) q_child[(int64_t)r * n_cq + idx] = src < 0 ? kNanBits : q[(int64_t)r * n_eq + src];
}

// [a, a + na) and [b, b + nb) share a byte
inline bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return na > 0 && nb > 0 && x < y + nb && y < x + na;
}

struct TriShape { int n_p, n_q; };
inline bool tri_shape(int elem_type, TriShape* t) {
    if (elem_type == FEP_P1) *t = {3, 1};
    else if (elem_type == FEP_P2) *t = {6, 7};
    else if (elem_type == FEP_P4) *t = {15, 12};
    else return false;
    return true;
}

// the arguments of both forms of the node transfer (host or device pointers: tested for NULL and for an output that shares
// bytes with an input)
int check_nodes(int elem_type, int n_comp, int64_t n_e, int64_t n_n_parent, int64_t n_child, int64_t n_n_child, const int32_t* elem_parent,
                const int32_t* elem_child, const int32_t* parent, const uint8_t* corners, const int8_t* shape_of_code, const double* w,
                const double* u, const double* u_child) {
    TriShape t;
    if (!tri_shape(elem_type, &t) || n_comp < 1 || n_comp > kMaxComp || n_e < 0 || n_n_parent < 0 || n_child < 0 || n_n_child < 0)
        return FEP_EINVAL;
    if (!shape_of_code || !w || (n_e > 0 && !elem_parent) || (n_n_parent > 0 && !u) || (n_n_child > 0 && !u_child) ||
        (n_child > 0 && (!elem_child || !parent || !corners)))
        return FEP_EINVAL;
    if (n_e >= (int64_t)INT32_MAX || n_n_parent >= (int64_t)INT32_MAX || n_child >= (int64_t)INT32_MAX || n_n_child >= (int64_t)INT32_MAX)
        return FEP_ERANGE;
    const size_t out_bytes = (size_t)(n_n_child * n_comp) * sizeof(double);
    const bool shared = overlap(u_child, out_bytes, u, (size_t)(n_n_parent * n_comp) * sizeof(double)) ||
                        overlap(u_child, out_bytes, elem_parent, (size_t)(t.n_p * n_e) * sizeof(int32_t)) ||
                        overlap(u_child, out_bytes, elem_child, (size_t)(t.n_p * n_child) * sizeof(int32_t)) ||
                        overlap(u_child, out_bytes, parent, (size_t)n_child * sizeof(int32_t)) ||
                        overlap(u_child, out_bytes, corners, (size_t)(3 * n_child)) || overlap(u_child, out_bytes, shape_of_code, 216) ||
                        overlap(u_child, out_bytes, w, (size_t)(FEP_TRANSFER_SHAPES * t.n_p * t.n_p) * sizeof(double));
    return shared ? FEP_EINVAL : FEP_OK;
}

template <int N_P, int LPC>
void launch_nodes(hipStream_t st, int n_comp, int64_t n_e, int64_t n_n_parent, int64_t n_child, int64_t n_n_child, const int32_t* elem_parent,
                  const int32_t* elem_child, const int32_t* parent, const uint8_t* corners, const int8_t* shape_of_code, const double* w,
                  const double* u, unsigned long long* owner, double* u_child) {
    hipLaunchKernelGGL(transfer_owner_kernel<N_P>, dim3(grid_for(n_child * N_P, kBlock)), dim3(kBlock), 0, st, n_child, n_n_child, elem_child,
                       owner);
    hipLaunchKernelGGL((transfer_nodes_kernel<N_P, LPC>), dim3(grid_for(n_child, kBlock / LPC)), dim3(kBlock), 0, st, n_comp, n_e, n_n_parent,
                       n_child, n_n_child, elem_parent, elem_child, parent, corners, shape_of_code, w, u, owner, u_child);
}

int transfer_nodes_impl(int device_id, hipStream_t st, int elem_type, int n_comp, int64_t n_e, int64_t n_n_parent, int64_t n_child,
                        int64_t n_n_child, const int32_t* elem_parent, const int32_t* elem_child, const int32_t* parent, const uint8_t* corners,
                        const int8_t* shape_of_code, const double* w, const double* u, double* u_child) {
    FEP_TRY(check_nodes(elem_type, n_comp, n_e, n_n_parent, n_child, n_n_child, elem_parent, elem_child, parent, corners, shape_of_code, w, u,
                        u_child));
    FEP_TRY(fep_set_device(device_id));
    if (n_n_child == 0) return FEP_OK;
    // the owners: the grow-only scratch of (device, stream); growing is an allocation, refused (FEP_ESTATE) during a capture
    unsigned long long* owner = nullptr;
    const size_t bytes = (size_t)n_n_child * sizeof(unsigned long long);
    FEP_TRY(stream_scratch(kScratchTransfer, device_id, st, bytes, bytes + bytes / 4, (void**)&owner));
    HIP_TRY(hipMemsetAsync(owner, 0xFF, bytes, st));
    if (n_child > 0) {
        if (elem_type == FEP_P1)
            launch_nodes<3, 4>(st, n_comp, n_e, n_n_parent, n_child, n_n_child, elem_parent, elem_child, parent, corners, shape_of_code, w, u,
                               owner, u_child);
        else if (elem_type == FEP_P2)
            launch_nodes<6, 8>(st, n_comp, n_e, n_n_parent, n_child, n_n_child, elem_parent, elem_child, parent, corners, shape_of_code, w, u,
                               owner, u_child);
        else
            launch_nodes<15, 16>(st, n_comp, n_e, n_n_parent, n_child, n_n_child, elem_parent, elem_child, parent, corners, shape_of_code, w, u,
                                 owner, u_child);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(transfer_orphans_kernel, dim3(grid_for(n_n_child, kBlock)), dim3(kBlock), 0, st, n_comp, n_n_child, owner, u_child);
    HIP_TRY(hipGetLastError());
    return FEP_OK;
}

int check_points(int elem_type, int n_rows, int64_t n_e, int64_t n_child, const int32_t* parent, const uint8_t* corners,
                 const int8_t* shape_of_code, const uint8_t* near, const double* q, const double* q_child) {
    TriShape t;
    if (!tri_shape(elem_type, &t) || n_rows < 1 || n_e < 0 || n_child < 0) return FEP_EINVAL;
    if (!shape_of_code || !near || (n_e > 0 && !q) || (n_child > 0 && (!parent || !corners || !q_child))) return FEP_EINVAL;
    if (n_e >= (int64_t)INT32_MAX || n_child >= (int64_t)INT32_MAX) return FEP_ERANGE;
    const size_t out_bytes = (size_t)n_rows * (size_t)(n_child * t.n_q) * sizeof(double);
    const bool shared = overlap(q_child, out_bytes, q, (size_t)n_rows * (size_t)(n_e * t.n_q) * sizeof(double)) ||
                        overlap(q_child, out_bytes, parent, (size_t)n_child * sizeof(int32_t)) ||
                        overlap(q_child, out_bytes, corners, (size_t)(3 * n_child)) || overlap(q_child, out_bytes, shape_of_code, 216) ||
                        overlap(q_child, out_bytes, near, (size_t)(FEP_TRANSFER_SHAPES * t.n_q));
    return shared ? FEP_EINVAL : FEP_OK;
}

int transfer_points_impl(int device_id, hipStream_t st, int elem_type, int n_rows, int64_t n_e, int64_t n_child, const int32_t* parent,
                         const uint8_t* corners, const int8_t* shape_of_code, const uint8_t* near, const double* q, double* q_child) {
    FEP_TRY(check_points(elem_type, n_rows, n_e, n_child, parent, corners, shape_of_code, near, q, q_child));
    FEP_TRY(fep_set_device(device_id));
    if (n_child == 0) return FEP_OK;
    const unsigned long long* src = (const unsigned long long*)q;
    unsigned long long* dst = (unsigned long long*)q_child;
    if (elem_type == FEP_P1)
        hipLaunchKernelGGL(transfer_points_kernel<1>, dim3(grid_for(n_child, kBlock)), dim3(kBlock), 0, st, n_rows, n_e, n_child, parent, corners,
                           shape_of_code, near, src, dst);
    else if (elem_type == FEP_P2)
        hipLaunchKernelGGL(transfer_points_kernel<7>, dim3(grid_for(n_child * 7, kBlock)), dim3(kBlock), 0, st, n_rows, n_e, n_child, parent,
                           corners, shape_of_code, near, src, dst);
    else
        hipLaunchKernelGGL(transfer_points_kernel<12>, dim3(grid_for(n_child * 12, kBlock)), dim3(kBlock), 0, st, n_rows, n_e, n_child, parent,
                           corners, shape_of_code, near, src, dst);
    HIP_TRY(hipGetLastError());
    return FEP_OK;
}

// Host forms: the caller's arrays staged through the device's engine into device blocks of this call, as the mesh host forms
// are (fep_mesh.hip); the owner scratch is that of the engine's stream.
enum CallBuf { kCallElemParent, kCallElemChild, kCallParent, kCallCorners, kCallShapeOfCode, kCallTable, kCallIn, kCallOut };

int transfer_nodes_host_impl(int device_id, int elem_type, int n_comp, int64_t n_e, int64_t n_n_parent, int64_t n_child, int64_t n_n_child,
                             const int32_t* elem_parent_h, const int32_t* elem_child_h, const int32_t* parent_h, const uint8_t* corners_h,
                             const int8_t* shape_of_code_h, const double* w_h, const double* u_h, double* u_child_h) {
    FEP_TRY(check_nodes(elem_type, n_comp, n_e, n_n_parent, n_child, n_n_child, elem_parent_h, elem_child_h, parent_h, corners_h,
                        shape_of_code_h, w_h, u_h, u_child_h));
    TriShape t;
    tri_shape(elem_type, &t);
    fep_stage::ScopedStore store;
    fep_stage::HostCall call(device_id, &store);
    const int32_t* elem_parent = call.in(kCallElemParent, elem_parent_h, (size_t)(t.n_p * n_e));
    const int32_t* elem_child = call.in(kCallElemChild, elem_child_h, (size_t)(t.n_p * n_child));
    const int32_t* parent = call.in(kCallParent, parent_h, (size_t)n_child);
    const uint8_t* corners = call.in(kCallCorners, corners_h, (size_t)(3 * n_child));
    const int8_t* shape_of_code = call.in(kCallShapeOfCode, shape_of_code_h, 216);
    const double* w = call.in(kCallTable, w_h, (size_t)(FEP_TRANSFER_SHAPES * t.n_p * t.n_p));
    const double* u = call.in(kCallIn, u_h, (size_t)(n_n_parent * n_comp));
    double* u_child = call.out(kCallOut, u_child_h, (size_t)(n_n_child * n_comp));
    return call.run([&] {
        return transfer_nodes_impl(device_id, call.stream(), elem_type, n_comp, n_e, n_n_parent, n_child, n_n_child, elem_parent, elem_child,
                                   parent, corners, shape_of_code, w, u, u_child);
    });
}

int transfer_points_host_impl(int device_id, int elem_type, int n_rows, int64_t n_e, int64_t n_child, const int32_t* parent_h,
                              const uint8_t* corners_h, const int8_t* shape_of_code_h, const uint8_t* near_h, const double* q_h,
                              double* q_child_h) {
    FEP_TRY(check_points(elem_type, n_rows, n_e, n_child, parent_h, corners_h, shape_of_code_h, near_h, q_h, q_child_h));
    TriShape t;
    tri_shape(elem_type, &t);
    fep_stage::ScopedStore store;
    fep_stage::HostCall call(device_id, &store);
    const int32_t* parent = call.in(kCallParent, parent_h, (size_t)n_child);
    const uint8_t* corners = call.in(kCallCorners, corners_h, (size_t)(3 * n_child));
    const int8_t* shape_of_code = call.in(kCallShapeOfCode, shape_of_code_h, 216);
    const uint8_t* near = call.in(kCallTable, near_h, (size_t)(FEP_TRANSFER_SHAPES * t.n_q));
    const double* q = call.in(kCallIn, q_h, (size_t)n_rows * (size_t)(n_e * t.n_q));
    double* q_child = call.out(kCallOut, q_child_h, (size_t)n_rows * (size_t)(n_child * t.n_q));
    return call.run([&] {
        return transfer_points_impl(device_id, call.stream(), elem_type, n_rows, n_e, n_child, parent, corners, shape_of_code, near, q, q_child);
    });
}

}  // namespace

extern "C" int fep_transfer_nodes_dev(int device_id, void* stream, int elem_type, int n_comp, int64_t n_e, int64_t n_n_parent, int64_t n_child,
                                      int64_t n_n_child, const int32_t* elem_parent_d, const int32_t* elem_child_d, const int32_t* parent_d,
                                      const uint8_t* corners_d, const int8_t* shape_of_code_d, const double* w_d, const double* u_d,
                                      double* u_child_d) {
    FEP_GUARD(transfer_nodes_impl(device_id, (hipStream_t)stream, elem_type, n_comp, n_e, n_n_parent, n_child, n_n_child, elem_parent_d,
                                  elem_child_d, parent_d, corners_d, shape_of_code_d, w_d, u_d, u_child_d))
}

extern "C" int fep_transfer_nodes_host(int device_id, int elem_type, int n_comp, int64_t n_e, int64_t n_n_parent, int64_t n_child,
                                       int64_t n_n_child, const int32_t* elem_parent_h, const int32_t* elem_child_h, const int32_t* parent_h,
                                       const uint8_t* corners_h, const int8_t* shape_of_code_h, const double* w_h, const double* u_h,
                                       double* u_child_h) {
    FEP_GUARD(transfer_nodes_host_impl(device_id, elem_type, n_comp, n_e, n_n_parent, n_child, n_n_child, elem_parent_h, elem_child_h, parent_h,
                                       corners_h, shape_of_code_h, w_h, u_h, u_child_h))
}

extern "C" int fep_transfer_points_dev(int device_id, void* stream, int elem_type, int n_rows, int64_t n_e, int64_t n_child,
                                       const int32_t* parent_d, const uint8_t* corners_d, const int8_t* shape_of_code_d, const uint8_t* near_d,
                                       const double* q_d, double* q_child_d) {
    FEP_GUARD(transfer_points_impl(device_id, (hipStream_t)stream, elem_type, n_rows, n_e, n_child, parent_d, corners_d, shape_of_code_d, near_d,
                                   q_d, q_child_d))
}

extern "C" int fep_transfer_points_host(int device_id, int elem_type, int n_rows, int64_t n_e, int64_t n_child, const int32_t* parent_h,
                                        const uint8_t* corners_h, const int8_t* shape_of_code_h, const uint8_t* near_h, const double* q_h,
                                        double* q_child_h) {
    FEP_GUARD(transfer_points_host_impl(device_id, elem_type, n_rows, n_e, n_child, parent_h, corners_h, shape_of_code_h, near_h, q_h,
                                        q_child_h))
}
