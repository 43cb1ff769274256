// Device memory of the Krylov solver (fep_solver.hip) and the part of its multigrid set-up that launches no kernel: the
// upload of one level of the hierarchy (fep_solver_amg_push_level) and dropping all of them.
//
// Every device array of the solver is a DeviceArray: it frees its block when it goes out of scope, so a set-up step that
// fails half way returns and leaves nothing allocated, and a level is dropped by levels.pop_back() / levels.clear().
// Allocation and upload report through HIP_TRY: hipErrorOutOfMemory gives FEP_ENOMEM, any other failure FEP_EHIP, and
// fep_last_hip_error() names it.
//
// As fep_staging.h: with FEP_STAGING_HOST_STUB defined this header includes no HIP header and uses the stand-ins of the
// including driver (tests/staging_san.cpp: hipMalloc / hipFree / hipMemcpy on heap memory, a counter that makes the n-th
// allocation fail, HIP_TRY, FEP_TRY, fep_set_device), so that push_level runs under the sanitizers on the CPU with every
// one of its allocations made to fail in turn.
#pragma once
#ifndef FEP_STAGING_HOST_STUB
#include "fep_common.h"
#endif
#include "fep_host.h"

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <utility>
#include <vector>

namespace fep_levels {

// `count` elements of T in device memory, owned; move-only.  Converts to T* where a kernel argument is wanted.
template <class T> class DeviceArray {
    T* p = nullptr;
    int64_t n = 0;

public:
    DeviceArray() = default;
    DeviceArray(const DeviceArray&) = delete;
    DeviceArray& operator=(const DeviceArray&) = delete;
    DeviceArray(DeviceArray&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
    DeviceArray& operator=(DeviceArray&& o) noexcept {
        if (this != &o) { reset(); p = o.p; n = o.n; o.p = nullptr; o.n = 0; }
        return *this;
    }
    ~DeviceArray() { reset(); }
    void reset() {
        if (p) (void)hipFree(p);                        // (a pointer of any device)
        p = nullptr; n = 0;
    }
    // at least one element, uninitialised; what the array held before is freed first; empty after a failure
    int alloc(int64_t count) {
        reset();
        count = std::max<int64_t>(count, 1);
        void* q = nullptr;
        HIP_TRY(hipMalloc(&q, (size_t)count * sizeof(T)));
        p = static_cast<T*>(q); n = count;
        return FEP_OK;
    }
    int upload(const T* src, int64_t count) {
        FEP_TRY(alloc(count));
        if (count > 0) HIP_TRY(hipMemcpy(p, src, (size_t)count * sizeof(T), hipMemcpyHostToDevice));
        return FEP_OK;
    }
    int upload(const std::vector<T>& v) { return upload(v.data(), (int64_t)v.size()); }
    operator T*() const { return p; }
    template <class U> U* as() const { return reinterpret_cast<U*>(p); }       // the same block as double2 / float4 ...
    int64_t size() const { return n; }                  // elements allocated
};

struct Csr {
    int64_t n_rows = 0, nnz = 0;
    DeviceArray<int32_t> indptr, indices;
    DeviceArray<double> vals;
};
// one term of a sparse product on fixed patterns (product_kernel): coefficient and the index of the value it multiplies
struct Term { double coef; int32_t idx; int32_t pad; };
struct Plan {
    int64_t n_out = 0, n_terms = 0;
    DeviceArray<int32_t> tptr;
    DeviceArray<Term> terms;
};
// The transfers once more for the V-cycle, in node blocks and single precision (the refresh plans keep the double-precision
// CSR): a fine node (BF = 2 DOFs on the mesh level, 3 below) against a coarse node (3 DOFs) is one BF x 3 block — one
// column id per block instead of one per entry, 4-byte values: P_0 at 1 M DOFs 36 instead of 92 MB per pass.
struct Blocks {
    int bf = 0; int64_t nf = 0, nc = 0, nblk = 0;
    DeviceArray<int32_t> pptr, pcol; DeviceArray<float> pval;       // per fine node: (coarse node, BF x 3 values, row-major)
    DeviceArray<int32_t> rptr, rcol; DeviceArray<float> rval;       // per coarse node: (fine node, 3 x BF values) = the transposes
};
// level k (k = 0 is the mesh) -> level k+1
struct Level {
    int64_t n_fine = 0, n_coarse = 0;
    Csr P, R, A, D;                       // A, D: operator of level k+1 (A = its inverse when last) and its block-Jacobi inverse
    double omega = 0.0;                   // damping of the smoother on level k
    bool last = false;
    DeviceArray<double> x, b, r, t;       // vectors of level k+1 (t: Chebyshev smoother)
    std::vector<int32_t> hPp, hPi, hRp, hRi;                            // host patterns of the transfers (refresh plans)
    // refresh: T = A_k P (values only), A_{k+1} = R T, positions of the 3x3 diagonal blocks in A_{k+1}
    Plan ap, rt;
    DeviceArray<double> T;
    DeviceArray<float> A32;                                             // single-precision copy of A's values for node3_kernel
    DeviceArray<int32_t> d9;
    DeviceArray<int32_t> nbp, nbc;                                      // node blocks of the padded A (node3_kernel)
    double* xcur = nullptr;                                             // which of x / t / r holds the level's iterate
    Blocks tb;
};

// The multigrid part of a solver, as the set-up below sees it (fep_solver derives from it)
struct Multigrid {
    std::vector<Level> levels;
    bool refresh = false;                     // every multigrid solve re-projects the coarse operators from its tangent
    DeviceArray<double> t0, q;                // level-0 residual of the V-cycle, q = K p: allocated with the first level, kept
    // single-precision copy of the solve's K for the V-cycle's four level-0 passes (the preconditioner need not see more than
    // seven digits of the matrix; CG's own product stays in double precision).  Measured at 1 M DOFs on the LOAD STEPS of BASELINE
    // configs[3], same session, twice each: 5.93 / 5.95 s with it, 6.20 / 6.43 s without, iteration counts 10 873 / 10 910 (the
    // first comparison of the round looked at the whole wall, set-up jitter included, and saw 1 %).  On; FEP_AMG_FP32=0 turns it off.
    DeviceArray<float> k32;
    bool fp32 = true;
    bool block_transfers = true;              // Level::tb for the V-cycle's transfers (FEP_AMG_BLOCK_TRANSFERS=0: the CSR forms)
};

inline void drop_levels(Multigrid& m) {
    m.levels.clear();
    m.refresh = false;
}

inline int upload_csr(Csr& m, int64_t n_rows, int64_t n_cols, const int32_t* ip, const int32_t* ix, const double* v) {
    if (!ip || !ix || !v || ip[0] != 0) return FEP_EINVAL;
    const int64_t nnz = ip[n_rows];
    for (int64_t i = 0; i < n_rows; ++i)
        if (ip[i + 1] < ip[i]) return FEP_EINVAL;
    for (int64_t t = 0; t < nnz; ++t)
        if (ix[t] < 0 || ix[t] >= n_cols) return FEP_ERANGE;
    m.n_rows = n_rows; m.nnz = nnz;
    FEP_TRY(m.indptr.upload(ip, n_rows + 1));
    FEP_TRY(m.indices.upload(ix, nnz));
    FEP_TRY(m.vals.upload(v, nnz));
    return FEP_OK;
}

// Level::tb from the prolongation in CSR (host): the blocks of a fine node = the coarse nodes any of its BF rows reaches
// (ascending), entries a row does not hold are zero; the restriction's blocks are the transposes, fine nodes ascending.
// A level whose sizes are not whole nodes keeps the CSR form (tb.bf stays 0).
inline int build_transfer_blocks(Level& l, int bf, const int32_t* Pp, const int32_t* Pi, const double* Pv) {
    if (l.n_fine % bf || l.n_coarse % 3) return FEP_OK;
    const int64_t nf = l.n_fine / bf, nc = l.n_coarse / 3;
    // two passes over the fine nodes on the host's cores: blocks per node, then (after the running sum) their ids and values
    std::vector<int32_t> pptr((size_t)nf + 1, 0), pcol;
    std::vector<float> pval;
    std::atomic<int> bad{0};
    auto node_cols = [&](int64_t i, std::vector<int32_t>& cols) {
        cols.clear();
        for (int32_t t = Pp[bf * i]; t < Pp[bf * i + bf]; ++t) {
            if (Pi[t] < 0 || Pi[t] >= l.n_coarse) { bad = 1; return; }
            cols.push_back(Pi[t] / 3);
        }
        std::sort(cols.begin(), cols.end());
        cols.erase(std::unique(cols.begin(), cols.end()), cols.end());
    };
    fep_host::parallel_chunks(nf, [&](int64_t lo, int64_t hi, int) {
        std::vector<int32_t> cols;
        for (int64_t i = lo; i < hi && !bad; ++i) { node_cols(i, cols); pptr[(size_t)i + 1] = (int32_t)cols.size(); }
    });
    if (bad) return FEP_ERANGE;
    for (int64_t i = 0; i < nf; ++i) {
        const int64_t t = (int64_t)pptr[(size_t)i] + pptr[(size_t)i + 1];
        if (t >= INT32_MAX / 9) return FEP_ERANGE;
        pptr[(size_t)i + 1] = (int32_t)t;
    }
    pcol.resize((size_t)pptr[(size_t)nf]);
    pval.assign(pcol.size() * (size_t)(3 * bf), 0.0f);
    fep_host::parallel_chunks(nf, [&](int64_t lo, int64_t hi, int) {
        std::vector<int32_t> cols;
        for (int64_t i = lo; i < hi; ++i) {
            node_cols(i, cols);
            const size_t b0 = (size_t)pptr[(size_t)i];
            std::copy(cols.begin(), cols.end(), pcol.begin() + (std::ptrdiff_t)b0);
            for (int r = 0; r < bf; ++r)
                for (int32_t t = Pp[bf * i + r]; t < Pp[bf * i + r + 1]; ++t) {
                    const size_t b = b0 + (size_t)(std::lower_bound(cols.begin(), cols.end(), Pi[t] / 3) - cols.begin());
                    pval[b * (size_t)(3 * bf) + (size_t)(3 * r + Pi[t] % 3)] = (float)Pv[t];
                }
        }
    });
    const size_t nblk = pcol.size();
    std::vector<int32_t> rptr((size_t)nc + 1, 0), rcol(nblk), fill;
    std::vector<float> rval(nblk * (size_t)(3 * bf));
    for (size_t b = 0; b < nblk; ++b) ++rptr[(size_t)pcol[b] + 1];
    for (int64_t J = 0; J < nc; ++J) rptr[(size_t)J + 1] += rptr[(size_t)J];
    fill.assign(rptr.begin(), rptr.end() - 1);
    for (int64_t i = 0; i < nf; ++i)
        for (int32_t b = pptr[(size_t)i]; b < pptr[(size_t)i + 1]; ++b) {
            const size_t q = (size_t)fill[(size_t)pcol[(size_t)b]]++;
            rcol[q] = (int32_t)i;
            for (int r = 0; r < bf; ++r)
                for (int c = 0; c < 3; ++c) rval[q * (size_t)(3 * bf) + (size_t)(c * bf + r)] = pval[(size_t)b * (size_t)(3 * bf) + (size_t)(3 * r + c)];
        }
    Blocks B;                                            // moved into the level only when all of it is on the device
    FEP_TRY(B.pptr.upload(pptr));
    FEP_TRY(B.pcol.upload(pcol));
    FEP_TRY(B.pval.upload(pval));
    FEP_TRY(B.rptr.upload(rptr));
    FEP_TRY(B.rcol.upload(rcol));
    FEP_TRY(B.rval.upload(rval));
    B.bf = bf; B.nf = nf; B.nc = nc; B.nblk = (int64_t)nblk;
    l.tb = std::move(B);
    return FEP_OK;
}

// One more level under the hierarchy of `m` (fep_solver_amg_push_level; n_dof, n_blk: DOFs and node blocks of the mesh
// level).  The level is built aside and joins `m` only when all of it is on the device, and so do t0 / q / k32, which come
// with the first level: whatever fails, `m` is as it was before the call.
inline int push_level(Multigrid& m, int device, int64_t n_dof, int64_t n_blk, int64_t n_fine, int64_t n_coarse,
                      const int32_t* p_indptr, const int32_t* p_indices, const double* p_vals,
                      const int32_t* r_indptr, const int32_t* r_indices, const double* r_vals,
                      const int32_t* a_indptr, const int32_t* a_indices, const double* a_vals,
                      const int32_t* d_indptr, const int32_t* d_indices, const double* d_vals, double omega_fine, int last) {
    if (n_fine <= 0 || n_coarse <= 0 || !(omega_fine > 0.0)) return FEP_EINVAL;
    if (!m.levels.empty() && (m.levels.back().last || m.levels.back().n_coarse != n_fine)) return FEP_ESTATE;
    if (m.levels.empty() && n_fine != n_dof) return FEP_EINVAL;
    if (!last && !d_indptr) return FEP_EINVAL;
    FEP_TRY(fep_set_device(device));
    Level l;
    l.n_fine = n_fine; l.n_coarse = n_coarse; l.omega = omega_fine; l.last = last != 0;
    FEP_TRY(upload_csr(l.P, n_fine, n_coarse, p_indptr, p_indices, p_vals));
    l.hPp.assign(p_indptr, p_indptr + n_fine + 1); l.hPi.assign(p_indices, p_indices + p_indptr[n_fine]);
    FEP_TRY(upload_csr(l.R, n_coarse, n_fine, r_indptr, r_indices, r_vals));
    l.hRp.assign(r_indptr, r_indptr + n_coarse + 1); l.hRi.assign(r_indices, r_indices + r_indptr[n_coarse]);
    FEP_TRY(upload_csr(l.A, n_coarse, n_coarse, a_indptr, a_indices, a_vals));
    if (!last) FEP_TRY(upload_csr(l.D, n_coarse, n_coarse, d_indptr, d_indices, d_vals));
    if (m.block_transfers) FEP_TRY(build_transfer_blocks(l, m.levels.empty() ? 2 : 3, p_indptr, p_indices, p_vals));
    for (DeviceArray<double>* v : {&l.x, &l.b, &l.r, &l.t}) FEP_TRY(v->alloc(n_coarse));
    DeviceArray<double> t0, q;
    DeviceArray<float> k32;
    const bool first = !m.t0;
    if (first) {
        FEP_TRY(t0.alloc(n_dof));
        FEP_TRY(q.alloc(n_dof));
        if (m.fp32) FEP_TRY(k32.alloc(n_blk * 4));
    }
    m.levels.push_back(std::move(l));
    if (first) { m.t0 = std::move(t0); m.q = std::move(q); m.k32 = std::move(k32); }
    return FEP_OK;
}

}  // namespace fep_levels
