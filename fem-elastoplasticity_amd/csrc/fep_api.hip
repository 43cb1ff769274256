// C-ABI implementation of include/fep.h (libfep_hip.so).  Host side: context, symbolic
// phase (node graph -> CSR pattern + gather lists), launches.  Device side: fep_kernels.hip.h.
#include "fep_common.h"
#include "fep_host.h"
#include "fep_kernels.hip.h"
#include "fep_staging.h"
#include "fep_step_plan.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <thread>
#include <type_traits>
#include <vector>

using namespace fep;

// workgroup shape of the 15-node element's patch form: 16 elements on 256 threads.  The same 16 elements on 512 threads with
// two lanes per (element, node) pair in phase 2 (ElemCfg: JS = 2; 116 instead of 240 VGPRs, twice the waves per CU) measured
// 3-4 % slower in one session (0.931 against 0.899-0.900 ms, profiles/r04_ablation.md): kept in the ablation build
#ifndef FEP_P4_TPB
#define FEP_P4_TPB 256
#define FEP_P4_JS 1
#endif

thread_local int fep_g_last_hip = 0;
#define g_last_hip fep_g_last_hip

// The switches of the PRODUCT library, read at every context creation (a process may create contexts on different routes
// one after the other; the parity tests do): everything else goes through fep_tune() and exists in -DFEP_ABLATION builds
// only (fep_common.h).
//   FEP_ROUTE=coo | patch   the element route in its COO form (every K_e block through HBM, csr_reduce_kernel) / its patch
//                           form for EVERY element type, P1 included: the independent cross-checks of the parity tests
//                           (unset: P1 takes its node route, the other types the patch form)
//   FEP_VALIDATE_PLAN=1     replay the gather plan against the symbolic phase at context creation (tests)
//   FEP_VERBOSE=1           plan statistics on stderr (kept with the context for its steps)
static const char* env_now(const char* name) { const char* v = std::getenv(name); return (v && *v) ? v : nullptr; }
static bool env_is(const char* name, const char* v) { const char* r = env_now(name); return r && std::strcmp(r, v) == 0; }

// What a context runs, chosen once at creation (choose_route), and what each of its calls launches (fep_step_plan.h)
using fep_plan::Route;
using fep_plan::StageA;
using fep_plan::StageB;
using fep_plan::StepPlan;

// Persistent device buffers of a context's *_host entry points (fep_ctx::hbuf; their sizes: size_host_buffers).  One block
// per enumerator before kCtxBufCount; the names after it share the block of a call that never runs at the same time (the
// calls of one device hold its engine's lock in turn): load_volume's f_v and point_coords' result (2 n_int each) lie in the
// block of s, load_volume's result in that of F, its weights in that of the transform's input.
enum CtxBuf {
    kBufU, kBufEp, kBufE, kBufS, kBufDs, kBufIndP, kBufK, kBufF, kBufCounts, kBufQ, kBufNode, kBufField, kBufSNode, kBufEta2,
    kBufStats, kCtxBufCount, kBufFv = kBufS, kBufXq = kBufS, kBufLoad = kBufF, kBufWeight = kBufQ,
};
// Device buffers of the mesh-free return map, in its engine's store (sized by each call)
enum RmBuf { kRmE, kRmEp, kRmShear, kRmBulk, kRmM3, kRmM4, kRmS, kRmDs, kRmIndP, kRmCounts, kRmField };

// The hardening curve of the fifth model as its kernels take it (fep.h, fep_return_map_vmi_*): R[0] = 0,
// R[j + 1] = R[j] + slope[j] * (kappa[j + 1] - kappa[j]) in this order without contraction, the segments behind the last padded
// with kappa = +Inf, R = 0, slope = 0.  FEP_EINVAL, with *out untouched, unless n_seg is 1 .. FEP_MAX_HARDENING_SEGMENTS,
// kappa[0] == 0, kappa strictly increasing and finite, slope finite.
static int make_hard(int n_seg, const double* kappa_h, const double* slope_h, Hard* out) {
#pragma clang fp contract(off)
    if (n_seg < 1 || n_seg > kHardSeg || !kappa_h || !slope_h) return FEP_EINVAL;
    if (!(kappa_h[0] == 0.0)) return FEP_EINVAL;
    for (int j = 0; j < n_seg; ++j) {
        if (!std::isfinite(kappa_h[j]) || !std::isfinite(slope_h[j])) return FEP_EINVAL;
        if (j > 0 && !(kappa_h[j] > kappa_h[j - 1])) return FEP_EINVAL;
    }
    Hard h;
    for (int j = 0; j < kHardSeg; ++j) { h.kappa[j] = HUGE_VAL; h.R[j] = 0.0; h.slope[j] = 0.0; }
    for (int j = 0; j < n_seg; ++j) {
        h.kappa[j] = kappa_h[j];
        h.slope[j] = slope_h[j];
        if (j > 0) {
            const double step = slope_h[j - 1] * (kappa_h[j] - kappa_h[j - 1]);
            h.R[j] = h.R[j - 1] + step;
        }
    }
    *out = h;
    return FEP_OK;
}
static Hard flat_hard() {
    const double zero = 0.0;
    Hard h;
    (void)make_hard(1, &zero, &zero, &h);
    return h;
}

// Compile-time flavour: a branch on it folds away, and in a template the product never instantiates what lies behind it
#ifdef FEP_ABLATION
static constexpr bool kAblationBuild = true;
#else
static constexpr bool kAblationBuild = false;
#endif

// The state of each route: its plan's sizes and flags, its device tables, its per-step scratch.  A context fills the one its
// Route tag names (its setup_*), and only that route's launchers read it.  `Variant`: what only the measurement build's
// switches ever set to anything but the default here (the product runs the defaults).

// P1 node route (fep_host.h, P1Plan): node-centric gather assembly from 48-byte geometry records
struct P1NodeRoute {
    struct Variant {                                    // ablation switches: the product keeps these defaults
        int tile = 256;                                 // FEP_P1_TILE: node-pair blocks per workgroup of the assembly kernel
        bool lds = true, pk = true;                     // FEP_P1_PATH: LDS-staged form, packed descriptors (the product declines any other plan)
        bool dma = false;                               // FEP_P1_DMA=1: node data and gather codes of the one-kernel step by LDS-DMA
        bool asm_from_nodes = false;                    // FEP_P1_ASM=nodes: assembly kernel with geometry from LDS-staged nodes (measured slower)
        int fused_mode = 1;                             // FEP_P1_FUSED=off|kf|all: 0 = never, 1 = only when no point output is wanted, 2 = always
        unsigned long long* clk = nullptr;              // FEP_P1_CLK=1: 8 stamps per tile of the last p1_node_lds_kernel launch, then of the last p1_fused_kernel launch
    } v;
    int n_tiles = 0;                                    // workgroups of the tile kernels
    bool rng = false;                                   // element lists as runs (in trec) instead of wg_elist
    // one-kernel step (p1_fused_kernel): per-tile node lists / runs, per staged element its tile-local node indices + owner bit
    bool fused = false, fused_rng = false;
    int L = 0, C = 0, NL = 0;                           // staged elements / gather codes / nodes per tile (max)
    // device, static
    int32_t* trec = nullptr;                            // one record of kRecInts ints per tile (fep_host.h, P1Plan::rec)
    int32_t* wg_elist = nullptr;                        // list form (rng false); the runs of the run form ride in trec
    uint16_t* perm_l = nullptr;                         // 16-bit gather codes
    uint2* pk = nullptr;                                // packed block descriptors, lanes sorted by segment length
    int32_t* wg_nlist = nullptr;
    uint32_t* el_nodes = nullptr;
    // tables of the variants the product never runs (NULL there): the unpacked descriptors read segptr, meta and ncol, the direct
    // kernel (p1_node_kernel) these and its gather list perm2
    int32_t *segptr = nullptr, *ncol = nullptr, *perm2 = nullptr;
    uint32_t* meta = nullptr;
    // device, scratch
    double* geo = nullptr;                              // 48-byte geometry record per element (geometry_kernel)
    unsigned long long* slot_counts = nullptr;          // one-kernel step: 256 slots x 16 words, zero between steps
};

// What element_kernel takes in either form of the element route (elem_form)
struct ElemForm {
    bool geo = true;                                    // geometry from coordinates instead of the dphi arrays
    int lds_pad = 0;                                    // ablation switch FEP_ELEM_LDS_PAD: extra LDS bytes per workgroup (occupancy experiments)
};

// Patch form of the element route (fep_host.h, PatchPlan)
struct PatchRoute {
    struct Variant {                                    // ablation switches: the product keeps this default
        unsigned long long* phase_clk = nullptr;        // FEP_PHASE_CLK=1: phase stamps of the last element_kernel launch (reported at destroy)
    } v;
    int eb = 0, tpb = 256, js = 1;                      // workgroup shape (ElemCfg)
    int64_t n_patch = 0, n_open = 0, n_fopen = 0;
    // device, static
    int32_t *desc = nullptr, *plist = nullptr, *pel = nullptr, *pnodes = nullptr;
    uint2 *items = nullptr, *fitems = nullptr;
    uint16_t *codes = nullptr, *fcodes = nullptr;
    uint4 *fix = nullptr, *ffix = nullptr;
    uint2* fixT = nullptr;
    // device, scratch rewritten by every step
    double *Pc = nullptr, *Pf = nullptr;                // partial blocks / forces of the open items
};

// COO form of the element route: every K_e block through HBM
struct CooRoute {
    struct Variant {                                    // ablation switches: the product keeps this default
        int csr_gathers = 4;                            // gathers in flight per lane of csr_reduce_kernel (FEP_CSR_GATHERS=2|4|6|8;
                                                        // measured P2 / Q2 / P4 reduce kernel: 2: 0.406 / 0.376 / 0.654 ms, 4: 0.392 / 0.347 / 0.651,
                                                        // 6: 0.382 / 0.371 / 0.650, 8 (5 waves per SIMD): 0.432 / 0.425 / 0.733)
    } v;
    int n_tiles = 0;                                    // tiles of csr_reduce*_kernel
    bool kc_aos = false;                                // K_e half-blocks: all blocks of an element adjacent (AoS) or block-major (SoA)
    // device, static
    int32_t* tstart = nullptr;                          // first block of every tile
    int32_t* perm = nullptr;                            // address of every contribution in Kc
    uint2* pkc = nullptr;                               // packed block descriptors of csr_reduce_pk_kernel (NULL: fields too wide)
    int32_t* segptr = nullptr;                          // the unpacked descriptors of csr_reduce_kernel, uploaded only without pkc
    uint32_t* meta = nullptr;
    // device, scratch rewritten by every step
    double *Kc = nullptr, *fe = nullptr;
};

struct fep_ctx {
    int device = 0;
    int elem_type = 0;
    int n_p = 0, n_q = 0;
    int64_t n_e = 0, n_n = 0, n_int = 0, n_dof = 0, nnz = 0, n_blk = 0;
    Route route = Route::Coo;                           // which of the route structs below is filled
    P1NodeRoute p1;
    PatchRoute patch;
    CooRoute coo;
    ElemForm elem_form;                                 // Patch and Coo
#ifdef FEP_ABLATION
    struct GenNodeRoute* gen = nullptr;                 // (defined with its set-up and launchers)
#endif
    bool have_materials = false;
    int model = FEP_MODEL_DP;                           // fep_ctx_set_model: which return map the steps run
    Hard hard = flat_hard();                            // FEP_MODEL_VMI: fep_ctx_set_hardening (one segment of slope 0 until then)
    std::vector<void*> owned;                           // every device allocation of dmalloc / upload (freed by fep_ctx_destroy)
    MatU matu{};                                        // homogeneous-material fast path (arrays not read)
    // device, static
    int32_t* elem = nullptr;
    double *coords = nullptr, *dh1 = nullptr, *dh2 = nullptr, *wf = nullptr;
    double *dphi1 = nullptr, *dphi2 = nullptr, *weight = nullptr, *det = nullptr;
    double *shear = nullptr, *bulk = nullptr, *eta = nullptr, *c = nullptr;
    int32_t *iptr = nullptr, *ilist = nullptr;
    double* xy = nullptr;                               // interleaved (x,y) per node
    P1Tab p1tab{};
    bool has_orphans = false;                           // nodes that belong to no element (their F entries are zeroed per step)
    // device, scratch rewritten by every step
    double *s_int = nullptr, *ds_int = nullptr;     // used when the caller does not ask for s / ds
    uint2* blk_counts = nullptr;                        // per-workgroup branch counters of the stage that counts: room for the route's
    int n_count_blocks = 0;                             // stage-A grid (n_count_blocks) and for the point kernel's
    fep_stage::DeviceStore hbuf{kCtxBufCount};          // persistent device buffers of the *_host entry points, by CtxBuf
    // host copies of the pattern
    std::vector<int32_t> indptr, indices;
    // in-situ profiling: 4 events per call (fep_step_dev, fep_assemble_dev)
    bool profiling = false;
    std::vector<hipEvent_t> events;
    bool verbose = false;                               // FEP_VERBOSE at creation
};

// The size of every host staging buffer, fixed by the mesh: each block is allocated once, at this size, by the first call
// that uses it (a shared block at the size of its largest user: kBufS holds 4 n_int although assemble copies 3 n_int in)
static void size_host_buffers(fep_ctx* c) {
    const size_t d = sizeof(double), n_int = (size_t)c->n_int, n_n = (size_t)c->n_n, n_dof = (size_t)c->n_dof;
    auto size = [&](CtxBuf b, size_t bytes) { c->hbuf[b].cap = bytes; };
    size(kBufU, n_dof * d);       size(kBufEp, 4 * n_int * d);   size(kBufE, 3 * n_int * d);   size(kBufS, 4 * n_int * d);
    size(kBufDs, 9 * n_int * d);  size(kBufIndP, n_int);         size(kBufK, (size_t)c->nnz * d);  size(kBufF, n_dof * d);
    size(kBufCounts, 2 * sizeof(int64_t));                       size(kBufQ, n_int * d);       size(kBufNode, n_n * d);
    size(kBufField, 4 * n_int * d);  size(kBufSNode, 4 * n_n * d);  size(kBufEta2, (size_t)c->n_e * d);  size(kBufStats, 4 * d);
}

__attribute__((visibility("hidden"))) int fep_set_device(int dev) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) { g_last_hip = (int)e; (void)hipGetLastError(); return FEP_ENODEV; }
    if (dev < 0 || dev >= n) return FEP_ENODEV;
    e = hipSetDevice(dev);
    if (e != hipSuccess) { g_last_hip = (int)e; (void)hipGetLastError(); return FEP_ENODEV; }
    return FEP_OK;
}

// device memory of a context: recorded in c->owned, freed by fep_ctx_destroy
template <class T> static int dmalloc(fep_ctx* c, T** p, int64_t count) {
    *p = nullptr;
    if (count <= 0) count = 1;
    try { c->owned.reserve(c->owned.size() + 1); } catch (...) { return FEP_ENOMEM; }   // (recording cannot fail once the memory is held)
    HIP_TRY(hipMalloc((void**)p, (size_t)count * sizeof(T)));
    c->owned.push_back(*p);
    return FEP_OK;
}
template <class T> static int upload(fep_ctx* c, T** p, const T* src, int64_t count) {
    FEP_TRY(dmalloc(c, p, count));
    if (count > 0) HIP_TRY(hipMemcpy(*p, src, (size_t)count * sizeof(T), hipMemcpyHostToDevice));
    return FEP_OK;
}

static inline unsigned grid_for(int64_t n, int per_block) { return (unsigned)((n + per_block - 1) / per_block); }

// Compile-time dispatch: every generic lambda below receives its template arguments as std::integral_constant /
// std::bool_constant values (C++17 has no template lambdas)
template <int T, int NP_, int NQ_> struct ElemT { static constexpr int type = T, NP = NP_, NQ = NQ_; };
template <int V> using int_c = std::integral_constant<int, V>;

// f(ElemT<type, NP, NQ>) for the element type `elem_type`; FEP_EINVAL for an unknown type
template <class F> static int with_type(int elem_type, F&& f) {
    switch (elem_type) {
        case FEP_P1: return f(ElemT<FEP_P1, 3, 1>{});
        case FEP_P2: return f(ElemT<FEP_P2, 6, 7>{});
        case FEP_Q1: return f(ElemT<FEP_Q1, 4, 4>{});
        case FEP_Q2: return f(ElemT<FEP_Q2, 8, 9>{});
        case FEP_P4: return f(ElemT<FEP_P4, 15, 12>{});
        default: return FEP_EINVAL;
    }
}
// f(int_c<FEP_MODEL_*>) for the material model `model`; FEP_EINVAL for an id that is none (4 is unassigned)
template <class F> static int with_model(int model, F&& f) {
    switch (model) {
        case FEP_MODEL_DP: return f(int_c<FEP_MODEL_DP>{});
        case FEP_MODEL_VM: return f(int_c<FEP_MODEL_VM>{});
        case FEP_MODEL_MC: return f(int_c<FEP_MODEL_MC>{});
        case FEP_MODEL_VMPS: return f(int_c<FEP_MODEL_VMPS>{});
        case FEP_MODEL_VMI: return f(int_c<FEP_MODEL_VMI>{});
        default: return FEP_EINVAL;
    }
}
template <class F> static int with_bool(bool v, F&& f) { return v ? f(std::true_type{}) : f(std::false_type{}); }
// A switch that only the ablation build varies: the product instantiates the value `Product` alone and refuses the other
// one (FEP_ESTATE: a context the product never creates)
template <bool Product, class F> static int with_ablation_bool(bool v, F&& f) {
    if constexpr (kAblationBuild) return with_bool(v, f);
    else return v == Product ? f(std::bool_constant<Product>{}) : FEP_ESTATE;
}

// Launches `kernel` with `lds` bytes of dynamic LDS, raising its limit first when `lds` is above `limit`
template <class... P, class... A>
static int launch_lds(void (*kernel)(P...), unsigned grid, unsigned tpb, size_t lds, size_t limit, hipStream_t st, A... args) {
    if (lds > limit) HIP_TRY(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(tpb), lds, st, args...);
    HIP_TRY(hipGetLastError());
    return FEP_OK;
}

// ---------------------------------------------------------------------------------------
extern "C" int fep_version(void) { return 1; }
extern "C" int fep_build_is_ablation(void) { return kAblationBuild ? 1 : 0; }

extern "C" const char* fep_strerror(int code) {
    switch (code) {
        case FEP_OK: return "ok";
        case FEP_EINVAL: return "invalid argument";
        case FEP_ENODEV: return "no usable HIP device";
        case FEP_ENOMEM: return "out of memory";
        case FEP_EHIP: return "HIP runtime error";
        case FEP_ERANGE: return "index out of range";
        case FEP_ESTATE: return "call order violated";
        default: return "unknown error";
    }
}
extern "C" int fep_last_hip_error(void) { return g_last_hip; }

extern "C" int fep_device_count(int* n_out) {
    if (!n_out) return FEP_EINVAL;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { g_last_hip = (int)e; (void)hipGetLastError(); *n_out = 0; return FEP_ENODEV; }
    *n_out = n;
    return FEP_OK;
}

extern "C" int fep_element_shape(int elem_type, int* n_p, int* n_q) {
    return with_type(elem_type, [&](auto et) {
        if (n_p) *n_p = decltype(et)::NP;
        if (n_q) *n_q = decltype(et)::NQ;
        return FEP_OK;
    });
}

extern "C" int fep_malloc(int device_id, void** ptr_d, int64_t bytes) {
    if (!ptr_d || bytes < 0) return FEP_EINVAL;
    FEP_TRY(fep_set_device(device_id));
    HIP_TRY(hipMalloc(ptr_d, (size_t)(bytes > 0 ? bytes : 1)));
    return FEP_OK;
}
extern "C" int fep_free(int device_id, void* ptr_d) {
    if (!ptr_d) return FEP_OK;
    FEP_TRY(fep_set_device(device_id));
    HIP_TRY(hipFree(ptr_d));
    return FEP_OK;
}
extern "C" int fep_memcpy_h2d(int device_id, void* dst_d, const void* src_h, int64_t bytes) {
    if (bytes < 0 || (bytes > 0 && (!dst_d || !src_h))) return FEP_EINVAL;
    FEP_TRY(fep_set_device(device_id));
    if (bytes) HIP_TRY(hipMemcpy(dst_d, src_h, (size_t)bytes, hipMemcpyHostToDevice));
    return FEP_OK;
}
extern "C" int fep_memcpy_d2h(int device_id, void* dst_h, const void* src_d, int64_t bytes) {
    if (bytes < 0 || (bytes > 0 && (!dst_h || !src_d))) return FEP_EINVAL;
    FEP_TRY(fep_set_device(device_id));
    if (bytes) HIP_TRY(hipMemcpy(dst_h, src_d, (size_t)bytes, hipMemcpyDeviceToHost));
    return FEP_OK;
}
extern "C" int fep_sync(int device_id, void* stream) {
    FEP_TRY(fep_set_device(device_id));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return FEP_OK;
}

// ---------------------------------------------------------------------------------------
// a2 mesh-free
// ---------------------------------------------------------------------------------------
static E0 make_e0(const double* e0_h) {
    E0 z;
    for (int i = 0; i < 4; ++i) z.v[i] = e0_h ? e0_h[i] : 0.0;
    return z;
}

// The material models.  ModelKernels<FEP_MODEL_*> is the only place that names a model's kernels: the tag the model puts into
// their names, whether they take its hardening curve (Hard, by value, as their last argument), and its kernel of each
// point-kernel family -- mesh-free, P1, general <NP, NQ> -- plain (FIELD false) and with an initial-strain field (fep_*_field_*).
// nullptr: the model has no such kernel and its launcher refuses the call.  Drucker-Prager's plain general step is the fused
// element route, and the mesh-free field pair fep_return_map_field_* keeps its three models (include/fep.h).
template <bool FIELD, class P, class F> static constexpr auto pick(P plain, F with_field) {
    if constexpr (FIELD) return with_field; else return plain;
}
template <class K> constexpr bool no_kernel = std::is_null_pointer_v<K>;
template <int MODEL> struct ModelKernels;
template <> struct ModelKernels<FEP_MODEL_DP> {
    static constexpr const char* tag = "";
    static constexpr bool has_hard = false;
    template <bool FIELD> static constexpr auto return_map = pick<FIELD>(return_map_kernel, return_map_field_kernel<FEP_MODEL_DP>);
    template <bool FIELD> static constexpr auto p1_point = pick<FIELD>(p1_point_kernel, p1_point_field_kernel<FEP_MODEL_DP>);
    template <bool FIELD, int NP, int NQ>
    static constexpr auto point = pick<FIELD>(nullptr, point_field_kernel<FEP_MODEL_DP, NP, NQ>);
};
template <> struct ModelKernels<FEP_MODEL_VM> {
    static constexpr const char* tag = "vm_";
    static constexpr bool has_hard = false;
    template <bool FIELD> static constexpr auto return_map = pick<FIELD>(return_map_vm_kernel, return_map_field_kernel<FEP_MODEL_VM>);
    template <bool FIELD> static constexpr auto p1_point = pick<FIELD>(p1_point_vm_kernel, p1_point_field_kernel<FEP_MODEL_VM>);
    template <bool FIELD, int NP, int NQ>
    static constexpr auto point = pick<FIELD>(point_vm_kernel<NP, NQ>, point_field_kernel<FEP_MODEL_VM, NP, NQ>);
};
template <> struct ModelKernels<FEP_MODEL_MC> {
    static constexpr const char* tag = "mc_";
    static constexpr bool has_hard = false;
    template <bool FIELD> static constexpr auto return_map = pick<FIELD>(return_map_mc_kernel, return_map_field_kernel<FEP_MODEL_MC>);
    template <bool FIELD> static constexpr auto p1_point = pick<FIELD>(p1_point_mc_kernel, p1_point_field_kernel<FEP_MODEL_MC>);
    template <bool FIELD, int NP, int NQ>
    static constexpr auto point = pick<FIELD>(point_mc_kernel<NP, NQ>, point_field_kernel<FEP_MODEL_MC, NP, NQ>);
};
template <> struct ModelKernels<FEP_MODEL_VMPS> {
    static constexpr const char* tag = "vmps_";
    static constexpr bool has_hard = false;
    template <bool FIELD> static constexpr auto return_map = pick<FIELD>(return_map_vmps_kernel, nullptr);
    template <bool FIELD> static constexpr auto p1_point = pick<FIELD>(p1_point_vmps_kernel, p1_point_field_kernel<FEP_MODEL_VMPS>);
    template <bool FIELD, int NP, int NQ>
    static constexpr auto point = pick<FIELD>(point_vmps_kernel<NP, NQ>, point_field_kernel<FEP_MODEL_VMPS, NP, NQ>);
};
template <> struct ModelKernels<FEP_MODEL_VMI> {
    static constexpr const char* tag = "vmi_";
    static constexpr bool has_hard = true;
    template <bool FIELD> static constexpr auto return_map = pick<FIELD>(return_map_vmi_kernel, nullptr);
    template <bool FIELD> static constexpr auto p1_point = pick<FIELD>(p1_point_vmi_kernel, p1_point_vmi_field_kernel);
    template <bool FIELD, int NP, int NQ>
    static constexpr auto point = pick<FIELD>(point_vmi_kernel<NP, NQ>, point_vmi_field_kernel<NP, NQ>);
};

// What a point kernel takes behind blk_counts: the initial-strain field and its scale (a *_field_kernel), then the hardening
// curve (a model with has_hard)
struct PointExtras { const double* field; double scale; const Hard* hard; };
// The one launch of the three families: `kernel` of ModelKernels MK on kBlock threads with `args` and what `x` adds for it.
// FEP_EINVAL: the model has no such kernel, or takes a curve and none came
template <class MK, bool FIELD, class K, class... A>
static int launch_point_kernel(K kernel, unsigned grid, hipStream_t st, const PointExtras& x, A... args) {
    if constexpr (no_kernel<K>) return FEP_EINVAL;
    else {
        if (MK::has_hard && !x.hard) return FEP_EINVAL;
        auto launch = [&](auto... extra) { hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), 0, st, args..., extra...); };
        auto with_hard = [&](auto... extra) { if constexpr (MK::has_hard) launch(extra..., *x.hard); else launch(extra...); };
        if constexpr (FIELD) with_hard(x.field, x.scale); else with_hard();
        HIP_TRY(hipGetLastError());
        return FEP_OK;
    }
}
// whether the mesh-free field pair takes `model`
static bool has_return_map_field(int model) {
    return with_model(model, [](auto m) {
        return no_kernel<decltype(ModelKernels<decltype(m)::value>::template return_map<true>)> ? FEP_EINVAL : FEP_OK;
    }) == FEP_OK;
}

// (`model`: the third and fourth parameter arrays are eta, c of Drucker-Prager, a, Y of von Mises in plane strain or plane stress,
// or sin_phi, c of Mohr-Coulomb)
static int return_map_dev_impl(int model, int device_id, void* stream, int64_t n_int,
                               const double* e_d, int64_t e_pt_stride, int64_t e_comp_stride,
                               const double* e0_h, double* ep_prev_d,
                               const double* shear_d, const double* bulk_d, const double* eta_d, const double* c_d,
                               int accept, double* s_d, double* ds_d, uint8_t* ind_p_d, int64_t* counts_d, const PointExtras& x) {
    if (n_int < 0) return FEP_EINVAL;
    if (n_int > 0 && (!e_d || !shear_d || !bulk_d || !eta_d || !c_d)) return FEP_EINVAL;
    FEP_TRY(fep_set_device(device_id));
    hipStream_t st = (hipStream_t)stream;
    if (n_int == 0) { if (counts_d) HIP_TRY(hipMemsetAsync(counts_d, 0, 2 * sizeof(int64_t), st)); return FEP_OK; }
    const unsigned n_blocks = grid_for(n_int, kBlock);
    // Per-workgroup branch counters (summed by counts_reduce_kernel): the grow-only scratch of (device, stream).  The kernel used
    // to add its two counters to the caller's counts with global atomics — one contended pair per workgroup, the pattern that
    // cost the P1 kernels 70 us per launch in round 1.
    uint2* blk = nullptr;
    if (counts_d)
        FEP_TRY(stream_scratch(kScratchRmCounts, device_id, st, n_blocks * sizeof(uint2),
                               ((size_t)n_blocks + n_blocks / 4 + 64) * sizeof(uint2), (void**)&blk));
    FEP_TRY(with_model(model, [&](auto m) {
        using MK = ModelKernels<decltype(m)::value>;
        return with_bool(x.field != nullptr, [&](auto fld) {
            constexpr bool FIELD = decltype(fld)::value;
            return launch_point_kernel<MK, FIELD>(MK::template return_map<FIELD>, n_blocks, st, x, n_int, e_d, e_pt_stride,
                                                  e_comp_stride, make_e0(e0_h), ep_prev_d, shear_d, bulk_d, eta_d, c_d, accept, s_d,
                                                  ds_d, ind_p_d, blk);
        });
    }));
    if (counts_d) {
        hipLaunchKernelGGL(counts_reduce_kernel, dim3(1), dim3(1024), 0, st, (int)n_blocks, blk, (unsigned long long*)counts_d);
        HIP_TRY(hipGetLastError());
    }
    return FEP_OK;
}

extern "C" int fep_return_map_dev(int device_id, void* stream, int64_t n_int,
                                  const double* e_d, int64_t e_pt_stride, int64_t e_comp_stride,
                                  const double* e0_h, double* ep_prev_d,
                                  const double* shear_d, const double* bulk_d, const double* eta_d, const double* c_d,
                                  int accept, double* s_d, double* ds_d, uint8_t* ind_p_d, int64_t* counts_d) {
    return return_map_dev_impl(FEP_MODEL_DP, device_id, stream, n_int, e_d, e_pt_stride, e_comp_stride, e0_h, ep_prev_d,
                               shear_d, bulk_d, eta_d, c_d, accept, s_d, ds_d, ind_p_d, counts_d, PointExtras{});
}

extern "C" int fep_return_map_vm_dev(int device_id, void* stream, int64_t n_int,
                                     const double* e_d, int64_t e_pt_stride, int64_t e_comp_stride,
                                     const double* e0_h, double* ep_prev_d,
                                     const double* shear_d, const double* bulk_d, const double* a_d, const double* y_d,
                                     int accept, double* s_d, double* ds_d, uint8_t* ind_p_d, int64_t* counts_d) {
    return return_map_dev_impl(FEP_MODEL_VM, device_id, stream, n_int, e_d, e_pt_stride, e_comp_stride, e0_h, ep_prev_d,
                               shear_d, bulk_d, a_d, y_d, accept, s_d, ds_d, ind_p_d, counts_d, PointExtras{});
}

extern "C" int fep_return_map_mc_dev(int device_id, void* stream, int64_t n_int,
                                     const double* e_d, int64_t e_pt_stride, int64_t e_comp_stride,
                                     const double* e0_h, double* ep_prev_d,
                                     const double* shear_d, const double* bulk_d, const double* sin_phi_d, const double* c_d,
                                     int accept, double* s_d, double* ds_d, uint8_t* ind_p_d, int64_t* counts_d) {
    return return_map_dev_impl(FEP_MODEL_MC, device_id, stream, n_int, e_d, e_pt_stride, e_comp_stride, e0_h, ep_prev_d,
                               shear_d, bulk_d, sin_phi_d, c_d, accept, s_d, ds_d, ind_p_d, counts_d, PointExtras{});
}

extern "C" int fep_return_map_vmps_dev(int device_id, void* stream, int64_t n_int,
                                       const double* e_d, int64_t e_pt_stride, int64_t e_comp_stride,
                                       const double* e0_h, double* ep_prev_d,
                                       const double* shear_d, const double* bulk_d, const double* a_d, const double* y_d,
                                       int accept, double* s_d, double* ds_d, uint8_t* ind_p_d, int64_t* counts_d) {
    return return_map_dev_impl(FEP_MODEL_VMPS, device_id, stream, n_int, e_d, e_pt_stride, e_comp_stride, e0_h, ep_prev_d,
                               shear_d, bulk_d, a_d, y_d, accept, s_d, ds_d, ind_p_d, counts_d, PointExtras{});
}

extern "C" int fep_return_map_vmi_dev(int device_id, void* stream, int64_t n_int,
                                      const double* e_d, int64_t e_pt_stride, int64_t e_comp_stride,
                                      const double* e0_h, double* ep_prev_d,
                                      const double* shear_d, const double* bulk_d, const double* a_d, const double* y_d,
                                      int n_seg, const double* kappa_h, const double* slope_h,
                                      int accept, double* s_d, double* ds_d, uint8_t* ind_p_d, int64_t* counts_d) {
    Hard hard;
    FEP_TRY(make_hard(n_seg, kappa_h, slope_h, &hard));
    return return_map_dev_impl(FEP_MODEL_VMI, device_id, stream, n_int, e_d, e_pt_stride, e_comp_stride, e0_h, ep_prev_d,
                               shear_d, bulk_d, a_d, y_d, accept, s_d, ds_d, ind_p_d, counts_d, PointExtras{nullptr, 0.0, &hard});
}

extern "C" int fep_return_map_field_dev(int model, int device_id, void* stream, int64_t n_int,
                                        const double* e_d, int64_t e_pt_stride, int64_t e_comp_stride,
                                        const double* e0_h, const double* e0_field_d, double e0_scale, double* ep_prev_d,
                                        const double* shear_d, const double* bulk_d, const double* m3_d, const double* m4_d,
                                        int accept, double* s_d, double* ds_d, uint8_t* ind_p_d, int64_t* counts_d) {
    if (!has_return_map_field(model) || !e0_field_d) return FEP_EINVAL;
    return return_map_dev_impl(model, device_id, stream, n_int, e_d, e_pt_stride, e_comp_stride, e0_h, ep_prev_d,
                               shear_d, bulk_d, m3_d, m4_d, accept, s_d, ds_d, ind_p_d, counts_d,
                               PointExtras{e0_field_d, e0_scale, nullptr});
}

extern "C" int fep_host_alloc(void** ptr_h, int64_t bytes) {
    if (!ptr_h || bytes < 0) return FEP_EINVAL;
    *ptr_h = nullptr;
    try { return fep_stage::pinned().alloc(ptr_h, (size_t)bytes); }
    catch (...) { return FEP_ENOMEM; }
}
extern "C" int fep_host_free(void* ptr_h) {
    try { return fep_stage::pinned().release(ptr_h); }
    catch (...) { return FEP_ENOMEM; }
}
extern "C" int fep_host_trim(void) {
    try { return fep_stage::pinned().trim(); }
    catch (...) { return FEP_ENOMEM; }
}

static int return_map_host_impl(int model, int device_id, int64_t n_int,
                                const double* e_h, int64_t e_pt_stride, int64_t e_comp_stride,
                                const double* e0_h, double* ep_prev_h,
                                const double* shear_h, const double* bulk_h, const double* eta_h, const double* c_h,
                                int accept, double* s_h, double* ds_h, uint8_t* ind_p_h, int64_t* counts_h,
                                const PointExtras& x) {            // (x.field: host memory, 4 n_int values)
    if (n_int < 0) return FEP_EINVAL;
    if (n_int > 0 && (!e_h || !shear_h || !bulk_h || !eta_h || !c_h)) return FEP_EINVAL;
    if (counts_h) { counts_h[0] = 0; counts_h[1] = 0; }
    if (n_int == 0) return FEP_OK;
    fep_stage::HostCall call(device_id);
    FEP_TRY(call.status());
    // the strain is copied as the dense block that contains the strided view
    const int64_t span = (n_int - 1) * e_pt_stride + 2 * e_comp_stride + 1;
    if (e_pt_stride <= 0 || e_comp_stride <= 0 || span < 3 * n_int) return FEP_EINVAL;
    const size_t n = (size_t)n_int;
    static const bool timing = fep_tune("FEP_TIME_HOST") != nullptr;
    auto ms = [t0 = std::chrono::steady_clock::now()] {
        return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    };
    const double* e = call.in(kRmE, e_h, (size_t)span);
    double* ep = call.inout(kRmEp, ep_prev_h, 4 * n, accept != 0);
    const double *sh = call.in(kRmShear, shear_h, n), *bu = call.in(kRmBulk, bulk_h, n);
    const double *m3 = call.in(kRmM3, eta_h, n), *m4 = call.in(kRmM4, c_h, n), *fld = call.in(kRmField, x.field, 4 * n);
    if (timing) {
        (void)hipStreamSynchronize(call.stream());
        std::fprintf(stderr, "[fep] return_map_host: inputs on the device after %.3f ms\n", ms());
    }
    double *s = call.out(kRmS, s_h, 4 * n), *ds = call.out(kRmDs, ds_h, 9 * n);
    uint8_t* ip = call.out(kRmIndP, ind_p_h, n);
    int64_t* cnt = call.scratch<int64_t>(kRmCounts, 2);     // the kernels always count; copied back only if asked for
    call.out(kRmCounts, counts_h, 2);
    const int rf = call.run([&] {
        return return_map_dev_impl(model, device_id, call.stream(), n_int, e, e_pt_stride, e_comp_stride, e0_h, ep, sh, bu, m3, m4,
                                   accept, s, ds, ip, cnt, PointExtras{fld, x.scale, x.hard});
    });
    if (timing) std::fprintf(stderr, "[fep] return_map_host: done after %.3f ms\n", ms());
    return rf;
}

extern "C" int fep_return_map_host(int device_id, int64_t n_int,
                                   const double* e_h, int64_t e_pt_stride, int64_t e_comp_stride,
                                   const double* e0_h, double* ep_prev_h,
                                   const double* shear_h, const double* bulk_h, const double* eta_h, const double* c_h,
                                   int accept, double* s_h, double* ds_h, uint8_t* ind_p_h, int64_t* counts_h) {
    FEP_GUARD(return_map_host_impl(FEP_MODEL_DP, device_id, n_int, e_h, e_pt_stride, e_comp_stride, e0_h, ep_prev_h, shear_h,
                                   bulk_h, eta_h, c_h, accept, s_h, ds_h, ind_p_h, counts_h, PointExtras{}))
}

extern "C" int fep_return_map_vm_host(int device_id, int64_t n_int,
                                      const double* e_h, int64_t e_pt_stride, int64_t e_comp_stride,
                                      const double* e0_h, double* ep_prev_h,
                                      const double* shear_h, const double* bulk_h, const double* a_h, const double* y_h,
                                      int accept, double* s_h, double* ds_h, uint8_t* ind_p_h, int64_t* counts_h) {
    FEP_GUARD(return_map_host_impl(FEP_MODEL_VM, device_id, n_int, e_h, e_pt_stride, e_comp_stride, e0_h, ep_prev_h, shear_h,
                                   bulk_h, a_h, y_h, accept, s_h, ds_h, ind_p_h, counts_h, PointExtras{}))
}

extern "C" int fep_return_map_mc_host(int device_id, int64_t n_int,
                                      const double* e_h, int64_t e_pt_stride, int64_t e_comp_stride,
                                      const double* e0_h, double* ep_prev_h,
                                      const double* shear_h, const double* bulk_h, const double* sin_phi_h, const double* c_h,
                                      int accept, double* s_h, double* ds_h, uint8_t* ind_p_h, int64_t* counts_h) {
    FEP_GUARD(return_map_host_impl(FEP_MODEL_MC, device_id, n_int, e_h, e_pt_stride, e_comp_stride, e0_h, ep_prev_h, shear_h,
                                   bulk_h, sin_phi_h, c_h, accept, s_h, ds_h, ind_p_h, counts_h, PointExtras{}))
}

extern "C" int fep_return_map_vmps_host(int device_id, int64_t n_int,
                                        const double* e_h, int64_t e_pt_stride, int64_t e_comp_stride,
                                        const double* e0_h, double* ep_prev_h,
                                        const double* shear_h, const double* bulk_h, const double* a_h, const double* y_h,
                                        int accept, double* s_h, double* ds_h, uint8_t* ind_p_h, int64_t* counts_h) {
    FEP_GUARD(return_map_host_impl(FEP_MODEL_VMPS, device_id, n_int, e_h, e_pt_stride, e_comp_stride, e0_h, ep_prev_h, shear_h,
                                   bulk_h, a_h, y_h, accept, s_h, ds_h, ind_p_h, counts_h, PointExtras{}))
}

extern "C" int fep_return_map_vmi_host(int device_id, int64_t n_int,
                                       const double* e_h, int64_t e_pt_stride, int64_t e_comp_stride,
                                       const double* e0_h, double* ep_prev_h,
                                       const double* shear_h, const double* bulk_h, const double* a_h, const double* y_h,
                                       int n_seg, const double* kappa_h, const double* slope_h,
                                       int accept, double* s_h, double* ds_h, uint8_t* ind_p_h, int64_t* counts_h) {
    Hard hard;
    FEP_TRY(make_hard(n_seg, kappa_h, slope_h, &hard));
    FEP_GUARD(return_map_host_impl(FEP_MODEL_VMI, device_id, n_int, e_h, e_pt_stride, e_comp_stride, e0_h, ep_prev_h, shear_h,
                                   bulk_h, a_h, y_h, accept, s_h, ds_h, ind_p_h, counts_h, PointExtras{nullptr, 0.0, &hard}))
}

extern "C" int fep_return_map_field_host(int model, int device_id, int64_t n_int,
                                         const double* e_h, int64_t e_pt_stride, int64_t e_comp_stride,
                                         const double* e0_h, const double* e0_field_h, double e0_scale, double* ep_prev_h,
                                         const double* shear_h, const double* bulk_h, const double* m3_h, const double* m4_h,
                                         int accept, double* s_h, double* ds_h, uint8_t* ind_p_h, int64_t* counts_h) {
    if (!has_return_map_field(model) || !e0_field_h) return FEP_EINVAL;
    FEP_GUARD(return_map_host_impl(model, device_id, n_int, e_h, e_pt_stride, e_comp_stride, e0_h, ep_prev_h, shear_h,
                                   bulk_h, m3_h, m4_h, accept, s_h, ds_h, ind_p_h, counts_h,
                                   PointExtras{e0_field_h, e0_scale, nullptr}))
}

using fep_host::Symbolic;
using fep_host::build_symbolic;

// `p1_geo`: the node route's record array when that is the route (NULL: no records are written)
static int launch_geometry(fep_ctx* c, double* p1_geo) {
    return with_type(c->elem_type, [&](auto et) {
        using ET = decltype(et);
        hipLaunchKernelGGL((geometry_kernel<ET::NP, ET::NQ>), dim3(grid_for(c->n_int, kBlock)), dim3(kBlock), 0, nullptr,
                           c->n_e, c->n_n, c->elem, c->coords, c->dh1, c->dh2, c->wf, c->dphi1, c->dphi2, c->weight, c->det,
                           p1_geo);
        HIP_TRY(hipGetLastError());
        return FEP_OK;
    });
}

// The element kernel's per-type choices (measured; the notes are at their use in elem_form / setup_patch)
static constexpr bool elem_geo_default(int elem_type, bool patch_form) {
    return elem_type == FEP_Q1 || elem_type == FEP_Q2 || ((elem_type == FEP_P2 || elem_type == FEP_P4) && patch_form);
}

// Every instantiated shape of element_kernel: f(ElemT, PATCH, GEO, TPB, JS) with compile-time arguments, or FEP_ESTATE for
// a shape without an instantiation.  The COO form runs kBlock threads, the patch form kBlock and, for P2, 512.  The
// product instantiates one geometry form per element type and form (elem_geo_default); the ablation build both, and
// three more patch shapes (Q2 384 / 2 and 512 / 1, P4 512 / 2).
template <class F> static int elem_shape(int elem_type, bool patch_form, bool geo, int tpb, int js, F&& f) {
    return with_type(elem_type, [&](auto et) {
        using ET = decltype(et);
        return with_bool(patch_form, [&](auto pf) {
            constexpr bool PATCH = decltype(pf)::value;
            auto shape = [&](auto tpb_c, auto js_c) {
                constexpr bool G = elem_geo_default(ET::type, PATCH);
                if constexpr (kAblationBuild) return with_bool(geo, [&](auto g) { return f(et, pf, g, tpb_c, js_c); });
                else return geo == G ? f(et, pf, std::bool_constant<G>{}, tpb_c, js_c) : FEP_ESTATE;
            };
            if (tpb == kBlock && js == 1) return shape(int_c<kBlock>{}, int_c<1>{});
            if constexpr (PATCH && ET::type == FEP_P2) { if (tpb == 512 && js == 1) return shape(int_c<512>{}, int_c<1>{}); }
#ifdef FEP_ABLATION
            if constexpr (PATCH && ET::type == FEP_Q2) {
                if (tpb == 384 && js == 2) return shape(int_c<384>{}, int_c<2>{});
                if (tpb == 512 && js == 1) return shape(int_c<512>{}, int_c<1>{});
            }
            if constexpr (PATCH && ET::type == FEP_P4) { if (tpb == 512 && js == 2) return shape(int_c<512>{}, int_c<2>{}); }
#endif
            return FEP_ESTATE;
        });
    });
}

static int elements_per_workgroup(const fep_ctx* c, bool patch_form, int tpb, int js, int* eb) {
    return elem_shape(c->elem_type, patch_form, c->elem_form.geo, tpb, js, [&](auto et, auto, auto geo, auto tpb_c, auto js_c) {
        using ET = decltype(et);
        *eb = ElemCfg<ET::NP, ET::NQ, decltype(geo)::value, decltype(tpb_c)::value, decltype(js_c)::value>::EB;
        return FEP_OK;
    });
}

// What the route set-ups read of fep_ctx_create's inputs
struct MeshIn {
    const Symbolic& S;
    const int32_t* elem;
    const double *coords, *dh1, *dh2, *wf;
    bool validate;                                      // FEP_VALIDATE_PLAN: replay every plan against the symbolic phase
};

#ifdef FEP_ABLATION
// The measurement build's general node route, whole: its state, its set-up, its two launchers.
// FEP_GEN_PATH=node: node route for P2 / Q1 / Q2 (point_kernel + node_lds_kernel; measured on MI355X, 1 M elements:
// Q1 0.276 vs 0.286 ms, P2 1.80 vs 1.30 ms, Q2 0.41 vs 0.34 ms per step — its LDS gather costs n_q times the P1 one).
struct GenNodeRoute {
    int tile = 256;                                     // node-pair blocks per workgroup of node_lds_kernel
    size_t lds = 0;
    int L = 0, C = 0;                                   // staged elements / gather codes per workgroup (max)
    int32_t *segptr = nullptr, *ncol = nullptr, *wg_elist = nullptr;
    uint32_t* meta = nullptr;
    uint16_t* perm_l = nullptr;
};
static constexpr size_t kLdsNodeLds = 48 * 1024;        // (node_lds_kernel raises its dynamic LDS limit from 48 KiB on)

// *taken = false: no plan fits, the element route.
static int setup_gen_node(fep_ctx* c, const MeshIn& in, bool* taken) {
    fep_host::GnPlan G;
    fep_host::build_gn_plan(in.S, c->n_p, c->n_q, c->n_e, G);
    *taken = G.ok;
    if (!G.ok) return FEP_OK;
    c->gen = new (std::nothrow) GenNodeRoute();         // (freed by fep_ctx_destroy)
    if (!c->gen) return FEP_ENOMEM;
    GenNodeRoute& r = *c->gen;
    r.tile = G.tile; r.L = G.L; r.C = G.C; r.lds = G.lds;
    FEP_TRY(upload(c, &r.wg_elist, G.elist_pad.data(), (int64_t)G.elist_pad.size()));
    FEP_TRY(upload(c, &r.perm_l, G.codes_pad.data(), (int64_t)G.codes_pad.size()));
    FEP_TRY(upload(c, &r.ncol, in.S.ncol.data(), (int64_t)in.S.ncol.size()));
    FEP_TRY(upload(c, &r.segptr, in.S.segptr.data(), (int64_t)in.S.segptr.size()));
    FEP_TRY(upload(c, &r.meta, in.S.meta.data(), (int64_t)in.S.meta.size()));
    c->n_count_blocks = (int)grid_for(c->n_int, kBlock);
    return FEP_OK;
}

// GenNode route, stage A: point_kernel
static int launch_point(fep_ctx* c, hipStream_t st, const double* u, E0 e0, double* ep, int accept, double* eout,
                        double* s, double* ds, uint8_t* indp, uint2* blk) {
    FEP_TRY(with_type(c->elem_type, [&](auto et) {
        using ET = decltype(et);
        if constexpr (ET::type == FEP_P1 || ET::type == FEP_P4) return FEP_EINVAL;
        else {
            hipLaunchKernelGGL((point_kernel<ET::NP, ET::NQ>), dim3(grid_for(c->n_int, kBlock)), dim3(kBlock), 0, st, c->n_e,
                               c->elem, c->xy, c->dh1, c->dh2, c->wf, u, e0, ep, c->shear, c->bulk, c->eta, c->c, c->matu,
                               accept, eout, s, ds, indp, blk);
            return FEP_OK;
        }
    }));
    HIP_TRY(hipGetLastError());
    return FEP_OK;
}

// GenNode route, stage B: node_lds_kernel
static int launch_gn_node(fep_ctx* c, const GenNodeRoute& r, hipStream_t st, const double* ds, const double* s, double* k_data,
                          double* f_out, int n_counts, unsigned long long* counts_d) {
    const int n_wg = (int)grid_for(c->n_blk, r.tile);
    const unsigned grid = xcd_grid(n_wg);
    FEP_TRY(with_type(c->elem_type, [&](auto et) {
        using ET = decltype(et);
        if constexpr (ET::type == FEP_P1 || ET::type == FEP_P4) return FEP_EINVAL;
        else return with_bool(r.tile == 256, [&](auto t256) {
            constexpr int TPB = decltype(t256)::value ? 256 : 128;
            return launch_lds(node_lds_kernel<ET::NP, ET::NQ, TPB>, grid, TPB, r.lds, kLdsNodeLds, st, c->n_blk, c->n_e,
                              r.L, r.C, r.segptr, r.perm_l, r.meta, r.ncol, r.wg_elist, c->elem, c->xy,
                              c->dh1, c->dh2, c->wf, k_data ? ds : nullptr, f_out ? s : nullptr, k_data, f_out, n_wg,
                              n_counts, c->blk_counts, counts_d);
        });
    }));
    return FEP_OK;
}
template <class N> static void name_point(const fep_ctx* c, N& o) { o.add("point_kernel<%d, %d>", c->n_p, c->n_q); }
template <class N> static void name_gn_node(const fep_ctx* c, const GenNodeRoute& r, N& o) {
    o.add("node_lds_kernel<%d, %d, %d>", c->n_p, c->n_q, r.tile == 256 ? 256 : 128);
}
#endif  // FEP_ABLATION

extern "C" int fep_ctx_destroy(fep_ctx* c) {
    if (!c) return FEP_OK;
    if (fep_set_device(c->device) == FEP_OK) {
#ifdef FEP_ABLATION
        const int64_t n_patch = c->patch.n_patch;
        if (c->patch.v.phase_clk && n_patch > 0) {            // mean shader clocks per phase of the LAST element_kernel launch
            std::vector<unsigned long long> h((size_t)(12 * n_patch));
            if (hipDeviceSynchronize() == hipSuccess &&
                hipMemcpy(h.data(), c->patch.v.phase_clk, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost) == hipSuccess) {
                double acc[6] = {0, 0, 0, 0, 0, 0}, cyc = 0.0, real = 0.0, st_ids = 0.0, st_data = 0.0, st_bar = 0.0;
                unsigned long long lo = ~0ull, hi = 0;
                for (int64_t p = 0; p < n_patch; ++p) {
                    const unsigned long long* s = h.data() + 12 * p;
                    for (int k = 0; k < 6; ++k) acc[k] += (double)(s[k + 1] - s[k]);
                    lo = std::min(lo, s[0]); hi = std::max(hi, s[6]);
                    cyc += (double)(s[6] - s[0]); real += (double)(s[9] - s[8]);
                    st_ids += (double)(s[10] - s[0]); st_data += (double)(s[11] - s[10]); st_bar += (double)(s[1] - s[11]);
                }
                std::fprintf(stderr, "[fep] staging of thread 0's wave: ids %.0f, node data %.0f, LDS writes + barrier (the other waves) %.0f\n",
                             st_ids / n_patch, st_data / n_patch, st_bar / n_patch);
                std::fprintf(stderr, "[fep] phase clocks, mean per workgroup of %lld (stage, phase1, phase2, wait, image, phase3): "
                             "%.0f %.0f %.0f %.0f %.0f %.0f  sum %.0f; first start -> last end %llu; shader clock %.0f MHz (s_memtime / s_memrealtime x 100 MHz over the workgroups)\n", (long long)n_patch,
                             acc[0] / n_patch, acc[1] / n_patch, acc[2] / n_patch, acc[3] / n_patch, acc[4] / n_patch,
                             acc[5] / n_patch, (acc[0] + acc[1] + acc[2] + acc[3] + acc[4] + acc[5]) / n_patch, hi - lo,
                             real > 0 ? cyc / real * 100.0 : 0.0);
            }
        }
        if (c->p1.v.clk && c->p1.n_tiles > 0) {               // mean shader clocks per phase of the LAST launch of each P1 tile kernel
            const int64_t n = c->p1.n_tiles;
            std::vector<unsigned long long> h((size_t)(16 * n));
            if (hipDeviceSynchronize() == hipSuccess &&
                hipMemcpy(h.data(), c->p1.v.clk, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost) == hipSuccess) {
                for (int k = 0; k < 2; ++k) {
                    double acc[5] = {0, 0, 0, 0, 0}, cyc = 0.0, real = 0.0;
                    int64_t seen = 0;
                    for (int64_t g = 0; g < n; ++g) {
                        const unsigned long long* s = h.data() + 8 * (k * n + g);
                        if (s[5] == 0) continue;            // the kernel did not run
                        ++seen;
                        for (int i = 0; i < 5; ++i) acc[i] += (double)(s[i + 1] - s[i]);
                        cyc += (double)(s[5] - s[0]); real += (double)(s[7] - s[6]);
                    }
                    if (seen == 0) continue;
                    std::fprintf(stderr, "[fep] %s tile clocks, mean per workgroup of %lld (entry -> tables, -> first operand, -> first barrier, "
                                 "-> gather done, -> end): %.0f %.0f %.0f %.0f %.0f  sum %.0f; shader clock %.0f MHz\n",
                                 k == 0 ? "p1_node_lds_kernel" : "p1_fused_kernel", (long long)seen, acc[0] / seen, acc[1] / seen,
                                 acc[2] / seen, acc[3] / seen, acc[4] / seen, cyc / seen, real > 0 ? cyc / real * 100.0 : 0.0);
                }
            }
        }
        delete c->gen;
#endif
        for (void* p : c->owned) (void)hipFree(p);
        for (hipEvent_t ev : c->events) (void)hipEventDestroy(ev);
        c->hbuf.release();
    }
    delete c;
    return FEP_OK;
}

static int ctx_create_impl(fep_ctx*& c, fep_ctx** ctx_out, int device_id, int elem_type, int64_t n_e, int64_t n_n,
                           const int32_t* elements_h, const double* coords_h,
                           const double* dhatp1_h, const double* dhatp2_h, const double* wf_h);

// Nothing may leave an extern "C" entry point by exception: the host symbolic phase allocates multi-GB std::vectors
// (std::bad_alloc at BASELINE configs[4] sizes on a small host) -> FEP_ENOMEM instead of std::terminate.
extern "C" int fep_ctx_create(fep_ctx** ctx_out, int device_id, int elem_type, int64_t n_e, int64_t n_n,
                              const int32_t* elements_h, const double* coords_h,
                              const double* dhatp1_h, const double* dhatp2_h, const double* wf_h) {
    if (!ctx_out) return FEP_EINVAL;
    *ctx_out = nullptr;
    fep_ctx* c = nullptr;
    int r;
    try {
        r = ctx_create_impl(c, ctx_out, device_id, elem_type, n_e, n_n, elements_h, coords_h, dhatp1_h, dhatp2_h, wf_h);
    } catch (const std::bad_alloc&) {
        r = FEP_ENOMEM;
    } catch (...) {
        r = FEP_EINVAL;
    }
    if (r != FEP_OK) { if (c) fep_ctx_destroy(c); *ctx_out = nullptr; }
    return r;
}

// P1 node route: the gather plan (fep_host.h, P1Plan) and its tables.  *taken = false: the product takes the element
// route instead.
static int setup_p1_node(fep_ctx* c, const MeshIn& in, bool* taken) {
    *taken = false;
    P1NodeRoute& r = c->p1;
    fep_host::P1Options opt;
    // FEP_P1_TILE=128: tiles of 128 blocks on 128 threads (16 instead of 8 resident per CU; VERDICT r3 item 5's structural
    // attempt: the K,F-only step measured 0.0706-0.0715 against 0.0629-0.0631 ms, profiles/r04_ablation.md)
    if (const char* tl = fep_tune("FEP_P1_TILE")) r.v.tile = std::atoi(tl) == 128 ? 128 : 256;
    {   // FEP_P1_PATH=node_direct | node_list | node_unpacked | node2k: plans without one of the default's ingredients
        const char* pth = fep_tune("FEP_P1_PATH");
        auto is = [&](const char* v) { return pth && std::strcmp(pth, v) == 0; };
        opt.allow_lds = !is("node_direct");
        opt.allow_rng = !is("node_list");
        opt.allow_pk = !is("node_unpacked");
        opt.allow_fused = !is("node2k");
        if (const char* sg = fep_tune("FEP_P1_SEGS")) opt.max_segs = std::max(1, std::min(std::atoi(sg), fep_host::kSegMax));
    }
    opt.tile = r.v.tile;
    fep_host::P1Plan P;
    FEP_TRY(fep_host::build_p1_plan(in.S, c->n_e, c->n_n, in.elem, opt, P));
    if (in.validate) {
        const int bad = fep_host::validate_p1_plan(P, in.S, c->n_e, c->n_n, in.elem);
        if (bad) { std::fprintf(stderr, "[fep] P1 plan fails check %d\n", bad); return FEP_EINVAL; }
    }
    // A mesh whose tiles do not fit the LDS-staged form or whose descriptor fields do not pack (node degree >= 2^12, ...)
    // takes the element route like every other element type: the product keeps ONE node route.
    if (!kAblationBuild && !(P.lds && P.pk)) {
        if (c->verbose) std::fprintf(stderr, "[fep] P1 plan without the LDS-staged packed form (lds %d pk %d): element route\n", (int)P.lds, (int)P.pk);
        return FEP_OK;
    }
    *taken = true;
    r.n_tiles = (int)P.n_wg;
    r.v.lds = P.lds; r.v.pk = P.pk;                     // (the product's plan has both: above)
    r.L = P.L; r.C = P.C; r.rng = P.rng;
    r.fused = P.fused; r.fused_rng = P.fused_rng; r.NL = P.NL;
    if (const char* am = fep_tune("FEP_P1_ASM")) r.v.asm_from_nodes = std::strcmp(am, "nodes") == 0;
    if (const char* dm = fep_tune("FEP_P1_DMA")) r.v.dma = std::strcmp(dm, "0") != 0;
    if (const char* fm = fep_tune("FEP_P1_FUSED"))
        r.v.fused_mode = std::strcmp(fm, "off") == 0 ? 0 : std::strcmp(fm, "kf") == 0 ? 1 : 2;
    if (fep_tune("FEP_P1_CLK") && P.n_wg > 0) {
        FEP_TRY(dmalloc(c, &r.v.clk, 16 * P.n_wg));
        (void)hipMemset(r.v.clk, 0, (size_t)(16 * P.n_wg) * sizeof(unsigned long long));
    }
    // only the variants that read them get the direct kernel's gather list and the unpacked descriptors (never the product's plan)
    if (!P.lds) FEP_TRY(upload(c, &r.perm2, P.perm2.data(), (int64_t)P.perm2.size()));
    if (!(P.lds && P.pk)) {
        FEP_TRY(upload(c, &r.segptr, in.S.segptr.data(), (int64_t)in.S.segptr.size()));
        FEP_TRY(upload(c, &r.meta, in.S.meta.data(), (int64_t)in.S.meta.size()));
        FEP_TRY(upload(c, &r.ncol, in.S.ncol.data(), (int64_t)in.S.ncol.size()));
    }
    FEP_TRY(upload(c, &r.trec, P.rec.data(), (int64_t)P.rec.size()));
    if (P.lds) {
        FEP_TRY(upload(c, &r.wg_elist, P.elist_pad.data(), (int64_t)P.elist_pad.size()));
        FEP_TRY(upload(c, &r.perm_l, P.codes_pad.data(), (int64_t)P.codes_pad.size()));
        if (P.pk) FEP_TRY(upload(c, &r.pk, (const uint2*)P.pkv.data(), (int64_t)P.pkv.size()));
    }
    if (P.fused) {
        FEP_TRY(upload(c, &r.el_nodes, P.elnodes.data(), (int64_t)P.elnodes.size()));
        if (!P.fused_rng) FEP_TRY(upload(c, &r.wg_nlist, P.nlist_pad.data(), (int64_t)P.nlist_pad.size()));
        FEP_TRY(dmalloc(c, &r.slot_counts, 256 * 16));
        HIP_TRY(hipMemset(r.slot_counts, 0, 256 * 16 * sizeof(unsigned long long)));
    }
    if (c->verbose)
        std::fprintf(stderr, "[fep] P1 plan: %lld tiles of <= %d blocks in <= %d segment(s), staged elements %lld "
                     "(%.2f per element, <= %d per tile), staged nodes <= %d, codes <= %d; lds %d rng %d pk %d fused %d/%d\n",
                     (long long)P.n_wg, P.tile, P.n_segs, (long long)P.staged_total, (double)P.staged_total / (double)c->n_e,
                     P.L, P.NL, P.C, (int)P.lds, (int)P.rng, (int)P.pk, (int)P.fused, (int)P.fused_rng);
    FEP_TRY(dmalloc(c, &r.geo, 6 * c->n_e));
    c->n_count_blocks = (int)grid_for(c->n_e, kBlock);
    return FEP_OK;
}

// Geometry of the element kernel from the coordinates (GEO) or from the streamed dphi arrays, fixed per type and form
// (elem_geo_default): measured on MI355X (1 M elements, element kernel alone): recomputed geometry wins for Q1 (0.204 vs
// 0.218 ms) and Q2 (0.344 vs 0.391 ms with 24 instead of 28 elements per workgroup, so that three workgroups still fit a
// CU) and loses for P2 in the COO form (0.50 vs 0.47 ms at 28 / 32 elements per workgroup); round 3, patch form:
// recomputed geometry wins for P2 as well (same session, 1 M elements: 0.754 vs 0.783 ms on a fast box, 0.888 vs 0.936
// on a slow one); round 4, final patch kernel, one session, two passes each: P4 0.769-0.771 against 0.842-0.869 ms (its 30
// gradient loads per point were a third of its workgroup's life), Q2 0.604 / 0.709, P2 0.632-0.638 / 0.700-0.710, Q1
// 0.163-0.164 / 0.167-0.174: recomputed for every type in the patch form
static void elem_form(fep_ctx* c, bool patch_form) {
    c->elem_form.geo = elem_geo_default(c->elem_type, patch_form);
    if (const char* ge = fep_tune("FEP_ELEM_GEO")) c->elem_form.geo = std::strcmp(ge, "0") != 0;
    if (const char* lp = fep_tune("FEP_ELEM_LDS_PAD")) c->elem_form.lds_pad = std::max(0, std::atoi(lp));
}

// Patch form of the element route (no K_e round trip through HBM; same session, 0.25-4 M elements, profiles/r03_ablation.md,
// r03_elem_bench.log: P2 -17 % (K,F-only -19 %, BASELINE configs[4] -14 %), Q2 -14 %, Q1 -13 %, P4 -21 % against the COO
// form).  *taken = false: no patch plan fits (a descriptor field too wide), the COO form.
static int setup_patch(fep_ctx* c, const MeshIn& in, bool* taken) {
    *taken = false;
    elem_form(c, true);
    // Workgroup shape (threads; lanes per (element, node) pair in phase 2: ElemCfg's JS), fixed per type:
    //   P2  512 / 1: 56 elements on 512 threads (two workgroups of eight waves per CU instead of four of four: the same waves,
    //       2.0 instead of 3.2 partials per element with four runs, fix-up kernel -35 %, element kernel +3-12 %): three boxes,
    //       same session each: 1 M elements 0.653 / 0.681 / 0.724 against 0.700 / 0.713 / 0.716 ms, BASELINE configs[4] 2.61 /
    //       2.89 / 2.89 against 2.86 / 3.09 / 3.00, K,F-only 0.613 against 0.653
    //   Q2  256 / 1 (40 elements on 512 threads, 3.5 instead of 5.8 partials per element: 0.76-0.80 against 0.62 ms; 24 elements
    //       on 384 threads with JS = 2: 0.82-0.83 against 0.62, profiles/r04_ablation.md)
    //   P4  FEP_P4_TPB / FEP_P4_JS
    int tpb = c->elem_type == FEP_P2 ? 512 : c->elem_type == FEP_P4 ? FEP_P4_TPB : 256;
    int js = c->elem_type == FEP_P4 ? FEP_P4_JS : 1;
    bool shape_forced = false;
    if (const char* tpb_env = fep_tune("FEP_PATCH_TPB")) {
        tpb = std::atoi(tpb_env);
        const char* js_env = fep_tune("FEP_PATCH_JS");
        js = js_env ? std::atoi(js_env) : 1;
        shape_forced = true;
    }
    int eb = 0;
    if (elements_per_workgroup(c, true, tpb, js, &eb) != FEP_OK) return FEP_EINVAL;      // no such instantiation
    fep_host::PatchPlan P;
    fep_host::PatchOptions popt;
    if (const char* po = fep_tune("FEP_PATCH_ORDER"))
        popt.order = std::strcmp(po, "consecutive") == 0 ? 0 : std::strcmp(po, "hilbert") == 0 ? 1 : 2;
    // Q1 (64 elements per patch): 4 runs of 16 measured 6 % faster than 2 of 32; P2 with 56 elements: 4 runs of 14
    // (1.96 partials per element) 1-3 % faster than 2 of 28 (2.86); with 28 elements 2 runs of 14 (4 of 7: +7 %)
    popt.runs = (c->elem_type == FEP_Q1 || tpb == 512) ? 4 : 2;
    // (runs starting on 128-byte boundaries of the point arrays — 16 / gcd(16, n_q) elements — measured no faster and
    // cost a third more partials: the aligned starts leave short leftovers)
    if (const char* pr = fep_tune("FEP_PATCH_RUNS")) popt.runs = std::max(1, std::atoi(pr));
    if (const char* pa = fep_tune("FEP_PATCH_ALIGN")) popt.align = std::max(1, std::atoi(pa));
    FEP_TRY(fep_host::build_patch_plan(in.S, c->n_p, c->n_e, c->n_n, in.elem, in.coords, eb, popt, P));
    if (!P.ok && tpb == 512 && js == 1 && !shape_forced) {         // the big patches cannot be built: the small ones
        tpb = 256;                                                  // (a forced shape is never changed silently)
        FEP_TRY(elements_per_workgroup(c, true, tpb, js, &eb));
        if (!fep_tune("FEP_PATCH_RUNS")) popt.runs = 2;
        FEP_TRY(fep_host::build_patch_plan(in.S, c->n_p, c->n_e, c->n_n, in.elem, in.coords, eb, popt, P));
    }
    if (!P.ok) return shape_forced && tpb != 256 ? FEP_ESTATE : FEP_OK;      // (a forced plan that could not be built)
    if (in.validate) {
        const int bad = fep_host::validate_patch_plan(P, in.S, c->n_p, c->n_e, c->n_n, in.elem);
        if (bad) { std::fprintf(stderr, "[fep] patch plan fails check %d\n", bad); return FEP_EINVAL; }
    }
    *taken = true;
    PatchRoute& r = c->patch;
    r.tpb = tpb; r.js = js;
    r.eb = P.eb; r.n_open = P.n_open; r.n_fopen = P.n_fopen; r.n_patch = P.n_patch;
    // one zero pad entry after each item / code table: element_kernel reads them at clamped indices, also for a patch
    // without items
    P.items.push_back(fep_host::U2{0u, 0u});
    P.fitems.push_back(fep_host::U2{0u, 0u});
    P.codes.insert(P.codes.end(), 2, 0);
    P.fcodes.insert(P.fcodes.end(), 2, 0);
    FEP_TRY(upload(c, &r.desc, P.pdesc.data(), (int64_t)P.pdesc.size()));
    FEP_TRY(upload(c, &r.pel, P.pel.data(), (int64_t)P.pel.size()));
    FEP_TRY(upload(c, &r.pnodes, P.pnodes.data(), (int64_t)P.pnodes.size()));
    FEP_TRY(upload(c, &r.items, (const uint2*)P.items.data(), (int64_t)P.items.size()));
    FEP_TRY(upload(c, &r.codes, P.codes.data(), (int64_t)P.codes.size()));
    FEP_TRY(upload(c, &r.fitems, (const uint2*)P.fitems.data(), (int64_t)P.fitems.size()));
    FEP_TRY(upload(c, &r.fcodes, P.fcodes.data(), (int64_t)P.fcodes.size()));
    FEP_TRY(upload(c, &r.fix, (const uint4*)P.fix.data(), (int64_t)P.fix.size()));
    FEP_TRY(upload(c, &r.fixT, (const uint2*)P.fixT.data(), (int64_t)P.fixT.size()));
    FEP_TRY(upload(c, &r.ffix, (const uint4*)P.ffix.data(), (int64_t)P.ffix.size()));
    FEP_TRY(upload(c, &r.plist, P.plist.data(), (int64_t)P.plist.size()));
    if (fep_tune("FEP_PHASE_CLK")) {
        FEP_TRY(dmalloc(c, &r.v.phase_clk, 12 * P.n_patch));
        (void)hipMemset(r.v.phase_clk, 0, (size_t)(12 * P.n_patch) * sizeof(unsigned long long));
    }
    FEP_TRY(dmalloc(c, &r.Pc, 4 * P.n_part));
    FEP_TRY(dmalloc(c, &r.Pf, 2 * P.n_fpart));
    if (c->verbose)
        std::fprintf(stderr, "[fep] patch plan: %lld patches of <= %d elements, %zu items (<= %d per patch), %lld open blocks of %lld, "
                     "%lld partials (%.2f per element), %lld open nodes\n", (long long)P.n_patch, P.eb, P.items.size(), P.max_items,
                     (long long)P.n_open, (long long)c->n_blk, (long long)P.n_part, (double)P.n_part / (double)c->n_e,
                     (long long)P.n_fopen);
    c->n_count_blocks = (int)r.n_patch;
    return FEP_OK;
}

// COO form of the element route: K_e / f_e through HBM, csr_reduce* and the force gather sum them per block / node
static int setup_coo(fep_ctx* c, const MeshIn& in, const std::vector<int32_t>& tstart) {
    elem_form(c, false);
    CooRoute& r = c->coo;
    int eb = 0;
    if (elements_per_workgroup(c, false, kBlock, 1, &eb) != FEP_OK) return FEP_EINVAL;
    c->n_count_blocks = (int)grid_for(c->n_e, eb);
    // measured at ~1 M points per type (tools/elem_bench.py): the element-major layout pays for the 15-node element only
    // (P4: step 1.47 -> 1.35 ms; P2 0.96 -> 1.06, Q2 0.82 -> 0.94, Q1 0.22 -> 0.26: their stores lose coalescing)
    r.kc_aos = c->elem_type == FEP_P4;
    if (const char* kl = fep_tune("FEP_KC_LAYOUT")) r.kc_aos = std::strcmp(kl, "aos") == 0;
    if (const char* cg = fep_tune("FEP_CSR_GATHERS")) r.v.csr_gathers = std::atoi(cg);
    const int n_p = c->n_p;
    const int64_t n_e = c->n_e;
    if ((int64_t)sym_block_count(n_p) * n_e >= (int64_t)1 << 30) return FEP_ERANGE;     // 2 * position fits int32
    const Symbolic& S = in.S;
    {   // element_kernel stores half of the symmetric K_e: re-address the contributions (block, transposed)
        std::vector<int32_t> perm_sym(S.perm.size());
        for (size_t i = 0; i < S.perm.size(); ++i) {
            const int64_t v = S.perm[i];
            const int ab = (int)(v / n_e);
            const int64_t e = v - (int64_t)ab * n_e;
            int idx; bool tr;
            sym_block_index(n_p, ab / n_p, ab % n_p, idx, tr, r.kc_aos);
            const int64_t pos = r.kc_aos ? e * sym_block_count(n_p) + idx : (int64_t)idx * n_e + e;
            perm_sym[i] = (int32_t)(2 * pos + (tr ? 1 : 0));
        }
        perm_sym.resize(perm_sym.size() + 4, 0);                    // csr_reduce_pk_kernel reads the addresses four at a time
        FEP_TRY(upload(c, &r.perm, perm_sym.data(), (int64_t)perm_sym.size()));
    }
    // one 8-byte descriptor per block, if its fields fit (fep_layout.h: pkc)
    std::vector<uint2> pkc((size_t)c->n_blk);
    bool fits = fep_tune("FEP_CSR_UNPACKED") == nullptr;
    for (int64_t b = 0; b < c->n_blk && fits; ++b) {
        const Meta mt = unpack_meta(S.meta[b]);
        const Pkc f{S.segptr[b + 1] - S.segptr[b], mt.deg, mt.slot};
        fits = pkc_fits(f);
        pkc[b] = make_uint2((uint32_t)S.segptr[b], pack_pkc(f.len, f.deg, f.slot));
    }
    if (fits) {
        FEP_TRY(upload(c, &r.pkc, pkc.data(), (int64_t)pkc.size()));
    } else {                                            // csr_reduce_kernel reads every block's contribution list unpacked
        FEP_TRY(upload(c, &r.segptr, S.segptr.data(), (int64_t)S.segptr.size()));
        FEP_TRY(upload(c, &r.meta, S.meta.data(), (int64_t)S.meta.size()));
    }
    FEP_TRY(upload(c, &r.tstart, tstart.data(), (int64_t)tstart.size()));
    r.n_tiles = (int)tstart.size() - 1;
    FEP_TRY(dmalloc(c, &r.Kc, 4 * (int64_t)sym_block_count(n_p) * n_e));
    FEP_TRY(dmalloc(c, &r.fe, 2 * (int64_t)n_p * n_e));
    return FEP_OK;
}

// The route of a new context, from its element type, FEP_ROUTE and whether the route's plan can be built:
//   P1         the node route unless FEP_ROUTE names a form of the element route (the product takes the patch form for a
//              plan without the LDS-staged packed form: setup_p1_node)
//   P2 Q1 Q2   (ablation build, FEP_GEN_PATH=node) the GenNode route if its plan fits
//   otherwise  the patch form unless FEP_ROUTE=coo; the COO form if no patch plan fits
static int choose_route(fep_ctx* c, const MeshIn& in, const std::vector<int32_t>& tstart) {
    const bool route_coo = env_is("FEP_ROUTE", "coo"), route_patch = env_is("FEP_ROUTE", "patch");
    bool taken = false;
    if (c->elem_type == FEP_P1) {                       // the reference-element tables by value, on EVERY route: the node route's kernels
                                                        // and the point kernel of a von Mises / Mohr-Coulomb step (step_model) take them
        for (int a = 0; a < 3; ++a) { c->p1tab.h1[a] = in.dh1[a]; c->p1tab.h2[a] = in.dh2[a]; }
        c->p1tab.wf = in.wf[0];
    }
    if (c->elem_type == FEP_P1 && !route_coo && !route_patch) {
        FEP_TRY(setup_p1_node(c, in, &taken));
        if (taken) c->route = Route::P1Node;
    }
#ifdef FEP_ABLATION
    else if (c->elem_type == FEP_P2 || c->elem_type == FEP_Q1 || c->elem_type == FEP_Q2) {
        const char* gp = fep_tune("FEP_GEN_PATH");
        if (gp && std::strcmp(gp, "node") == 0) FEP_TRY(setup_gen_node(c, in, &taken));
        if (taken) c->route = Route::GenNode;
    }
#endif
    if (!taken && !route_coo) {
        FEP_TRY(setup_patch(c, in, &taken));
        if (taken) c->route = Route::Patch;
    }
    if (!taken) {
        c->route = Route::Coo;
        FEP_TRY(setup_coo(c, in, tstart));
    }
    return FEP_OK;
}

static int ctx_create_impl(fep_ctx*& c, fep_ctx** ctx_out, int device_id, int elem_type, int64_t n_e, int64_t n_n,
                           const int32_t* elements_h, const double* coords_h,
                           const double* dhatp1_h, const double* dhatp2_h, const double* wf_h) {
    int n_p = 0, n_q = 0;
    FEP_TRY(fep_element_shape(elem_type, &n_p, &n_q));
    if (n_e <= 0 || n_n <= 0 || !elements_h || !coords_h || !dhatp1_h || !dhatp2_h || !wf_h) return FEP_EINVAL;
    if (n_e * (int64_t)n_q >= INT32_MAX / 16) return FEP_ERANGE;
    Symbolic S;
    FEP_TRY(build_symbolic(n_p, n_e, n_n, elements_h, S));
    FEP_TRY(fep_set_device(device_id));
    c = new (std::nothrow) fep_ctx();
    if (!c) return FEP_ENOMEM;
    c->device = device_id; c->elem_type = elem_type; c->n_p = n_p; c->n_q = n_q;
    c->verbose = env_now("FEP_VERBOSE") != nullptr;
    c->n_e = n_e; c->n_n = n_n; c->n_int = n_e * n_q; c->n_dof = 2 * n_n;
    c->n_blk = (int64_t)S.ncol.size(); c->nnz = 4 * c->n_blk;
    size_host_buffers(c);
    for (int64_t n = 0; n < n_n && !c->has_orphans; ++n) c->has_orphans = S.iptr[n + 1] == S.iptr[n];
    // host CSR pattern on DOFs
    c->indptr.resize(c->n_dof + 1);
    c->indices.resize(c->nnz);
    for (int64_t n = 0; n < n_n; ++n) {
        const int64_t d = S.nptr[n + 1] - S.nptr[n];
        for (int i = 0; i < 2; ++i) {
            const int64_t start = 4 * (int64_t)S.nptr[n] + i * 2 * d;
            c->indptr[2 * n + i] = (int32_t)start;
            for (int64_t s = 0; s < d; ++s) {
                c->indices[start + 2 * s] = 2 * S.ncol[S.nptr[n] + s];
                c->indices[start + 2 * s + 1] = 2 * S.ncol[S.nptr[n] + s] + 1;
            }
        }
    }
    c->indptr[c->n_dof] = (int32_t)c->nnz;
    FEP_TRY(upload(c, &c->elem, elements_h, (int64_t)n_p * n_e));
    FEP_TRY(upload(c, &c->coords, coords_h, 2 * n_n));
    FEP_TRY(upload(c, &c->dh1, dhatp1_h, (int64_t)n_p * n_q));
    FEP_TRY(upload(c, &c->dh2, dhatp2_h, (int64_t)n_p * n_q));
    FEP_TRY(upload(c, &c->wf, wf_h, (int64_t)n_q));
    FEP_TRY(dmalloc(c, &c->dphi1, (int64_t)n_p * c->n_int));
    FEP_TRY(dmalloc(c, &c->dphi2, (int64_t)n_p * c->n_int));
    FEP_TRY(dmalloc(c, &c->weight, c->n_int));
    FEP_TRY(dmalloc(c, &c->det, c->n_int));
    FEP_TRY(dmalloc(c, &c->shear, c->n_int)); FEP_TRY(dmalloc(c, &c->bulk, c->n_int));
    FEP_TRY(dmalloc(c, &c->eta, c->n_int)); FEP_TRY(dmalloc(c, &c->c, c->n_int));
    {   // interleaved (x, y) per node: the kernels recompute dphi / weight from the coordinates
        std::vector<double> xy(2 * (size_t)n_n);
        for (int64_t n = 0; n < n_n; ++n) { xy[2 * n] = coords_h[n]; xy[2 * n + 1] = coords_h[n_n + n]; }
        FEP_TRY(upload(c, &c->xy, xy.data(), (int64_t)xy.size()));
    }
    // node -> incident (element, local node) lists: force gather of the COO route and fep_transform_*
    FEP_TRY(upload(c, &c->iptr, S.iptr.data(), (int64_t)S.iptr.size()));
    FEP_TRY(upload(c, &c->ilist, S.ilist.data(), (int64_t)S.ilist.size()));
    // COO route: tiles of whole nodes with at most kBlock node-pair blocks (csr_reduce_kernel's work units; a node of more
    // blocks is refused on every route)
    std::vector<int32_t> tstart;
    FEP_TRY(fep_host::row_tiles(S, n_n, kBlock, tstart));
    FEP_TRY(choose_route(c, MeshIn{S, elements_h, coords_h, dhatp1_h, dhatp2_h, wf_h, env_now("FEP_VALIDATE_PLAN") != nullptr},
                         tstart));
    FEP_TRY(dmalloc(c, &c->blk_counts, std::max<int64_t>(c->n_count_blocks, grid_for(c->n_int, kBlock))));
    FEP_TRY(launch_geometry(c, c->route == Route::P1Node ? c->p1.geo : nullptr));
    if (hipDeviceSynchronize() != hipSuccess) { g_last_hip = (int)hipGetLastError(); return FEP_EHIP; }
    *ctx_out = c;
    return FEP_OK;
}

extern "C" int fep_ctx_sizes(const fep_ctx* c, int64_t sizes[8]) {
    if (!c || !sizes) return FEP_EINVAL;
    sizes[0] = c->n_e; sizes[1] = c->n_n; sizes[2] = c->n_p; sizes[3] = c->n_q;
    sizes[4] = c->n_int; sizes[5] = c->n_dof; sizes[6] = c->nnz; sizes[7] = c->n_blk;
    return FEP_OK;
}

// What plan_step reads of a context
static fep_plan::StepFacts facts_of(const fep_ctx* c) {
    fep_plan::StepFacts f;
    f.route = c->route;
    f.dp = c->model == FEP_MODEL_DP;
    f.lds = c->p1.v.lds; f.fused = c->p1.fused; f.fused_mode = c->p1.v.fused_mode; f.asm_from_nodes = c->p1.v.asm_from_nodes;
    f.pkc = c->coo.pkc != nullptr;
    return f;
}

// The only place that allocates the internal ds / s arrays (fep_plan::Scratch: a plan's `need`, or prealloc_scratch of the
// context's facts), each once; refused while `st` is being captured
static int ensure_scratch(fep_ctx* c, hipStream_t st, fep_plan::Scratch need) {
    const bool want_ds = need.ds && !c->ds_int, want_s = need.s && !c->s_int;
    if (want_ds || want_s) FEP_TRY(scratch_alloc_allowed(st));
    if (want_ds) FEP_TRY(dmalloc(c, &c->ds_int, 9 * c->n_int));
    if (want_s) FEP_TRY(dmalloc(c, &c->s_int, 4 * c->n_int));
    return FEP_OK;
}

extern "C" int fep_ctx_geometry_host(fep_ctx* c, double* dphi1_h, double* dphi2_h, double* weight_h, double* det_h) {
    if (!c) return FEP_EINVAL;
    FEP_TRY(fep_set_device(c->device));
    const size_t nb = (size_t)c->n_int * sizeof(double);
    if (dphi1_h) HIP_TRY(hipMemcpy(dphi1_h, c->dphi1, nb * c->n_p, hipMemcpyDeviceToHost));
    if (dphi2_h) HIP_TRY(hipMemcpy(dphi2_h, c->dphi2, nb * c->n_p, hipMemcpyDeviceToHost));
    if (weight_h) HIP_TRY(hipMemcpy(weight_h, c->weight, nb, hipMemcpyDeviceToHost));
    if (det_h) HIP_TRY(hipMemcpy(det_h, c->det, nb, hipMemcpyDeviceToHost));
    return FEP_OK;
}

extern "C" int fep_ctx_pattern_host(const fep_ctx* c, int32_t* indptr_h, int32_t* indices_h) {
    if (!c) return FEP_EINVAL;
    if (indptr_h) std::memcpy(indptr_h, c->indptr.data(), c->indptr.size() * sizeof(int32_t));
    if (indices_h) std::memcpy(indices_h, c->indices.data(), c->indices.size() * sizeof(int32_t));
    return FEP_OK;
}

extern "C" int fep_ctx_set_materials_host(fep_ctx* c, const double* shear_h, const double* bulk_h,
                                          const double* eta_h, const double* c_h) {
    if (!c || !shear_h || !bulk_h || !eta_h || !c_h) return FEP_EINVAL;
    FEP_TRY(fep_set_device(c->device));
    const size_t nb = (size_t)c->n_int * sizeof(double);
    HIP_TRY(hipMemcpy(c->shear, shear_h, nb, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->bulk, bulk_h, nb, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->eta, eta_h, nb, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->c, c_h, nb, hipMemcpyHostToDevice));
    c->have_materials = true;
    // the ds / s scratch of every step that does not allocate on first use must exist before the first fep_step_dev (which
    // may run inside a stream capture)
    FEP_TRY(ensure_scratch(c, nullptr, fep_plan::prealloc_scratch(facts_of(c))));
    // every parameter constant over the mesh (the reference's demos): the kernels skip the four arrays
    bool uni = fep_tune("FEP_NO_UNIFORM") == nullptr;
    for (int64_t k = 1; uni && k < c->n_int; ++k)
        uni = shear_h[k] == shear_h[0] && bulk_h[k] == bulk_h[0] && eta_h[k] == eta_h[0] && c_h[k] == c_h[0];
    c->matu = MatU{shear_h[0], bulk_h[0], eta_h[0], c_h[0], uni ? 1 : 0};
    return FEP_OK;
}

// The models besides Drucker-Prager run as point kernel + the route's assembly: their ds / s scratch is allocated here, so
// that fep_step_dev never allocates on such a context.
extern "C" int fep_ctx_set_model(fep_ctx* c, int model) {
    if (!c || with_model(model, [](auto) { return FEP_OK; }) != FEP_OK) return FEP_EINVAL;
    if (model != FEP_MODEL_DP) {
        if (c->route == Route::GenNode) return FEP_ESTATE;
        FEP_TRY(fep_set_device(c->device));
        fep_plan::StepFacts facts = facts_of(c);
        facts.dp = false;
        const fep_plan::Scratch need = fep_plan::prealloc_scratch(facts);
        if (!fep_plan::covers(fep_plan::Scratch{c->ds_int != nullptr, c->s_int != nullptr}, need)) {
            // refused while a capture is in progress (the query on the default stream fails during a capture on another)
            hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
            if (hipStreamIsCapturing(nullptr, &cs) != hipSuccess) { (void)hipGetLastError(); return FEP_ESTATE; }
            if (cs != hipStreamCaptureStatusNone) return FEP_ESTATE;
        }
        FEP_TRY(ensure_scratch(c, nullptr, need));
    }
    c->model = model;
    return FEP_OK;
}

// (the curve of a context outlives a change of its model and back: only this call writes it)
extern "C" int fep_ctx_set_hardening(fep_ctx* c, int n_seg, const double* kappa_h, const double* slope_h) {
    if (!c) return FEP_EINVAL;
    if (c->model != FEP_MODEL_VMI) return FEP_ESTATE;
    Hard hard;
    FEP_TRY(make_hard(n_seg, kappa_h, slope_h, &hard));
    c->hard = hard;
    return FEP_OK;
}

extern "C" int fep_ctx_model(const fep_ctx* c, int* model) {
    if (!c || !model) return FEP_EINVAL;
    *model = c->model;
    return FEP_OK;
}

extern "C" int fep_ctx_device_ptr(const fep_ctx* c, int which, void** ptr_d) {
    if (!c || !ptr_d) return FEP_EINVAL;
    switch (which) {
        case 0: *ptr_d = c->shear; break;
        case 1: *ptr_d = c->bulk; break;
        case 2: *ptr_d = c->eta; break;
        case 3: *ptr_d = c->c; break;
        case 4: *ptr_d = c->weight; break;
        case 5: *ptr_d = c->dphi1; break;
        case 6: *ptr_d = c->dphi2; break;
        default: return FEP_EINVAL;
    }
    return FEP_OK;
}

// The kernels of a plan as rocprofv3 prints them, joined by " + " (fep_ctx_kernel_names).  Each name_* function stands next
// to the launcher that picks the kernel's template arguments and reads the same fields
struct Names {
    char s[512] = "";
    size_t n = 0;
    template <class... A> void add(const char* fmt, A... a) {
        if (n) n += (size_t)std::snprintf(s + n, sizeof s - n, " + ");
        n = std::min(n, sizeof s - 1);
        n += (size_t)std::snprintf(s + n, sizeof s - n, fmt, a...);
        n = std::min(n, sizeof s - 1);
    }
};
static const char* tf(bool v) { return v ? "true" : "false"; }

// ---------------------------------------------------------------------------------------
// hot path
// ---------------------------------------------------------------------------------------
static int prof_mark(fep_ctx* c, hipStream_t st) {
    if (!c->profiling) return FEP_OK;
    hipEvent_t ev;
    HIP_TRY(hipEventCreate(&ev));
    c->events.push_back(ev);
    HIP_TRY(hipEventRecord(ev, st));
    return FEP_OK;
}

static constexpr size_t kLdsDefault = 64 * 1024;        // dynamic LDS a launch gets without raising the kernel's limit

// Nodes of no element get no block: no kernel writes their force except the COO form's force gather.  Their F is zeroed
// per call, before mark 0 on the node routes, inside stage A on the patch route (in_stage_a).
static int zero_orphan_forces(fep_ctx* c, hipStream_t st, double* f_out, bool in_stage_a) {
    if (!c->has_orphans || !f_out || c->route == Route::Coo || in_stage_a != (c->route == Route::Patch)) return FEP_OK;
    HIP_TRY(hipMemsetAsync(f_out, 0, (size_t)c->n_dof * sizeof(double), st));
    return FEP_OK;
}

// What fep_step_dev, a staged step and fep_assemble_dev open with: the orphans' forces on the node routes, mark 0, the
// orphans' forces on the patch route
static int begin_call(fep_ctx* c, hipStream_t st, double* f_out) {
    FEP_TRY(zero_orphan_forces(c, st, f_out, false));
    FEP_TRY(prof_mark(c, st));
    return zero_orphan_forces(c, st, f_out, true);
}

// element routes, stage A: element_kernel.  Patch form: phase 3 writes the caller's CSR values / force, fixup_kernel the
// open rest; COO form: K_e / f_e to HBM (coo.Kc, coo.fe) when K / F are wanted.  The one launcher the two forms share: it
// reads `ef` and, by the route, the patch form's tables or the COO form's scratch
template <bool FROM_U>
static int launch_element(fep_ctx* c, const ElemForm& ef, hipStream_t st, const double* u, E0 e0, double* ep, int accept,
                          double* eout, double* s, double* ds, uint8_t* indp, uint2* blk_counts, double* k_data, double* f_out) {
    const bool patch = c->route == Route::Patch;
    const PatchRoute& pr = c->patch;                    // (all defaults on the COO form: no tables, 256 threads)
    double* Kc = !patch && k_data ? c->coo.Kc : nullptr;
    double* fe = !patch && f_out ? c->coo.fe : nullptr;
    const PatchArgs pa{pr.desc, pr.pel, pr.pnodes, pr.items, pr.codes, pr.fitems, pr.fcodes, pr.Pc, pr.Pf,
                       patch ? k_data : nullptr, patch ? f_out : nullptr
#ifdef FEP_ABLATION
                       , pr.v.phase_clk
#endif
    };
    FEP_TRY(elem_shape(c->elem_type, patch, ef.geo, pr.tpb, pr.js, [&](auto et, auto pf, auto geo, auto tpb_c, auto js_c) {
        using ET = decltype(et);
        constexpr bool PATCH = decltype(pf)::value, GEO = decltype(geo)::value;
        constexpr int TPB = decltype(tpb_c)::value, JS = decltype(js_c)::value;
        using Cfg = ElemCfg<ET::NP, ET::NQ, GEO, TPB, JS>;
        if (pr.eb != 0 && pr.eb != Cfg::EB) return FEP_ESTATE;
        hipLaunchKernelGGL((element_kernel<ET::NP, ET::NQ, FROM_U, GEO, PATCH, TPB, JS>),
                           dim3(PATCH ? (unsigned)pr.n_patch : grid_for(c->n_e, Cfg::EB)), dim3(TPB), (size_t)ef.lds_pad, st, c->n_e,
                           c->elem, c->dphi1, c->dphi2, c->weight, c->xy, c->dh1, c->dh2, c->wf, u, e0, ep, c->shear,
                           c->bulk, c->eta, c->c, c->matu, accept, eout, s, ds, indp, blk_counts, Kc, fe, c->coo.kc_aos ? 1 : 0, pa);
        return FEP_OK;
    }));
    HIP_TRY(hipGetLastError());
    return FEP_OK;
}
static void name_element(const fep_ctx* c, const ElemForm& ef, bool from_u, Names& o) {
    const bool patch = c->route == Route::Patch;
    o.add("element_kernel<%d, %d, %s, %s, %s, %d, %d>", c->n_p, c->n_q, tf(from_u), tf(ef.geo), tf(patch), c->patch.tpb, c->patch.js);
}

// COO form, stage B (K wanted): K_e blocks -> CSR values (the force gather rides in the reduce kernel's launch: the workgroups
// past the last tile take 256 nodes each; so does the sum of `n_counts` branch counters).  `form`: StageB::ReducePk or Reduce
static int reduce_gathers(const CooRoute& r) {          // gathers in flight of the unpacked form: four, but for the ablation switch
    const int g = r.v.csr_gathers;
    return kAblationBuild && (g == 2 || g == 6 || g == 8) ? g : 4;
}
static int launch_reduce(fep_ctx* c, const CooRoute& r, hipStream_t st, StageB form, double* k_data, double* f_out, int n_counts,
                         unsigned long long* counts_d) {
    ForceArgs fa{c->n_n, c->iptr, c->ilist, r.fe, f_out};
    const unsigned grid = (unsigned)r.n_tiles + (counts_d ? 1u : 0u) + (f_out ? grid_for(c->n_n, kBlock) : 0u);
    auto reduce = [&](auto gathers) {
        hipLaunchKernelGGL(csr_reduce_kernel<decltype(gathers)::value>, dim3(grid), dim3(kBlock), 0, st,
                           r.n_tiles, r.tstart, r.segptr, r.perm, r.meta, r.Kc, k_data, n_counts, c->blk_counts, counts_d, fa);
    };
    if (form == StageB::ReducePk)
        hipLaunchKernelGGL(csr_reduce_pk_kernel, dim3(grid), dim3(kBlock), 0, st, r.n_tiles,
                           r.tstart, r.pkc, r.perm, r.Kc, k_data, n_counts, c->blk_counts, counts_d, fa);
#ifdef FEP_ABLATION
    else if (reduce_gathers(r) == 2) reduce(int_c<2>{});
    else if (reduce_gathers(r) == 6) reduce(int_c<6>{});
    else if (reduce_gathers(r) == 8) reduce(int_c<8>{});
#endif
    else reduce(int_c<4>{});                             // (descriptor fields too wide for the packed form: four gathers in flight)
    HIP_TRY(hipGetLastError());
    return FEP_OK;
}
static void name_reduce(const CooRoute& r, StageB form, Names& o) {
    if (form == StageB::ReducePk) o.add("%s", "csr_reduce_pk_kernel");
    else o.add("csr_reduce_kernel<%d>", reduce_gathers(r));
}

// COO form, stage C: the force gather when the reduce kernel did not take it
static int launch_force(fep_ctx* c, const CooRoute& r, hipStream_t st, double* f_out) {
    hipLaunchKernelGGL(force_reduce_kernel, dim3(grid_for(c->n_n, kBlock)), dim3(kBlock), 0, st,
                       c->n_n, c->iptr, c->ilist, r.fe, f_out);
    HIP_TRY(hipGetLastError());
    return FEP_OK;
}

// patch form, stage B: open blocks / open nodes from the patches' partials (+ the sum of `n_counts` branch counters on the
// side).  A mesh whose patches leave nothing open gives an empty grid when no counters are summed: nothing is launched
static int launch_fixup(fep_ctx* c, const PatchRoute& r, hipStream_t st, double* k_data, double* f_out, int n_counts,
                        unsigned long long* counts_d) {
    const unsigned nb_k = k_data ? grid_for(r.n_open, kBlock) : 0u;
    const unsigned nb_f = f_out ? grid_for(r.n_fopen, kBlock) : 0u;
    const unsigned grid = nb_k + nb_f + (counts_d ? 1u : 0u);
    if (grid == 0) return FEP_OK;
    hipLaunchKernelGGL(fixup_kernel, dim3(grid), dim3(kBlock), 0, st, (int)nb_k, r.n_open, r.fix, r.fixT, r.n_fopen, r.ffix,
                       r.plist, r.Pc, r.Pf, k_data, f_out, n_counts, c->blk_counts, counts_d);
    HIP_TRY(hipGetLastError());
    return FEP_OK;
}

// P1 node route, stage B (K or F wanted): the assembly kernel `form` names -- StageB::Tile, Direct or FromNodes -- reads ds / s,
// writes CSR values and nodal force; with `counts_d` it also sums `n_counts` per-workgroup branch counters (not the direct kernel)
static int launch_p1_node(fep_ctx* c, const P1NodeRoute& r, hipStream_t st, StageB form, const double* ds, const double* s,
                          double* k_data, double* f_out, int n_counts, unsigned long long* counts_d) {
    if (!k_data) ds = nullptr;
    if (!f_out) s = nullptr;
    const int n_wg = r.n_tiles;
    const unsigned grid = xcd_grid(n_wg);
#ifdef FEP_ABLATION
    if (form == StageB::FromNodes) {
        // opt-in (FEP_P1_ASM=nodes): assembly-only form of the one-kernel step, geometry from the tile's LDS-staged nodes
        // instead of the 48-byte record per staged element (same values bit for bit; 25 % fewer bytes but one barrier
        // and the geometry arithmetic more: 72.0 against 66.4 us at 1 M elements, profiles/r02_ablation.md)
        const size_t lds = (size_t)p1_tile_lds(r.L, r.C, r.NL, r.v.tile, false, true).total;
        if (r.L > 256 || r.NL > 256) return FEP_ESTATE;
        FEP_TRY(with_bool(r.fused_rng, [&](auto rng) {
            return launch_lds(p1_fused_kernel<false, 256, decltype(rng)::value, 1, 1, true>, grid, 256, lds, kLdsDefault, st,
                              c->n_e, r.L, r.C, r.NL, r.perm_l, r.wg_elist,
                              r.wg_nlist, r.el_nodes, r.pk, r.trec, c->xy, c->p1tab,
                              (const double*)nullptr, make_e0(nullptr), (const double*)nullptr, c->shear, c->bulk, c->eta,
                              c->c, c->matu, (double*)nullptr, (double*)nullptr, (double*)nullptr, (uint8_t*)nullptr,
                              k_data, f_out, n_wg, (unsigned long long*)nullptr, ds, s, n_counts, c->blk_counts, counts_d,
                              r.v.clk ? r.v.clk + 8 * (size_t)n_wg : (unsigned long long*)nullptr);
        }));
        return FEP_OK;
    }
    if (form == StageB::Direct) {
        hipLaunchKernelGGL(p1_node_kernel, dim3(grid_for(c->n_blk, kBlock)), dim3(kBlock), 0, st,
                           c->n_blk, c->n_e, r.segptr, r.perm2, r.meta, r.ncol, r.geo, ds, s, k_data, f_out);
        HIP_TRY(hipGetLastError());
        return FEP_OK;
    }
#endif
    if (form != StageB::Tile) return FEP_ESTATE;        // (the product runs the tile kernel alone)
    // operands + codes while gathering, then the same LDS holds the tile's output (4*TPB values + forces)
    const size_t lds = (size_t)p1_tile_lds(r.L, r.C, 0, r.v.tile, false, false).total;
    if (c->verbose) {
        static bool once = false;
        if (!once) {
            once = true;
            std::fprintf(stderr, "[fep] p1 assembly kernel: %d tiles of <= %d blocks, staged elements <= %d, codes <= %d, "
                         "LDS %zu bytes per workgroup\n", n_wg, r.v.tile, r.L, r.C, lds);
        }
    }
    // tiles of 128 blocks (ablation build, FEP_P1_TILE) or 256 (128 / 512 were measured slower, profiles/r01_ablation.md)
    FEP_TRY(with_ablation_bool<false>(r.v.tile == 128, [&](auto t128) {
        constexpr int TPB = decltype(t128)::value ? 128 : 256;
        if (r.L > TPB) return FEP_ESTATE;          // one staged element per lane (fep_host.h)
        return with_bool(r.rng, [&](auto rng) {
            // (the product's node route always has packed descriptors: setup_p1_node.  That instantiation never reads
            // segptr, meta and ncol -- every use lies behind the compile-time PK -- and gets them as NULL)
            return with_ablation_bool<true>(r.v.pk, [&](auto pk) {
                return launch_lds(p1_node_lds_kernel<TPB, decltype(rng)::value, 1, decltype(pk)::value>, grid, TPB, lds,
                                  kLdsDefault, st, c->n_e, r.L, r.C, r.segptr, r.perm_l, r.meta, r.ncol,
                                  r.wg_elist, r.pk, r.trec, r.geo, ds, s, k_data, f_out, n_wg,
                                  n_counts, c->blk_counts, counts_d
#ifdef FEP_ABLATION
                                  , r.v.clk
#endif
                                  );
            });
        });
    }));
    return FEP_OK;
}
static void name_p1_node(const P1NodeRoute& r, StageB form, Names& o) {
    if (form == StageB::FromNodes) o.add("p1_fused_kernel<false, 256, %s, 1, 1, true, false>", tf(r.fused_rng));
    else if (form == StageB::Direct) o.add("%s", "p1_node_kernel");
    else o.add("p1_node_lds_kernel<%d, %s, 1, %s>", r.v.tile, tf(r.rng), tf(r.v.pk));
}

// P1, one kernel per step (non-accepting calls with K and/or F wanted): p1_fused_kernel, then the counter sum
static int launch_p1_fused(fep_ctx* c, const P1NodeRoute& r, hipStream_t st, const double* u, E0 e0, const double* ep, double* eout,
                           double* s, double* ds, uint8_t* indp, double* k_data, double* f_out, unsigned long long* counts_d) {
    const bool dma = r.v.dma;
    const size_t lds = (size_t)p1_tile_lds(r.L, r.C, r.NL, r.v.tile, dma, true).total;
    const int n_wg = r.n_tiles;
    const unsigned grid = xcd_grid(n_wg);
    // L, NL <= threads: one staged element / node per lane (fep_host.h)
    if (r.L > r.v.tile || r.NL > r.v.tile) return FEP_ESTATE;
    // (the product runs the one-kernel step for K,F-only calls: fused_mode 1)
    const bool full = eout || s || ds || indp;
    FEP_TRY(with_ablation_bool<false>(full, [&](auto full_c) {
        return with_bool(r.fused_rng, [&](auto rng) {
            return with_ablation_bool<false>(dma, [&](auto dma_c) {
                return with_ablation_bool<false>(r.v.tile == 128, [&](auto t128) {
                    constexpr int TPB = decltype(t128)::value ? 128 : 256;
                    return launch_lds(p1_fused_kernel<decltype(full_c)::value, TPB, decltype(rng)::value, 1, 1, false, decltype(dma_c)::value>,
                                      grid, TPB, lds, kLdsDefault, st, c->n_e, r.L, r.C, r.NL, r.perm_l,
                                      r.wg_elist, r.wg_nlist, r.el_nodes,
                                      r.pk, r.trec, c->xy, c->p1tab, u, e0, ep, c->shear, c->bulk, c->eta, c->c, c->matu,
                                      eout, s, ds, indp, k_data, f_out, n_wg,
                                      counts_d ? r.slot_counts : (unsigned long long*)nullptr, (const double*)nullptr,
                                      (const double*)nullptr, 0, (const uint2*)nullptr, (unsigned long long*)nullptr
#ifdef FEP_ABLATION
                                      , r.v.clk ? r.v.clk + 8 * (size_t)n_wg : (unsigned long long*)nullptr
#endif
                                      );
                });
            });
        });
    }));
    if (counts_d) {
        hipLaunchKernelGGL(counts_finalize_kernel, dim3(1), dim3(256), 0, st, r.slot_counts, counts_d);
        HIP_TRY(hipGetLastError());
    }
    return FEP_OK;
}
static void name_p1_fused(const P1NodeRoute& r, bool full, Names& o) {
    o.add("p1_fused_kernel<%s, %d, %s, 1, 1, false, %s>", tf(full), r.v.tile, tf(r.fused_rng), tf(r.v.dma));
}

// Stage A of a staged step, and of Drucker-Prager's two-kernel P1 step: the point kernel of the context's model (ModelKernels),
// p1_point_* for the 3-node triangle and point_*<NP, NQ> for the other types, with `field` its *_field_kernel
static int launch_point_stage(fep_ctx* c, hipStream_t st, const double* u, E0 e0, double* ep, int accept, double* eout,
                              double* s, double* ds, uint8_t* indp, uint2* blk, const double* field, double scale) {
    const unsigned n_blocks = grid_for(c->n_int, kBlock);
    const PointExtras x{field, scale, &c->hard};
    return with_type(c->elem_type, [&](auto et) {
        using ET = decltype(et);
        return with_model(c->model, [&](auto m) {
            using MK = ModelKernels<decltype(m)::value>;
            return with_bool(field != nullptr, [&](auto fld) {
                constexpr bool FIELD = decltype(fld)::value;
                if constexpr (ET::type == FEP_P1)
                    return launch_point_kernel<MK, FIELD>(MK::template p1_point<FIELD>, n_blocks, st, x, c->n_e, c->elem, c->xy,
                                                          c->p1tab, u, e0, ep, c->shear, c->bulk, c->eta, c->c, c->matu, accept,
                                                          eout, s, ds, indp, blk);
                else    // (Drucker-Prager has none without a field: fep_step_dev takes the element route)
                    return launch_point_kernel<MK, FIELD>(MK::template point<FIELD, ET::NP, ET::NQ>, n_blocks, st, x, c->n_e,
                                                          c->elem, c->xy, c->dh1, c->dh2, c->wf, u, e0, ep, c->shear, c->bulk,
                                                          c->eta, c->c, c->matu, accept, eout, s, ds, indp, blk);
            });
        });
    });
}

static int name_point_stage(const fep_ctx* c, Names& o) {       // (without a field: the steps fep_ctx_kernel_names describes)
    return with_model(c->model, [&](auto m) {
        const char* tag = ModelKernels<decltype(m)::value>::tag;
        if (c->elem_type == FEP_P1) o.add("p1_point_%skernel", tag);
        else o.add("point_%skernel<%d, %d>", tag, c->n_p, c->n_q);
        return FEP_OK;
    });
}

// What a call hands to run_step.  s / ds: the caller's arrays (fep_assemble_dev: its inputs), NULL where it has none
struct StepArgs {
    const double* u; E0 e0; double* ep; int accept;
    double *e, *s, *ds; uint8_t* indp;
    double *K, *F; unsigned long long* cnt;
    const double* field; double scale;
};

// The one launch sequence of fep_step_dev, fep_step_field_dev and fep_assemble_dev, which record four events per call
// (fep_ctx_profile_end: three intervals):
//   begin_call (mark 0), stage A, mark 1, the assembly-only element kernel of a staged step, stage B (with counts_finalize_kernel
//   behind the one-kernel step), mark 2, stage C (COO form: the force gather), mark 3, counts_reduce_kernel if no kernel took the sum
static int run_step(fep_ctx* c, hipStream_t st, const StepPlan& p, const StepArgs& a) {
    using fep_plan::CountGrid;
    using fep_plan::CountSum;
    double* ds = a.ds ? a.ds : p.use.ds ? c->ds_int : nullptr;
    double* s = a.s ? a.s : p.use.s ? c->s_int : nullptr;
    // the per-workgroup counters the summing launch reads: those of the stage that counted (the one-kernel step counts in its slots)
    const int n_counts = p.grid == CountGrid::RouteStageA ? c->n_count_blocks : p.grid == CountGrid::PointKernel ? (int)grid_for(c->n_int, kBlock) : 0;
    uint2* blk = n_counts ? c->blk_counts : nullptr;
    unsigned long long* cnt_b = p.sum == CountSum::StageB || p.sum == CountSum::Finalize ? a.cnt : nullptr;
    auto element_from_u = [&] { return launch_element<true>(c, c->elem_form, st, a.u, a.e0, a.ep, a.accept, a.e, s, ds, a.indp, blk, a.K, a.F); };
    auto element_from_ds = [&] { return launch_element<false>(c, c->elem_form, st, nullptr, make_e0(nullptr), nullptr, 0, nullptr, s, ds, nullptr, nullptr, a.K, a.F); };
    hipStream_t ms = st;                                // stream of marks 1-3 and of stages B and C
#ifdef FEP_ABLATION
    // FEP_FIX_SIDE=1 — an UPPER BOUND, not a route: fixup_kernel on a side stream, NOT ordered behind this call's element kernel (it
    // adds whatever partials the call before left; K's open blocks are stale), joined at the end: what a perfectly overlapped
    // fix-up could save
    const bool fix_side = p.a == StageA::ElementFromU && c->route == Route::Patch && fep_tune("FEP_FIX_SIDE");
    static hipStream_t side = nullptr;
    static hipEvent_t ev_a = nullptr, ev_b = nullptr;
    if (fix_side && !side) { HIP_TRY(hipStreamCreateWithFlags(&side, hipStreamNonBlocking)); HIP_TRY(hipEventCreateWithFlags(&ev_a, hipEventDisableTiming)); HIP_TRY(hipEventCreateWithFlags(&ev_b, hipEventDisableTiming)); }
#else
    constexpr bool fix_side = false;
#endif
    FEP_TRY(begin_call(c, st, a.F));
    switch (p.a) {
        case StageA::None: break;
        case StageA::Point: FEP_TRY(launch_point_stage(c, st, a.u, a.e0, a.ep, a.accept, a.e, s, ds, a.indp, blk, a.field, a.scale)); break;
        case StageA::ElementFromU: if (!fix_side) FEP_TRY(element_from_u()); break;
        case StageA::ElementFromDs: FEP_TRY(element_from_ds()); break;
#ifdef FEP_ABLATION
        case StageA::GenPoint: FEP_TRY(launch_point(c, st, a.u, a.e0, a.ep, a.accept, a.e, s, ds, a.indp, blk)); break;
#endif
        default: return FEP_ESTATE;
    }
#ifdef FEP_ABLATION
    if (fix_side) {
        HIP_TRY(hipEventRecord(ev_a, st));
        HIP_TRY(hipStreamWaitEvent(side, ev_a, 0));
        ms = side;
    }
#endif
    FEP_TRY(prof_mark(c, ms));
    if (p.elem_assembly) FEP_TRY(element_from_ds());
    switch (p.b) {
        case StageB::None: break;
        case StageB::OneKernel: FEP_TRY(launch_p1_fused(c, c->p1, st, a.u, a.e0, a.ep, a.e, a.s, a.ds, a.indp, a.K, a.F, cnt_b)); break;
        case StageB::Tile: case StageB::Direct: case StageB::FromNodes:
            FEP_TRY(launch_p1_node(c, c->p1, ms, p.b, ds, s, a.K, a.F, n_counts, cnt_b)); break;
        case StageB::Fixup: FEP_TRY(launch_fixup(c, c->patch, ms, a.K, a.F, n_counts, cnt_b)); break;
        case StageB::ReducePk: case StageB::Reduce: FEP_TRY(launch_reduce(c, c->coo, ms, p.b, a.K, a.F, n_counts, cnt_b)); break;
#ifdef FEP_ABLATION
        case StageB::GenNode: FEP_TRY(launch_gn_node(c, *c->gen, ms, ds, s, a.K, a.F, n_counts, cnt_b)); break;
#endif
        default: return FEP_ESTATE;
    }
    FEP_TRY(prof_mark(c, ms));
    if (p.force_gather) FEP_TRY(launch_force(c, c->coo, ms, a.F));
    FEP_TRY(prof_mark(c, ms));
#ifdef FEP_ABLATION
    if (fix_side) {
        HIP_TRY(hipEventRecord(ev_b, side));
        FEP_TRY(element_from_u());
        HIP_TRY(hipStreamWaitEvent(st, ev_b, 0));
    }
#endif
    if (p.sum == CountSum::Reduce) {
        hipLaunchKernelGGL(counts_reduce_kernel, dim3(1), dim3(1024), 0, st, n_counts, c->blk_counts, a.cnt);
        HIP_TRY(hipGetLastError());
    }
    return FEP_OK;
}

// One step: validate, plan, ensure the plan's scratch, run.  `field_d`: fep_step_field_dev
static int step_dev_impl(fep_ctx* c, void* stream, const double* u_d, const double* e0_h, const double* field_d, double scale,
                         double* ep_prev_d, int accept, double* e_out_d, double* s_d, double* ds_d, uint8_t* ind_p_d,
                         double* k_data_d, double* f_out_d, int64_t* counts_d) {
    if (!fep_aligned16(u_d) || !fep_aligned16(f_out_d) || !fep_aligned16(k_data_d)) return FEP_EINVAL;
    if (!c->have_materials) return FEP_ESTATE;
    if (field_d && c->route == Route::GenNode) return FEP_ESTATE;
    FEP_TRY(fep_set_device(c->device));
    hipStream_t st = (hipStream_t)stream;
    const fep_plan::StepWants w{accept != 0, e_out_d != nullptr, s_d != nullptr, ds_d != nullptr, ind_p_d != nullptr,
                                k_data_d != nullptr, f_out_d != nullptr, counts_d != nullptr, field_d != nullptr, false};
    const StepPlan plan = fep_plan::plan_step(facts_of(c), w);
    FEP_TRY(ensure_scratch(c, st, plan.need));
    return run_step(c, st, plan, StepArgs{u_d, make_e0(e0_h), ep_prev_d, accept, e_out_d, s_d, ds_d, ind_p_d, k_data_d, f_out_d,
                                          (unsigned long long*)counts_d, field_d, scale});
}

extern "C" int fep_step_dev(fep_ctx* c, void* stream, const double* u_d, const double* e0_h,
                            double* ep_prev_d, int accept, double* e_out_d, double* s_d, double* ds_d,
                            uint8_t* ind_p_d, double* k_data_d, double* f_out_d, int64_t* counts_d) {
    if (!c || !u_d) return FEP_EINVAL;
    return step_dev_impl(c, stream, u_d, e0_h, nullptr, 0.0, ep_prev_d, accept, e_out_d, s_d, ds_d, ind_p_d, k_data_d, f_out_d, counts_d);
}

extern "C" int fep_step_field_dev(fep_ctx* c, void* stream, const double* u_d, const double* e0_h,
                                  const double* e0_field_d, double e0_scale,
                                  double* ep_prev_d, int accept, double* e_out_d, double* s_d, double* ds_d,
                                  uint8_t* ind_p_d, double* k_data_d, double* f_out_d, int64_t* counts_d) {
    if (!c || !u_d || !e0_field_d) return FEP_EINVAL;
    return step_dev_impl(c, stream, u_d, e0_h, e0_field_d, e0_scale, ep_prev_d, accept, e_out_d, s_d, ds_d, ind_p_d, k_data_d,
                         f_out_d, counts_d);
}

extern "C" int fep_assemble_dev(fep_ctx* c, void* stream, const double* ds_d, const double* s_d,
                                double* k_data_d, double* f_out_d) {
    if (!c) return FEP_EINVAL;
    if ((k_data_d && !ds_d) || (f_out_d && !s_d)) return FEP_EINVAL;
    if (!fep_aligned16(f_out_d) || !fep_aligned16(k_data_d)) return FEP_EINVAL;
    FEP_TRY(fep_set_device(c->device));
    hipStream_t st = (hipStream_t)stream;
    fep_plan::StepWants w;
    w.K = k_data_d != nullptr; w.F = f_out_d != nullptr; w.assemble = true;
    const StepPlan plan = fep_plan::plan_step(facts_of(c), w);
    FEP_TRY(ensure_scratch(c, st, plan.need));
    return run_step(c, st, plan, StepArgs{nullptr, make_e0(nullptr), nullptr, 0, nullptr, const_cast<double*>(s_d),
                                          const_cast<double*>(ds_d), nullptr, k_data_d, f_out_d, nullptr, nullptr, 0.0});
}

static int step_host_impl(fep_ctx* c, bool u_planar, const double* u_h, const double* e0_h, double* ep_prev_h, int accept,
                          double* e_out_h, double* s_h, double* ds_h, uint8_t* ind_p_h,
                          double* k_data_h, double* f_out_h, int64_t* counts_h,
                          const double* field_h = nullptr, double scale = 0.0) {
    if (!c || !u_h) return FEP_EINVAL;
    fep_stage::HostCall call(c->device, &c->hbuf);
    const size_t n = (size_t)c->n_int, n_dof = (size_t)c->n_dof;
    const double* u = u_planar ? call.in_interleave2(kBufU, u_h, (size_t)c->n_n) : call.in(kBufU, u_h, n_dof);
    double* ep = call.inout(kBufEp, ep_prev_h, 4 * n, accept != 0);
    const double* fld = call.in(kBufField, field_h, 4 * n);
    // copied back in this order: the largest result first, its transfer hides the others' set-up
    double *kd = call.out(kBufK, k_data_h, (size_t)c->nnz), *f = call.out(kBufF, f_out_h, n_dof);
    double *ds = call.out(kBufDs, ds_h, 9 * n), *s = call.out(kBufS, s_h, 4 * n), *eo = call.out(kBufE, e_out_h, 3 * n);
    uint8_t* ip = call.out(kBufIndP, ind_p_h, n);
    int64_t* cnt = call.scratch<int64_t>(kBufCounts, 2);    // the kernels always count; copied back only if asked for
    call.out(kBufCounts, counts_h, 2);
    return call.run([&] {
        return field_h ? fep_step_field_dev(c, call.stream(), u, e0_h, fld, scale, ep, accept, eo, s, ds, ip, kd, f, cnt)
                       : fep_step_dev(c, call.stream(), u, e0_h, ep, accept, eo, s, ds, ip, kd, f, cnt);
    });
}

extern "C" int fep_step_host(fep_ctx* c, const double* u_h, const double* e0_h, double* ep_prev_h, int accept,
                             double* e_out_h, double* s_h, double* ds_h, uint8_t* ind_p_h,
                             double* k_data_h, double* f_out_h, int64_t* counts_h) {
    FEP_GUARD(step_host_impl(c, false, u_h, e0_h, ep_prev_h, accept, e_out_h, s_h, ds_h, ind_p_h, k_data_h, f_out_h, counts_h))
}

extern "C" int fep_step_field_host(fep_ctx* c, const double* u_h, const double* e0_h, const double* e0_field_h, double e0_scale,
                                   double* ep_prev_h, int accept, double* e_out_h, double* s_h, double* ds_h, uint8_t* ind_p_h,
                                   double* k_data_h, double* f_out_h, int64_t* counts_h) {
    if (!e0_field_h) return FEP_EINVAL;
    FEP_GUARD(step_host_impl(c, false, u_h, e0_h, ep_prev_h, accept, e_out_h, s_h, ds_h, ind_p_h, k_data_h, f_out_h, counts_h,
                             e0_field_h, e0_scale))
}

extern "C" int fep_step_host_planar(fep_ctx* c, const double* u2_h, const double* e0_h, double* ep_prev_h, int accept,
                                    double* e_out_h, double* s_h, double* ds_h, uint8_t* ind_p_h,
                                    double* k_data_h, double* f_out_h, int64_t* counts_h) {
    FEP_GUARD(step_host_impl(c, true, u2_h, e0_h, ep_prev_h, accept, e_out_h, s_h, ds_h, ind_p_h, k_data_h, f_out_h, counts_h))
}

static int assemble_host_impl(fep_ctx* c, const double* ds_h, const double* s_h, double* k_data_h, double* f_out_h) {
    if (!c) return FEP_EINVAL;
    if ((k_data_h && !ds_h) || (f_out_h && !s_h)) return FEP_EINVAL;
    fep_stage::HostCall call(c->device, &c->hbuf);
    const size_t n = (size_t)c->n_int;
    const double *ds = call.in(kBufDs, ds_h, 9 * n), *s = call.in(kBufS, s_h, 3 * n);     // (s: 3 n_int into the 4 n_int block)
    double *kd = call.out(kBufK, k_data_h, (size_t)c->nnz), *f = call.out(kBufF, f_out_h, (size_t)c->n_dof);
    return call.run([&] { return fep_assemble_dev(c, call.stream(), ds, s, kd, f); });
}

extern "C" int fep_assemble_host(fep_ctx* c, const double* ds_h, const double* s_h, double* k_data_h, double* f_out_h) {
    FEP_GUARD(assemble_host_impl(c, ds_h, s_h, k_data_h, f_out_h))
}

extern "C" int fep_gather_f64(int device_id, void* stream, int64_t n, const double* src_d, const int32_t* idx_d, double* dst_d) {
    if (n < 0 || (n > 0 && (!src_d || !idx_d || !dst_d))) return FEP_EINVAL;
    FEP_TRY(fep_set_device(device_id));
    if (n == 0) return FEP_OK;
    hipLaunchKernelGGL(gather_or_zero_kernel, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, n, src_d, idx_d, dst_d);
    HIP_TRY(hipGetLastError());
    return FEP_OK;
}

extern "C" int fep_scatter_f64(int device_id, void* stream, int64_t n, const double* src_d, const int32_t* src_idx_d,
                               const int32_t* dst_idx_d, double* dst_d) {
    if (n < 0 || (n > 0 && (!src_d || !src_idx_d || !dst_idx_d || !dst_d))) return FEP_EINVAL;
    FEP_TRY(fep_set_device(device_id));
    if (n == 0) return FEP_OK;
    hipLaunchKernelGGL(scatter_kernel, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, n, src_d, src_idx_d,
                       dst_idx_d, dst_d);
    HIP_TRY(hipGetLastError());
    return FEP_OK;
}

extern "C" int fep_iface_sum_f64(int device_id, void* stream, int64_t n, const int32_t* loc_d, const int32_t* ptr_d,
                                 const int32_t* src_d, const double* recv_d, double* f_d) {
    if (n < 0 || (n > 0 && (!loc_d || !ptr_d || !src_d || !f_d))) return FEP_EINVAL;
    FEP_TRY(fep_set_device(device_id));
    if (n == 0) return FEP_OK;
    hipLaunchKernelGGL(iface_sum_kernel, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, n, loc_d, ptr_d, src_d,
                       recv_d, f_d);
    HIP_TRY(hipGetLastError());
    return FEP_OK;
}

extern "C" int fep_csr_merge_f64(int device_id, void* stream, int64_t n_blocks, const int32_t* first_d, const int32_t* multi_ptr_d,
                                 const int32_t* multi_src_d, const double* recv_d, double* k_global_d) {
    if (n_blocks < 0 || (n_blocks > 0 && (!first_d || !multi_ptr_d || !recv_d || !k_global_d))) return FEP_EINVAL;
    if ((((uintptr_t)recv_d) | ((uintptr_t)k_global_d)) & 15) return FEP_EINVAL;      // pairs move as 16-byte words
    if (n_blocks >= (int64_t)INT32_MAX / 4) return FEP_ERANGE;
    FEP_TRY(fep_set_device(device_id));
    if (n_blocks == 0) return FEP_OK;
    hipLaunchKernelGGL(csr_merge_kernel, dim3(grid_for(2 * n_blocks, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, 2 * n_blocks,
                       first_d, multi_ptr_d, multi_src_d, (const double2*)recv_d, (double2*)k_global_d);
    HIP_TRY(hipGetLastError());
    return FEP_OK;
}

extern "C" int fep_transform_dev(fep_ctx* c, void* stream, const double* q_int_d, double* q_node_d) {
    if (!c || !q_int_d || !q_node_d) return FEP_EINVAL;
    FEP_TRY(fep_set_device(c->device));
    hipLaunchKernelGGL(nodal_average_kernel, dim3(grid_for(c->n_n, kBlock)), dim3(kBlock), 0, (hipStream_t)stream,
                       c->n_n, c->n_e, c->n_q, c->iptr, c->ilist, c->weight, q_int_d, q_node_d);
    HIP_TRY(hipGetLastError());
    return FEP_OK;
}

static int transform_host_impl(fep_ctx* c, const double* q_int_h, double* q_node_h) {
    if (!c || !q_int_h || !q_node_h) return FEP_EINVAL;
    fep_stage::HostCall call(c->device, &c->hbuf);
    const double* q = call.in(kBufQ, q_int_h, (size_t)c->n_int);
    double* o = call.out(kBufNode, q_node_h, (size_t)c->n_n);
    return call.run([&] { return fep_transform_dev(c, call.stream(), q, o); });
}

extern "C" int fep_transform_host(fep_ctx* c, const double* q_int_h, double* q_node_h) {
    FEP_GUARD(transform_host_impl(c, q_int_h, q_node_h))
}

// ---- external loads (EL:246-364) ----
extern "C" int fep_load_volume_dev(fep_ctx* c, void* stream, const double* hatp_h, const double* f_v_d, double fx, double fy,
                                   const double* weight_d, double* f_out_d) {
    if (!c || !hatp_h || !f_out_d) return FEP_EINVAL;
    if (!fep_aligned16(f_out_d)) return FEP_EINVAL;
    if (c->n_p * c->n_q > kLoadTabMax) return FEP_EINVAL;
    FEP_TRY(fep_set_device(c->device));
    if (c->n_n == 0) return FEP_OK;
    LoadTab tab{};                                      // travels as a kernel argument: nothing to copy, capturable
    for (int i = 0; i < c->n_p * c->n_q; ++i) tab.h[i] = hatp_h[i];
    const double* w = weight_d ? weight_d : c->weight;
    const dim3 grid(grid_for(c->n_n, kBlock)), block(kBlock);
    if (f_v_d)
        hipLaunchKernelGGL(load_volume_kernel<true>, grid, block, 0, (hipStream_t)stream, c->n_n, c->n_e, c->n_p, c->n_q,
                           c->iptr, c->ilist, w, f_v_d, 0.0, 0.0, tab, f_out_d);
    else
        hipLaunchKernelGGL(load_volume_kernel<false>, grid, block, 0, (hipStream_t)stream, c->n_n, c->n_e, c->n_p, c->n_q,
                           c->iptr, c->ilist, w, (const double*)nullptr, fx, fy, tab, f_out_d);
    HIP_TRY(hipGetLastError());
    return FEP_OK;
}

static int load_volume_host_impl(fep_ctx* c, const double* hatp_h, const double* f_v_h, double fx, double fy,
                                 const double* weight_h, double* f_out_h) {
    if (!c || !hatp_h || !f_out_h) return FEP_EINVAL;
    fep_stage::HostCall call(c->device, &c->hbuf);
    const size_t n = (size_t)c->n_int;
    const double *f = call.in(kBufFv, f_v_h, 2 * n), *w = call.in(kBufWeight, weight_h, n);
    double* o = call.out(kBufLoad, f_out_h, (size_t)c->n_dof);
    return call.run([&] { return fep_load_volume_dev(c, call.stream(), hatp_h, f, fx, fy, w, o); });
}

extern "C" int fep_load_volume_host(fep_ctx* c, const double* hatp_h, const double* f_v_h, double fx, double fy,
                                    const double* weight_h, double* f_out_h) {
    FEP_GUARD(load_volume_host_impl(c, hatp_h, f_v_h, fx, fy, weight_h, f_out_h))
}

// Coordinates of the integration points (fep.h): point_coords_kernel, the table as a kernel argument
extern "C" int fep_ctx_point_coords_dev(fep_ctx* c, void* stream, const double* hatp_h, double* xq_d) {
    if (!c || !hatp_h || !xq_d) return FEP_EINVAL;
    if (c->n_p * c->n_q > kLoadTabMax) return FEP_EINVAL;
    FEP_TRY(fep_set_device(c->device));
    if (c->n_int == 0) return FEP_OK;
    LoadTab tab{};
    for (int i = 0; i < c->n_p * c->n_q; ++i) tab.h[i] = hatp_h[i];
    hipLaunchKernelGGL(point_coords_kernel, dim3(grid_for(c->n_int, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, c->n_e,
                       c->n_n, c->n_p, c->n_q, c->elem, c->coords, tab, xq_d);
    HIP_TRY(hipGetLastError());
    return FEP_OK;
}

static int point_coords_host_impl(fep_ctx* c, const double* hatp_h, double* xq_h) {
    if (!c || !hatp_h || !xq_h) return FEP_EINVAL;
    fep_stage::HostCall call(c->device, &c->hbuf);
    double* o = call.out(kBufXq, xq_h, 2 * (size_t)c->n_int);
    return call.run([&] { return fep_ctx_point_coords_dev(c, call.stream(), hatp_h, o); });
}

extern "C" int fep_ctx_point_coords_host(fep_ctx* c, const double* hatp_h, double* xq_h) {
    FEP_GUARD(point_coords_host_impl(c, hatp_h, xq_h))
}

// ---- recovered-stress error indicator (fep.h): recover_stress_kernel, estimate_kernel; the statistics are fep_mesh.hip's ----
extern "C" int fep_recover_stress_dev(fep_ctx* c, void* stream, const double* s_d, double* s_node_d) {
    if (!c || !s_d || !s_node_d) return FEP_EINVAL;
    FEP_TRY(fep_set_device(c->device));
    if (c->n_n == 0) return FEP_OK;
    hipLaunchKernelGGL(recover_stress_kernel, dim3(grid_for(c->n_n, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, c->n_n, c->n_e,
                       c->n_q, c->iptr, c->ilist, c->weight, s_d, s_node_d);
    HIP_TRY(hipGetLastError());
    return FEP_OK;
}

extern "C" int fep_estimate_dev(fep_ctx* c, void* stream, const double* hatp_h, const double* s_d, const double* s_node_d,
                                double* eta2_d, double* stats_d) {
    if (!c || !s_d || !s_node_d || !eta2_d) return FEP_EINVAL;
    if (c->elem_type != FEP_P1 && !hatp_h) return FEP_EINVAL;
    if (!c->have_materials) return FEP_ESTATE;
    FEP_TRY(fep_set_device(c->device));
    hipStream_t st = (hipStream_t)stream;
    if (stats_d) FEP_TRY(fep_indicator_reserve(c->device, st, c->n_e));
    LoadTab tab{};                                      // travels as a kernel argument, as in fep_load_volume_dev
    if (c->elem_type != FEP_P1)
        for (int i = 0; i < c->n_p * c->n_q; ++i) tab.h[i] = hatp_h[i];
    FEP_TRY(with_type(c->elem_type, [&](auto et) {
        using E = decltype(et);
        hipLaunchKernelGGL((estimate_kernel<E::NP, E::NQ>), dim3(grid_for(c->n_e, kBlock)), dim3(kBlock), 0, st, c->n_e, c->n_n,
                           c->elem, c->weight, c->shear, c->bulk, c->matu, tab, s_d, s_node_d, eta2_d);
        HIP_TRY(hipGetLastError());
        return FEP_OK;
    }));
    if (stats_d) FEP_TRY(fep_indicator_stats(c->device, st, c->n_e, eta2_d, stats_d));
    return FEP_OK;
}

static int recover_stress_host_impl(fep_ctx* c, const double* s_h, double* s_node_h) {
    if (!c || !s_h || !s_node_h) return FEP_EINVAL;
    fep_stage::HostCall call(c->device, &c->hbuf);
    const double* s = call.in(kBufS, s_h, 4 * (size_t)c->n_int);
    double* o = call.out(kBufSNode, s_node_h, 4 * (size_t)c->n_n);
    return call.run([&] { return fep_recover_stress_dev(c, call.stream(), s, o); });
}

extern "C" int fep_recover_stress_host(fep_ctx* c, const double* s_h, double* s_node_h) {
    FEP_GUARD(recover_stress_host_impl(c, s_h, s_node_h))
}

static int estimate_host_impl(fep_ctx* c, const double* hatp_h, const double* s_h, const double* s_node_h, double* eta2_h,
                              double* stats_h) {
    if (!c || !s_h || !s_node_h || !eta2_h) return FEP_EINVAL;
    if (c->elem_type != FEP_P1 && !hatp_h) return FEP_EINVAL;
    if (!c->have_materials) return FEP_ESTATE;
    fep_stage::HostCall call(c->device, &c->hbuf);
    const double *s = call.in(kBufS, s_h, 4 * (size_t)c->n_int), *sn = call.in(kBufSNode, s_node_h, 4 * (size_t)c->n_n);
    double *o = call.out(kBufEta2, eta2_h, (size_t)c->n_e), *st = call.out(kBufStats, stats_h, 4);
    return call.run([&] { return fep_estimate_dev(c, call.stream(), hatp_h, s, sn, o, st); });
}

extern "C" int fep_estimate_host(fep_ctx* c, const double* hatp_h, const double* s_h, const double* s_node_h, double* eta2_h,
                                 double* stats_h) {
    FEP_GUARD(estimate_host_impl(c, hatp_h, s_h, s_node_h, eta2_h, stats_h))
}

// Incidence of the loaded nodes, built per call (n_e_s is of the order of sqrt(n_e)), packed with the edge table into one
// int32 upload: [edges | bnode | bptr | blist].
static int load_traction_impl(int device_id, void* stream, int64_t n_n, int64_t n_e_s, int n_p_s, int n_q_s,
                              const int32_t* edges_h, const double* xy, bool xy_on_host, const double* hatp_s_h,
                              const double* dhatp1_s_h, const double* wf_s_h, const double* t_int, bool t_on_host,
                              double* f_out, bool out_on_host) {
    if (n_n < 0 || n_e_s < 0 || n_p_s < 2 || n_p_s > kEdgeNodesMax || n_q_s < 1 || n_q_s > kEdgePointsMax) return FEP_EINVAL;
    if (!f_out && n_n > 0) return FEP_EINVAL;
    if (n_e_s > 0 && (!edges_h || !xy || !hatp_s_h || !dhatp1_s_h || !wf_s_h || !t_int)) return FEP_EINVAL;
    if (!out_on_host && !fep_aligned16(f_out)) return FEP_EINVAL;
    const int64_t n_inc = (int64_t)n_p_s * n_e_s;
    if (n_inc * (int64_t)kEdgePointsMax >= (int64_t)INT32_MAX / 4) return FEP_ERANGE;
    for (int64_t i = 0; i < n_inc; ++i)
        if (edges_h[i] < 0 || edges_h[i] >= n_n) return FEP_ERANGE;
    FEP_TRY(fep_set_device(device_id));
    if (n_n == 0) return FEP_OK;
    hipStream_t st = (hipStream_t)stream;
    // loaded nodes in ascending id, each with its (edge, local node) codes ordered by (e, a)
    std::vector<int32_t> bnode(edges_h, edges_h + n_inc);
    std::sort(bnode.begin(), bnode.end());
    bnode.erase(std::unique(bnode.begin(), bnode.end()), bnode.end());
    const int64_t n_b = (int64_t)bnode.size();
    std::vector<int32_t> pack((size_t)(2 * n_inc + 2 * n_b + 1), 0);
    int32_t* P_edges = pack.data();
    int32_t* P_bnode = P_edges + n_inc;
    int32_t* P_bptr = P_bnode + n_b;
    int32_t* P_blist = P_bptr + n_b + 1;
    auto slot = [&](int32_t nd) { return (int64_t)(std::lower_bound(bnode.begin(), bnode.end(), nd) - bnode.begin()); };
    for (int64_t i = 0; i < n_inc; ++i) { P_edges[i] = edges_h[i]; P_bptr[slot(edges_h[i]) + 1]++; }
    for (int64_t b = 0; b < n_b; ++b) { P_bnode[b] = bnode[b]; P_bptr[b + 1] += P_bptr[b]; }
    {
        std::vector<int32_t> fill(P_bptr, P_bptr + n_b);
        for (int64_t e = 0; e < n_e_s; ++e)
            for (int a = 0; a < n_p_s; ++a) P_blist[fill[slot(edges_h[(int64_t)a * n_e_s + e])]++] = (int32_t)((int64_t)a * n_e_s + e);
    }
    EdgeTab tab{};
    for (int i = 0; i < n_p_s * n_q_s; ++i) { tab.h[i] = hatp_s_h[i]; tab.dh[i] = dhatp1_s_h[i]; }
    for (int q = 0; q < n_q_s; ++q) tab.wf[q] = wf_s_h[q];
    // device scratch of this call: released on every exit
    struct Scratch {
        std::vector<void*> p;
        ~Scratch() { for (void* q : p) (void)hipFree(q); }
        int get(void** out, size_t bytes) {
            HIP_TRY(hipMalloc(out, bytes ? bytes : 1));
            p.push_back(*out);
            return FEP_OK;
        }
    } scratch;
    const size_t n_pts = (size_t)(n_e_s * n_q_s);
    void *d_pack = nullptr, *d_xy = (void*)xy, *d_t = (void*)t_int, *d_out = (void*)f_out;
    FEP_TRY(scratch.get(&d_pack, pack.size() * sizeof(int32_t)));
    HIP_TRY(hipMemcpyAsync(d_pack, pack.data(), pack.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if (xy_on_host && n_e_s > 0) {
        FEP_TRY(scratch.get(&d_xy, 2 * (size_t)n_n * sizeof(double)));
        HIP_TRY(hipMemcpyAsync(d_xy, xy, 2 * (size_t)n_n * sizeof(double), hipMemcpyHostToDevice, st));
    }
    if (t_on_host && n_e_s > 0) {
        FEP_TRY(scratch.get(&d_t, 2 * n_pts * sizeof(double)));
        HIP_TRY(hipMemcpyAsync(d_t, t_int, 2 * n_pts * sizeof(double), hipMemcpyHostToDevice, st));
    }
    if (out_on_host) FEP_TRY(scratch.get(&d_out, 2 * (size_t)n_n * sizeof(double)));
    HIP_TRY(hipMemsetAsync(d_out, 0, 2 * (size_t)n_n * sizeof(double), st));
    if (n_b > 0) {
        const int32_t* dp = (const int32_t*)d_pack;
        hipLaunchKernelGGL(load_traction_kernel, dim3(grid_for(n_b, kBlock)), dim3(kBlock), 0, st, (int)n_b, n_n, n_e_s, n_p_s,
                           n_q_s, dp, dp + n_inc, dp + n_inc + n_b, dp + n_inc + 2 * n_b + 1, (const double*)d_xy,
                           (const double*)d_t, tab, (double*)d_out);
        HIP_TRY(hipGetLastError());
    }
    if (out_on_host) HIP_TRY(hipMemcpyAsync(f_out, d_out, 2 * (size_t)n_n * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));                  // the scratch above is freed on return
    return FEP_OK;
}

extern "C" int fep_load_traction_dev(int device_id, void* stream, int64_t n_n, int64_t n_e_s, int n_p_s, int n_q_s,
                                     const int32_t* edges_h, const double* xy_d, const double* hatp_s_h,
                                     const double* dhatp1_s_h, const double* wf_s_h, const double* t_int_d, double* f_out_d) {
    FEP_GUARD(load_traction_impl(device_id, stream, n_n, n_e_s, n_p_s, n_q_s, edges_h, xy_d, false, hatp_s_h, dhatp1_s_h, wf_s_h,
                                 t_int_d, false, f_out_d, false))
}

extern "C" int fep_load_traction_host(int device_id, int64_t n_n, int64_t n_e_s, int n_p_s, int n_q_s,
                                      const int32_t* edges_h, const double* xy_h, const double* hatp_s_h,
                                      const double* dhatp1_s_h, const double* wf_s_h, const double* t_int_h, double* f_out_h) {
    FEP_GUARD(load_traction_impl(device_id, nullptr, n_n, n_e_s, n_p_s, n_q_s, edges_h, xy_h, true, hatp_s_h, dhatp1_s_h, wf_s_h,
                                 t_int_h, true, f_out_h, true))
}

// The kernels of a step, named as rocprofv3 prints them (bench.py labels its roofline with these and checks them against the
// kernel names of the recorded counter passes): the stages of the plan of a non-accepting step that wants every output
// (which = 0) or K and F alone (1), without the counter sum
extern "C" int fep_ctx_kernel_names(const fep_ctx* c, int which, char* buf, int64_t cap) {
    if (!c || !buf || cap <= 0 || (which != 0 && which != 1)) return FEP_EINVAL;
    fep_plan::StepWants w;
    w.K = w.F = true;
    w.e = w.s = w.ds = w.ind_p = which == 0;
    const StepPlan p = fep_plan::plan_step(facts_of(c), w);
    Names o;
    switch (p.a) {
        case StageA::None: break;
        case StageA::Point: FEP_TRY(name_point_stage(c, o)); break;
        case StageA::ElementFromU: name_element(c, c->elem_form, true, o); break;
        case StageA::ElementFromDs: name_element(c, c->elem_form, false, o); break;
#ifdef FEP_ABLATION
        case StageA::GenPoint: name_point(c, o); break;
#endif
        default: return FEP_ESTATE;
    }
    if (p.elem_assembly) name_element(c, c->elem_form, false, o);
    switch (p.b) {
        case StageB::None: break;
        case StageB::OneKernel: name_p1_fused(c->p1, which == 0, o); break;
        case StageB::Tile: case StageB::Direct: case StageB::FromNodes: name_p1_node(c->p1, p.b, o); break;
        case StageB::Fixup: o.add("%s", "fixup_kernel"); break;
        case StageB::ReducePk: case StageB::Reduce: name_reduce(c->coo, p.b, o); break;
#ifdef FEP_ABLATION
        case StageB::GenNode: name_gn_node(c, *c->gen, o); break;
#endif
        default: return FEP_ESTATE;
    }
    if (p.force_gather) o.add("%s", "force_reduce_kernel");
    std::snprintf(buf, (size_t)cap, "%s", o.s);
    return FEP_OK;
}

extern "C" int fep_ctx_profile_begin(fep_ctx* c) {
    if (!c) return FEP_EINVAL;
    for (hipEvent_t ev : c->events) (void)hipEventDestroy(ev);
    c->events.clear();
    c->profiling = true;
    return FEP_OK;
}

extern "C" int fep_ctx_profile_end(fep_ctx* c, void* stream, double ms_out[3], int* n_steps) {
    if (!c || !ms_out) return FEP_EINVAL;
    c->profiling = false;
    FEP_TRY(fep_set_device(c->device));
    hipError_t e = hipStreamSynchronize((hipStream_t)stream);
    double acc[3] = {0.0, 0.0, 0.0};
    const int n = (int)(c->events.size() / 4);
    for (int s = 0; s < n && e == hipSuccess; ++s)
        for (int k = 0; k < 3 && e == hipSuccess; ++k) {
            float ms = 0.f;
            e = hipEventElapsedTime(&ms, c->events[4 * s + k], c->events[4 * s + k + 1]);
            acc[k] += ms;
        }
    for (hipEvent_t ev : c->events) (void)hipEventDestroy(ev);
    c->events.clear();
    if (e != hipSuccess) { g_last_hip = (int)e; (void)hipGetLastError(); return FEP_EHIP; }
    for (int k = 0; k < 3; ++k) ms_out[k] = n ? acc[k] / n : 0.0;
    if (n_steps) *n_steps = n;
    return FEP_OK;
}
