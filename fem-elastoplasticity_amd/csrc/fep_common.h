// Shared by the translation units of libfep_hip.so: error plumbing of the C ABI (include/fep.h).
#pragma once
#include <hip/hip_runtime.h>
#include <new>

#include "../../include/fep.h"

extern __attribute__((visibility("hidden"))) thread_local int fep_g_last_hip;   // last failing hipError_t of this host thread (fep_last_hip_error)

#define HIP_TRY(expr)                                   \
    do {                                                \
        hipError_t _e = (expr);                         \
        if (_e != hipSuccess) {                         \
            fep_g_last_hip = (int)_e;                   \
            (void)hipGetLastError();                    \
            return _e == hipErrorOutOfMemory ? FEP_ENOMEM : FEP_EHIP; \
        }                                               \
    } while (0)
#define FEP_TRY(expr)                  \
    do {                               \
        int _r = (expr);               \
        if (_r != FEP_OK) return _r;   \
    } while (0)
// Body of an extern "C" entry point: nothing may leave it by exception
#define FEP_GUARD(call) \
    try { return call; } catch (const std::bad_alloc&) { return FEP_ENOMEM; } catch (...) { return FEP_EINVAL; }

__attribute__((visibility("hidden"))) int fep_set_device(int dev);
// fep_mesh.hip, for fep_estimate_dev: the statistics {total, max, non-finite, n} of an indicator array, enqueued on `st`;
// _reserve makes sure of their scratch beforehand (FEP_ESTATE if it would have to grow during a capture)
__attribute__((visibility("hidden"))) int fep_indicator_reserve(int device, hipStream_t st, int64_t n);
__attribute__((visibility("hidden"))) int fep_indicator_stats(int device, hipStream_t st, int64_t n, const double* eta2_d, double* stats_d);

#include <stdint.h>
static inline bool fep_aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }   // NULL counts as aligned              // hipSetDevice with range check -> FEP_ENODEV


// Measurement switches (variant selection by environment variable, per-phase clocks, ...) exist only in builds made with
// -DFEP_ABLATION (`python fem-elastoplasticity_amd/build.py --ablation` -> csrc/libfep_hip_abl.so, used through
// FEP_LIB_PATH by tools/).  The product library is built without it: fep_tune() is then a constant NULL, every branch on
// it folds away and the variants behind it are not instantiated.
#include <cstdlib>
#ifdef FEP_ABLATION
static inline const char* fep_tune(const char* name) { return std::getenv(name); }
#else
static constexpr const char* fep_tune(const char*) { return nullptr; }
#endif
