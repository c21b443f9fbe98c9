// pamg_host.h — what the host-side units of the device runtime (runtime.hip, matrix.hip) share:
// the status-checking macros, the vector padding, and device allocation / zeroing.
#pragma once

#include <cstddef>
#include <cstdint>

#include "pamg_device.h"

using pamg::fail;

#define HIPC(expr)                                                                    \
    do {                                                                              \
        hipError_t e_ = (expr);                                                       \
        if (e_ != hipSuccess)                                                         \
            return fail(PAMG_E_HIP, "%s:%d %s: %s", __FILE__, __LINE__, #expr,        \
                        hipGetErrorString(e_));                                       \
    } while (0)

#define NCCLC(expr)                                                                   \
    do {                                                                              \
        ncclResult_t r_ = (expr);                                                     \
        if (r_ != ncclSuccess)                                                        \
            return fail(PAMG_E_RCCL, "%s:%d %s: %s", __FILE__, __LINE__, #expr,       \
                        ncclGetErrorString(r_));                                      \
    } while (0)

#define CHECK(expr)                   \
    do {                              \
        int rc_ = (expr);             \
        if (rc_ != PAMG_OK) return rc_; \
    } while (0)

constexpr int kVecPad = 8;  // trailing doubles so 16-byte vector loads never run off the end

template <class T>
int dalloc(T** p, int64_t n) {
    *p = nullptr;
    if (n <= 0) return PAMG_OK;
    HIPC(hipMalloc(reinterpret_cast<void**>(p), sizeof(T) * (size_t)n));
    return PAMG_OK;
}

template <class T>
void dfree(T*& p) {
    if (p) (void)hipFree(p);
    p = nullptr;
}

inline int set_device(const pamg_ctx* ctx) {
    HIPC(hipSetDevice(ctx->device));
    return PAMG_OK;
}

// Zero device memory in the context's stream order and wait for it: hipMemset runs on the
// null stream, which the context's non-blocking streams do not wait for, so a kernel enqueued
// right after it could run first (found in round 5: PCG's first initial residual raced with the
// zeroing of its freshly allocated vectors).
inline int dzero(pamg_ctx* ctx, void* p, size_t bytes) {
    HIPC(hipMemsetAsync(p, 0, bytes, ctx->s_comp));
    HIPC(hipStreamSynchronize(ctx->s_comp));
    return PAMG_OK;
}
