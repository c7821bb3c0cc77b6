// What the host code around the kernels shares: the buffers a handle owns, the error macros, and the steps of the lifecycle that
// every handle of the read-mapping chain follows (kmx_vote.hip, kmx_align.hip, kmx_script.hip, kmx_strands.hip, kmx_pairs.hip, kmx_rescue.hip,
// kmx_tags.hip, kmx_contigs.hip, kmx_secondary.hip, kmx_clip.hip, kmx_supplementary.hip, kmx_realign.hip).
// A chain handle has the members `device`, `release()` (its buffers go, on its device) and `clear()` (an empty result).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "kmx_types.h"

namespace kmx {

kmx_status set_error(kmx_status st, const std::string& msg);    // kmx_capi.hip: kmx_last_error's message

// a HIP call that failed ends the function: the sticky error is cleared, the text names the call
#define TRY_HIP(expr)                                                                                  \
    do {                                                                                               \
        hipError_t e__ = (expr);                                                                       \
        if (e__ != hipSuccess) {                                                                       \
            (void)hipGetLastError();                                                                   \
            return kmx::set_error(e__ == hipErrorOutOfMemory ? KMX_ERR_OUT_OF_MEMORY : KMX_ERR_HIP,    \
                                  std::string(#expr) + ": " + hipGetErrorString(e__));                 \
        }                                                                                              \
    } while (0)
// ... and so does a step of ours that failed (it has set the error text)
#define TRY_KMX(expr) do { const kmx_status st__ = (expr); if (st__ != KMX_OK) return st__; } while (0)

// grow-only device buffer, released with its owner
struct Buf {
    void* p = nullptr;
    size_t cap = 0;
    Buf() = default;
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    hipError_t ensure(size_t bytes)
    {
        if (bytes <= cap) return hipSuccess;
        release();
        const size_t want = bytes + bytes / 8 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) { p = nullptr; return e; }
        cap = want;
        return hipSuccess;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    ~Buf() { release(); }
    template <typename T> T* as() const { return static_cast<T*>(p); }
};

// page-locked host array that keeps its contents when it grows; freed with its owner
struct PinnedArr {
    void* p = nullptr;
    size_t cap = 0;
    PinnedArr() = default;
    PinnedArr(const PinnedArr&) = delete;
    PinnedArr& operator=(const PinnedArr&) = delete;
    ~PinnedArr() { release(); }
    bool grow(size_t bytes)
    {
        if (bytes <= cap) return true;
        const size_t want = std::max(bytes, cap * 2) + 64;
        void* q = nullptr;
        if (hipHostMalloc(&q, want, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return false; }
        if (p) { std::memcpy(q, p, cap); (void)hipHostFree(p); }
        p = q; cap = want;
        return true;
    }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
    template <typename T> T* as() const { return static_cast<T*>(p); }
};

// the caller's current device, restored at scope exit (only if it could be read)
struct DeviceGuard {
    int cur = 0;
    const bool have = hipGetDevice(&cur) == hipSuccess;
    DeviceGuard() { if (!have) (void)hipGetLastError(); }
    DeviceGuard(const DeviceGuard&) = delete;
    ~DeviceGuard() { if (have) (void)hipSetDevice(cur); }
};

inline unsigned int grid_for(uint64_t n, uint64_t per_block) { return unsigned(std::max<uint64_t>((n + per_block - 1) / per_block, 1)); }

// `bytes` at d (counters, a total) into h, there when the call returns; fn: the entry point, for the text
inline kmx_status read_back(const char* fn, hipStream_t s, const void* d, PinnedArr& h, size_t bytes)
{
    if (!h.grow(bytes)) return set_error(KMX_ERR_OUT_OF_MEMORY, std::string(fn) + ": page-locked host allocation failed");
    TRY_HIP(hipMemcpyAsync(h.p, d, bytes, hipMemcpyDeviceToHost, s));
    TRY_HIP(hipStreamSynchronize(s));
    return KMX_OK;
}

// Host reads (ranks, roff[nr + 1]): what is wrong with them, or nullptr and *n_letters = their letters.
inline const char* check_host_reads(const void* ranks, const uint64_t* roff, uint64_t nr, uint64_t* n_letters)
{
    if (nr && roff[0] != 0) return "roff[0] must be 0";
    for (uint64_t i = 0; i < nr; ++i)
        if (roff[i + 1] < roff[i]) return "roff must be non-decreasing";
    *n_letters = nr ? roff[nr] : 0;
    if (*n_letters && !ranks) return "NULL read letters (ranks)";
    return nullptr;
}

// ... and their way to the device on stream s (the caller synchronises s before its own caller may touch the arrays again)
inline kmx_status upload_reads(const void* ranks, const void* roff, uint64_t nr, uint64_t n_letters, Buf& d_ranks, Buf& d_roff, hipStream_t s)
{
    TRY_HIP(d_ranks.ensure(std::max<uint64_t>(n_letters, 1)));
    TRY_HIP(d_roff.ensure((nr + 1) * 8));
    if (n_letters) TRY_HIP(hipMemcpyAsync(d_ranks.p, ranks, n_letters, hipMemcpyHostToDevice, s));
    TRY_HIP(hipMemcpyAsync(d_roff.p, roff, (nr + 1) * 8, hipMemcpyHostToDevice, s));
    return KMX_OK;
}

// *inout becomes a handle on `device` (created when NULL), and `device` the current one: the caller holds a DeviceGuard.
template <typename H>
kmx_status bind_handle(H** inout, int device)
{
    H* h = *inout;
    if (h && h->device != device) {                            // buffers of another device: start afresh on this one
        (void)hipSetDevice(h->device);
        h->release();
        h->clear();
    }
    TRY_HIP(hipSetDevice(device));
    if (!h) h = new H();
    *inout = h;
    h->device = device;
    return KMX_OK;
}

template <typename H>
void free_handle(H* h)
{
    if (!h) return;
    DeviceGuard dg;
    (void)hipSetDevice(h->device);
    h->release();                                              // (hipFree waits for the kernels of the last call)
    delete h;
}

// One array of a host view: room for max(count, 1) elements of `elem` bytes in h, and the first `count` of d copied there.
struct HostCopy {
    PinnedArr& h;
    const Buf& d;
    uint64_t count;
    uint32_t elem;
};

// Grows every array (a failure refuses before any copy), then copies on stream s of `device` and synchronises once.
inline kmx_status host_view(const char* fn, int device, hipStream_t s, const HostCopy* items, size_t n)
{
    bool any = false;
    for (const HostCopy* c = items; c != items + n; ++c) {
        if (!c->h.grow(std::max<uint64_t>(c->count, 1) * c->elem))
            return set_error(KMX_ERR_OUT_OF_MEMORY, std::string(fn) + ": page-locked host allocation failed");
        any = any || c->count;
    }
    if (!any) return KMX_OK;
    DeviceGuard dg;
    TRY_HIP(hipSetDevice(device));
    for (const HostCopy* c = items; c != items + n; ++c)
        if (c->count) TRY_HIP(hipMemcpyAsync(c->h.p, c->d.p, c->count * c->elem, hipMemcpyDeviceToHost, s));
    TRY_HIP(hipStreamSynchronize(s));
    return KMX_OK;
}

} // namespace kmx
