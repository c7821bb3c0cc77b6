// What the host code around the kernels shares: the buffers a handle owns, the error macros, the refusals every entry point starts
// with, and the steps of the lifecycle that every handle of the read-mapping chain follows (kmx_vote.hip, kmx_align.hip,
// kmx_script.hip, kmx_strands.hip, kmx_pairs.hip, kmx_rescue.hip, kmx_tags.hip, kmx_contigs.hip, kmx_secondary.hip, kmx_clip.hip,
// kmx_supplementary.hip, kmx_realign.hip, kmx_pileup.hip).  The other private headers of the chain: kmx_vote.h (what a stage reads of
// the handle before it), kmx_strands.h and kmx_clips.h (the handle structs that two sources fill), kmx_align_core.h,
// kmx_script_core.h, kmx_runs.h and kmx_fold_core.h (device code that several sources compile).
// A chain handle has the members `device`, `release()` (its buffers go, on its device) and `clear()` (an empty result).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "kmx_approx.h"
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

// the first refusals of an entry point `who` ("kmx_...: ") with options o and a handle to fill at *inout
template <typename O>
kmx_status check_call(const std::string& who, const O* o, const void* inout)
{
    if (!o) return set_error(KMX_ERR_INVALID_ARGUMENT, who + "options is NULL");
    if (!inout) return set_error(KMX_ERR_INVALID_ARGUMENT, who + "inout is NULL");
    if (o->struct_size < sizeof(O)) return set_error(KMX_ERR_INVALID_ARGUMENT, who + "options->struct_size is too small");
    return KMX_OK;
}

// *X = the replica of `index` on `device`, where `whose` ("the scripts", "the loci", ...) live; false: there is none, or the index is
// broken, and (*st, *why) is the refusal
inline bool index_for(const kmx_index* index, int device, const char* whose, IndexAccess* X, kmx_status* st, std::string* why)
{
    if (!index_access_on(index, device, X)) {
        *st = KMX_ERR_INVALID_ARGUMENT;
        *why = std::string(whose) + " live on a device that holds no replica of this index";
        return false;
    }
    if (X->broken) {
        *st = KMX_ERR_HIP;
        *why = "the index is unusable: a failed kmx_index_extend_query_size_range left its replicas inconsistent";
        return false;
    }
    return true;
}

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

// *inout becomes a handle on `device` (created when NULL), and `device` the current one: the caller holds a DeviceGuard.  When the
// device cannot be made current, a handle there is holds an empty result, as after every refusal that has looked at it.
template <typename H>
kmx_status bind_handle(H** inout, int device)
{
    H* h = *inout;
    if (h && h->device != device) {                            // buffers of another device: start afresh on this one
        (void)hipSetDevice(h->device);
        h->release();
        h->clear();
    }
    if (hipError_t e = hipSetDevice(device); e != hipSuccess) {
        (void)hipGetLastError();
        if (h) h->clear();
        return set_error(KMX_ERR_HIP, std::string("hipSetDevice(device): ") + hipGetErrorString(e));
    }
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
