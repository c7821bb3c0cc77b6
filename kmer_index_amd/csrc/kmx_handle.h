// What the host code around the kernels shares: the buffers a handle owns, the error macros, the refusals every entry point starts
// with, and the steps of the lifecycle that every handle of the read-mapping chain follows (kmx_vote.hip, kmx_align.hip,
// kmx_script.hip, kmx_strands.hip, kmx_pairs.hip, kmx_rescue.hip, kmx_tags.hip, kmx_contigs.hip, kmx_secondary.hip, kmx_clip.hip,
// kmx_supplementary.hip, kmx_realign.hip, kmx_pileup.hip).  The other private headers of the chain: kmx_vote.h (what a stage reads of
// the handle before it), kmx_strands.h and kmx_clips.h (the handle structs that two sources fill), kmx_align_core.h,
// kmx_script_core.h, kmx_runs.h and kmx_fold_core.h (device code that several sources compile).
// A chain handle has the members `device`, `stream`, `host_valid` and `h_ctr`, declares its result arrays once, as Arr members and the list
// `results()`, and its scratch buffers as the list `scratch()`; release_arrays, clear_arrays, the device view of an array (ArrOf::dev) and
// host_view are derived from those lists here.  `release()` (its buffers go, on its device) and `clear()` (an empty result) stay the
// handle's own: the scalar counters are per handle.  DESIGN.md 7l has one row per handle and array.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

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

// the refusal of an index whose replicas a failed extension has left apart (kmx_capi.hip and kmx_approx.hip word theirs differently)
inline constexpr const char* kIndexUnusable = "the index is unusable: a failed kmx_index_extend_query_size_range left its replicas inconsistent";

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
        *why = kIndexUnusable;
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

// One result array of a chain handle.  It is its grow-only device buffer (ensure(), p and as<T>() as for any Buf: what the kernels of a run
// take), and holds the page-locked host copy and the live count n, the elements the handle exposes now: 0 after clear().  Room and live
// count are apart: ensure() only grows the device buffer, n is set when the fill has succeeded.
enum : uint32_t {
    ARR_OFFSETS = 1,       // an offset array (u64): while it exposes nothing its host view holds the one offset 0
    ARR_OWN_VIEW = 2,      // copied to the host by a view of its own, not with the handle's other arrays
};
struct Arr : Buf {
    PinnedArr h;
    const uint32_t elem;   // bytes per element
    const uint32_t flags;  // ARR_*
    uint64_t n = 0;
    Arr(uint32_t elem, uint32_t flags) : elem(elem), flags(flags) {}
    void release() { Buf::release(); h.release(); n = 0; }
};
// ... of elements T: the typed views
template <typename T>
struct ArrOf : Arr {
    explicit ArrOf(uint32_t flags = 0) : Arr(sizeof(T), flags) {}
    const T* dev() const { return n ? as<T>() : nullptr; }     // the device view: NULL while the array exposes nothing
    const T* host() const { return h.as<T>(); }                // the host view behind host_view(): never NULL
};

inline void expose(const std::vector<Arr*>& arrs, uint64_t n) { for (Arr* a : arrs) a->n = n; }

// what release() and clear() of a handle H do about its arrays
template <typename H>
void release_arrays(H& h)
{
    for (Arr* a : h.results()) a->release();
    for (Buf* b : h.scratch()) b->release();
    h.h_ctr.release();
}
template <typename H>
void clear_arrays(H& h)
{
    for (Arr* a : h.results()) a->n = 0;
    h.host_valid = false;
}

// The live elements of every array to its host copy: room for max(n, 1) elements each first (a failure refuses before any copy; the
// host pointers are never NULL), then the copies on stream s of `device` and one synchronisation.  fn: the entry point, for the text.
inline kmx_status copy_to_host(const char* fn, int device, hipStream_t s, const std::vector<Arr*>& arrs)
{
    bool any = false;
    for (Arr* a : arrs) {
        if (!a->h.grow(std::max<uint64_t>(a->n, 1) * a->elem))
            return set_error(KMX_ERR_OUT_OF_MEMORY, std::string(fn) + ": page-locked host allocation failed");
        if ((a->flags & ARR_OFFSETS) && !a->n) a->h.as<uint64_t>()[0] = 0;
        any = any || a->n;
    }
    if (!any) return KMX_OK;
    DeviceGuard dg;
    TRY_HIP(hipSetDevice(device));
    for (Arr* a : arrs)
        if (a->n) TRY_HIP(hipMemcpyAsync(a->h.p, a->p, a->n * a->elem, hipMemcpyDeviceToHost, s));
    TRY_HIP(hipStreamSynchronize(s));
    return KMX_OK;
}

// The host view of a handle: unless it is valid, every result array without a view of its own; `also`: one more array, whatever the
// handle's view holds (the caller keeps that array's validity)
template <typename H>
kmx_status host_view(const char* fn, H& h, Arr* also = nullptr)
{
    std::vector<Arr*> arrs;
    if (!h.host_valid)
        for (Arr* a : h.results())
            if (!(a->flags & ARR_OWN_VIEW)) arrs.push_back(a);
    if (also) arrs.push_back(also);
    if (arrs.empty()) return KMX_OK;
    TRY_KMX(copy_to_host(fn, h.device, h.stream, arrs));
    h.host_valid = true;
    return KMX_OK;
}

// The refusals of the entry point `who` behind its first ones, once it has looked at the handle h (nullptr: there is none yet): the handle
// holds an empty result.  who and h are the caller's variables, read when the refusal is made.
template <typename H>
auto refuser(const std::string& who, H*& h)
{
    return [&who, &h](kmx_status st, const std::string& msg) {
        if (h) h->clear();
        return set_error(st, who + msg);
    };
}

// The step an entry point ends in: the handle takes stream s and holds an empty result, the sticky HIP error goes, the stage runs; when
// it fails nothing is left in flight and the handle holds an empty result again, not half of this one.
template <typename H, typename F>
kmx_status run_into(H* h, hipStream_t s, F&& stage)
{
    h->stream = s;
    h->clear();
    (void)hipGetLastError();
    const kmx_status st = stage();
    if (st != KMX_OK) {
        (void)hipStreamSynchronize(s);
        h->clear();
    }
    return st;
}

} // namespace kmx
