// Seed voting (kmx_windows_vote, include/kmx.h): the candidate loci of every read from the hit lists of a windows search.
//
// Every hit p of window j of a read is one vote on the diagonal D = p - j * stride; a locus is a maximal run of a read's sorted
// diagonals in which neighbours are at most `band` apart.  The diagonals are handled BIASED, as d = D + B_r with
// B_r = (c_r - 1) * stride (the offset of the read's last window), so that they are unsigned: d = p + (c_r - 1 - j) * stride.
//
//   k_vote_count        a wave per read: its votes (hit counts of the voting windows), its skipped windows, its class
//   k_vote_small<T,CAP> a workgroup per read of at most CAP votes (and n + B_r < 2^32): the votes are read once into LDS as 32-bit
//                       keys, sorted there (bitonic, all exchanges ascending so that the padding is never stored), cut into loci,
//                       filtered by min_votes and written to scratch; two shapes, 256 threads up to kCapA votes, 1024 beyond
//   k_vote_compact      the scratch loci of the small reads into the final arrays (behind the scan over the per-read counts)
//   k_vote_emit         the large reads' votes as 64-bit keys (read << dbits | d) for kmx::sort_pairs_u64, then
//   k_vote_heads / k_vote_starts / k_vote_keep / k_vote_large_write: heads, scan, unique in the manner of the edit path
// Both classes write the same final arrays at locus_off[r], the exclusive scan of the per-read locus counts.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>

#include "kmx_kernels.h"
#include "kmx_vote.h"

namespace {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kWave = 64;
constexpr uint32_t kCapA = 2048;          // votes of the 256-thread shape: 8 KiB of keys, up to 8 workgroups per CU stay resident
constexpr uint32_t kBigThreads = 1024;
constexpr uint32_t kCapB = 15104;         // votes of the 1024-thread shape: 59 KiB of keys + 4 KiB of tables < 64 KiB, two workgroups per CU
constexpr uint32_t kWinChunk = 256;       // windows whose hit lists are located together
constexpr uint32_t kCountReads = 8;       // reads per wave of k_vote_count

enum : uint8_t { CLS_NONE = 0, CLS_SMALL_A = 1, CLS_SMALL_B = 2, CLS_LARGE = 3 };
enum { CTR_VOTES = 0, CTR_SMALL_A, CTR_SMALL_B, CTR_LARGE, CTR_LARGE_VOTES, CTR_LARGE_MAXB, CTR_OVERFLOW, CTR_SMALL_BOUND, CTR_COUNT };

using kmx::Buf;
using Pinned = kmx::PinnedArr;
using kmx::grid_for;

inline uint32_t bit_width(uint64_t x) { uint32_t b = 0; while (x) { ++b; x >>= 1; } return b; }

// what every kernel reads of the windows result and the options
struct VoteIn {
    const uint64_t* win_off;
    const uint64_t* hit_off;
    const uint32_t* positions;
    uint64_t nr, n;
    uint32_t stride, band, min_votes, max_occ;
};

__device__ __forceinline__ bool window_votes(uint64_t c, uint32_t max_occ) { return c != 0 && (max_occ == 0 || c <= max_occ); }

// ---- 1. count and classify ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_vote_count(VoteIn A, uint32_t cap, uint32_t cap_a, uint32_t* __restrict__ vcnt,
                                                       uint32_t* __restrict__ skipped, uint8_t* __restrict__ cls, uint32_t* __restrict__ smax,
                                                       uint32_t* __restrict__ lcnt, unsigned long long* __restrict__ ctr)
{
    __shared__ unsigned long long s_ctr[CTR_COUNT];
    if (threadIdx.x < CTR_COUNT) s_ctr[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    const uint64_t r0 = (uint64_t(blockIdx.x) * (kBlock / kWave) + wave) * kCountReads;
    for (uint32_t k = 0; k < kCountReads; ++k) {
        const uint64_t r = r0 + k;
        if (r >= A.nr) break;
        const uint64_t w0 = A.win_off[r], w1 = A.win_off[r + 1];
        uint64_t v = 0;
        uint32_t sk = 0;
        for (uint64_t j = w0 + lane; j < w1; j += kWave) {
            const uint64_t c = A.hit_off[j + 1] - A.hit_off[j];
            if (window_votes(c, A.max_occ)) v += c;
            else if (c) ++sk;
        }
        for (int off = kWave / 2; off > 0; off >>= 1) {
            v += __shfl_xor(v, off);
            sk += __shfl_xor(sk, off);
        }
        if (lane != 0) continue;
        const uint64_t cw = w1 - w0;
        const uint64_t bias = cw ? (cw - 1) * A.stride : 0;
        uint8_t c = CLS_NONE;
        if (v > 0xFFFFFFFFull) { atomicAdd(&s_ctr[CTR_OVERFLOW], 1ull); v = 0xFFFFFFFFull; }
        if (v) {
            const bool small = v <= cap && A.n + bias < (uint64_t(1) << 32);
            c = !small ? CLS_LARGE : v <= cap_a ? CLS_SMALL_A : CLS_SMALL_B;
            atomicAdd(&s_ctr[CTR_VOTES], (unsigned long long)v);
            atomicAdd(&s_ctr[c == CLS_LARGE ? CTR_LARGE : c == CLS_SMALL_A ? CTR_SMALL_A : CTR_SMALL_B], 1ull);
            if (small) {
                atomicAdd(&s_ctr[CTR_SMALL_BOUND], (unsigned long long)(v / A.min_votes));
            } else {
                atomicAdd(&s_ctr[CTR_LARGE_VOTES], (unsigned long long)v);
                atomicMax(&s_ctr[CTR_LARGE_MAXB], (unsigned long long)bias);
            }
        }
        vcnt[r] = uint32_t(v);
        skipped[r] = sk;
        cls[r] = c;
        smax[r] = (c == CLS_SMALL_A || c == CLS_SMALL_B) ? uint32_t(v / A.min_votes) : 0u;   // a read has at most votes / min_votes loci
        lcnt[r] = c == CLS_LARGE ? uint32_t(v) : 0u;
    }
    __syncthreads();
    if (threadIdx.x < CTR_COUNT && s_ctr[threadIdx.x]) {
        if (threadIdx.x == CTR_LARGE_MAXB) atomicMax(&ctr[threadIdx.x], s_ctr[threadIdx.x]);
        else atomicAdd(&ctr[threadIdx.x], s_ctr[threadIdx.x]);
    }
}

// ---- shared by both classes: a read's votes, located chunk of windows by chunk of windows -----------------------------------------------
template <int T>
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t* total)
{
    __shared__ uint32_t wave_sum[T / kWave];
    const uint32_t lane = threadIdx.x % kWave, w = threadIdx.x / kWave;
    uint32_t inc = v;
    for (uint32_t off = 1; off < kWave; off <<= 1) {
        const uint32_t t = __shfl_up(inc, off);
        if (lane >= off) inc += t;
    }
    if (lane == kWave - 1) wave_sum[w] = inc;
    __syncthreads();
    uint32_t carry = 0, tot = 0;
    for (uint32_t i = 0; i < T / kWave; ++i) {
        const uint32_t s = wave_sum[i];
        if (i < w) carry += s;
        tot += s;
    }
    __syncthreads();                                           // (the next call writes wave_sum again)
    *total = tot;
    return carry + inc - v;
}

// store(i, p, j): vote i of the read (in window order) is hit p of window j.  The first kWinChunk threads take a window each, an
// exclusive scan of the voting windows' counts places their lists, and all T threads then walk the chunk's votes in order — a
// binary search over the kWinChunk starts names the window — so that `positions` is read with coalesced loads.
// wvo: kWinChunk + 1 words, whs: kWinChunk words of LDS.
template <int T, typename Store>
__device__ __forceinline__ void load_votes(const VoteIn& A, uint64_t w0, uint64_t cw, uint32_t* wvo, uint64_t* whs, Store store)
{
    const uint32_t tid = threadIdx.x;
    uint32_t base = 0;
    for (uint64_t wc = 0; wc < cw; wc += kWinChunk) {
        uint32_t cnt = 0;
        if (tid < kWinChunk && wc + tid < cw) {
            const uint64_t hs = A.hit_off[w0 + wc + tid], c = A.hit_off[w0 + wc + tid + 1] - hs;
            if (window_votes(c, A.max_occ)) cnt = uint32_t(c);  // (the read's votes fit 32 bits: k_vote_count saw to it)
            whs[tid] = hs;
        }
        uint32_t tot;
        const uint32_t ex = block_exclusive_scan<T>(cnt, &tot);
        if (tid < kWinChunk) wvo[tid] = ex;
        if (tid == 0) wvo[kWinChunk] = tot;
        __syncthreads();
        for (uint32_t i = tid; i < tot; i += T) {
            uint32_t lo = 0, hi = kWinChunk;                    // the last window that starts at or before vote i (it is not empty)
            while (hi - lo > 1) {
                const uint32_t mid = (lo + hi) >> 1;
                if (wvo[mid] <= i) lo = mid; else hi = mid;
            }
            store(base + i, A.positions[whs[lo] + (i - wvo[lo])], wc + lo);
        }
        base += tot;
        __syncthreads();
    }
}

// ---- 2. the small class -------------------------------------------------------------------------------------------------------------
struct SmallOut {
    const uint32_t* vcnt;
    const uint8_t* cls;
    const uint64_t* sc_off;     // first scratch slot of every read (exclusive scan of smax)
    int64_t* sc_diag;
    uint32_t* sc_span;
    uint32_t* sc_votes;
    uint32_t* lcount;           // loci kept per read
};

template <int T, int CAP, uint8_t CLS>
__global__ __launch_bounds__(T) void k_vote_small(VoteIn A, SmallOut O)
{
    constexpr uint32_t AUX = (T + 1 > int(kWinChunk) + 2 + 2 * int(kWinChunk)) ? T + 1 : kWinChunk + 2 + 2 * kWinChunk;
    __shared__ uint32_t keys[CAP];
    __shared__ uint64_t aux64[(AUX + 1) / 2];
    const uint64_t r = blockIdx.x;
    if (O.cls[r] != CLS) return;
    const uint32_t tid = threadIdx.x;
    const uint32_t v = min(O.vcnt[r], uint32_t(CAP));           // (a read of this class has at most CAP votes)
    const uint64_t w0 = A.win_off[r], cw = A.win_off[r + 1] - w0;
    const uint32_t bias = uint32_t((cw - 1) * A.stride);        // n + bias < 2^32 for this class
    const uint32_t stride = A.stride;
    uint32_t* wvo = reinterpret_cast<uint32_t*>(aux64);
    uint64_t* whs = aux64 + (kWinChunk + 2) / 2;
    load_votes<T>(A, w0, cw, wvo, whs, [&](uint32_t i, uint32_t p, uint64_t j) {
        if (i < v) keys[i] = p + (bias - uint32_t(j) * stride);
    });
    // bitonic sort of keys[0, v) as the head of n2 = 2^ceil(log2 v) keys whose tail is +infinity: every exchange puts the smaller key
    // at the lower index (the first step of a merge mirrors its partner), so a pair that reaches into the tail never exchanges and
    // the tail is never stored
    uint32_t n2 = 1;
    while (n2 < v) n2 <<= 1;
    for (uint32_t k = 2; k <= n2; k <<= 1) {
        const uint32_t half = k >> 1;
        for (uint32_t t = tid; t < (n2 >> 1); t += T) {
            const uint32_t blk = t / half, off = t % half;
            const uint32_t i = blk * k + off, l = blk * k + (k - 1 - off);
            if (l < v) {
                const uint32_t a = keys[i], b = keys[l];
                if (a > b) { keys[i] = b; keys[l] = a; }
            }
        }
        __syncthreads();
        for (uint32_t j = half >> 1; j > 0; j >>= 1) {
            for (uint32_t t = tid; t < (n2 >> 1); t += T) {
                const uint32_t i = 2 * j * (t / j) + t % j, l = i + j;
                if (l < v) {
                    const uint32_t a = keys[i], b = keys[l];
                    if (a > b) { keys[i] = b; keys[l] = a; }
                }
            }
            __syncthreads();
        }
    }
    // loci: thread t owns keys[lo, hi), an odd number of them (no LDS bank is hit twice by a wave); first[t] = the first head in its
    // range, then, by a suffix minimum, the first head at or behind lo: where a locus that leaves the range ends
    uint32_t* first = reinterpret_cast<uint32_t*>(aux64);       // T + 1 words (the window tables are done with)
    const uint32_t per = ((v + T - 1) / T) | 1u;
    const uint32_t lo = min(tid * per, v), hi = min(lo + per, v);
    const uint32_t band = A.band;
    auto head = [&](uint32_t i) { return i == 0 || keys[i] - keys[i - 1] > band; };
    uint32_t fh = v;
    for (uint32_t i = lo; i < hi; ++i)
        if (head(i)) { fh = i; break; }
    first[tid] = fh;
    if (tid == 0) first[T] = v;
    __syncthreads();
    for (uint32_t off = 1; off < T; off <<= 1) {
        const uint32_t x = tid + off < T ? first[tid + off] : v;
        __syncthreads();
        if (x < first[tid]) first[tid] = x;
        __syncthreads();
    }
    const uint32_t next_first = first[tid + 1];
    const uint32_t min_votes = A.min_votes;
    uint32_t kept = 0;
    for (uint32_t i = fh; i < hi;) {                            // i is a head
        uint32_t e = i + 1;
        while (e < hi && !head(e)) ++e;
        const uint32_t end = e < hi ? e : next_first;
        if (end - i >= min_votes) ++kept;
        i = e;
    }
    uint32_t total;
    uint32_t at = block_exclusive_scan<T>(kept, &total);
    const uint64_t sc = O.sc_off[r];
    for (uint32_t i = fh; i < hi;) {
        uint32_t e = i + 1;
        while (e < hi && !head(e)) ++e;
        const uint32_t end = e < hi ? e : next_first;
        if (end - i >= min_votes) {
            O.sc_diag[sc + at] = int64_t(keys[i]) - int64_t(bias);
            O.sc_span[sc + at] = keys[end - 1] - keys[i];
            O.sc_votes[sc + at] = end - i;
            ++at;
        }
        i = e;
    }
    if (tid == 0) O.lcount[r] = total;
}

// a wave per small read: its loci from scratch to their place in the final arrays
__global__ __launch_bounds__(kBlock) void k_vote_compact(uint64_t nr, const uint8_t* __restrict__ cls, const uint64_t* __restrict__ sc_off,
                                                         const uint32_t* __restrict__ lcount, const uint64_t* __restrict__ locus_off,
                                                         const int64_t* __restrict__ sc_diag, const uint32_t* __restrict__ sc_span,
                                                         const uint32_t* __restrict__ sc_votes, int64_t* __restrict__ diag,
                                                         uint32_t* __restrict__ span, uint32_t* __restrict__ votes)
{
    const uint64_t r = uint64_t(blockIdx.x) * (kBlock / kWave) + threadIdx.x / kWave;
    if (r >= nr || (cls[r] != CLS_SMALL_A && cls[r] != CLS_SMALL_B)) return;
    const uint64_t src = sc_off[r], dst = locus_off[r];
    const uint32_t c = lcount[r];
    for (uint32_t i = threadIdx.x % kWave; i < c; i += kWave) {
        diag[dst + i] = sc_diag[src + i];
        span[dst + i] = sc_span[src + i];
        votes[dst + i] = sc_votes[src + i];
    }
}

// ---- 3. the large class -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_vote_emit(VoteIn A, const uint8_t* __restrict__ cls, const uint32_t* __restrict__ vcnt,
                                                      const uint64_t* __restrict__ lvote_off, uint32_t dbits, uint64_t* __restrict__ keys)
{
    __shared__ uint32_t wvo[kWinChunk + 2];
    __shared__ uint64_t whs[kWinChunk];
    const uint64_t r = blockIdx.x;
    if (cls[r] != CLS_LARGE) return;
    const uint64_t w0 = A.win_off[r], cw = A.win_off[r + 1] - w0;
    const uint64_t bias = (cw - 1) * A.stride, at = lvote_off[r], hi = r << dbits;
    const uint32_t v = vcnt[r], stride = A.stride;
    load_votes<kBlock>(A, w0, cw, wvo, whs, [&](uint32_t i, uint32_t p, uint64_t j) {
        if (i < v) keys[at + i] = hi | (uint64_t(p) + (bias - j * stride));
    });
}

// a head: the first vote of a read, or one more than `band` above the vote before it
__global__ __launch_bounds__(kBlock) void k_vote_heads(const uint64_t* __restrict__ keys, uint64_t n_v, uint32_t dbits, uint32_t band,
                                                       uint32_t* __restrict__ head)
{
    const uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (i >= n_v) return;
    bool h = i == 0;
    if (!h) {
        const uint64_t a = keys[i - 1], b = keys[i];
        h = (a >> dbits) != (b >> dbits) || b - a > band;
    }
    head[i] = h ? 1u : 0u;
}

__global__ __launch_bounds__(kBlock) void k_vote_starts(const uint32_t* __restrict__ head, const uint64_t* __restrict__ rank, uint64_t n_v,
                                                        uint64_t* __restrict__ hstart)
{
    const uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (i < n_v && head[i]) hstart[rank[i]] = i;
}

// per locus of the large reads: kept or not, counted into its read; the first locus of every read names itself in ufirst
__global__ __launch_bounds__(kBlock) void k_vote_keep(const uint64_t* __restrict__ keys, const uint64_t* __restrict__ hstart, uint64_t n_u,
                                                      uint64_t n_v, uint32_t dbits, uint32_t min_votes, uint32_t* __restrict__ keep,
                                                      uint32_t* __restrict__ lcount, uint64_t* __restrict__ ufirst)
{
    const uint64_t u = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (u >= n_u) return;
    const uint64_t s = hstart[u], e = u + 1 < n_u ? hstart[u + 1] : n_v;
    const uint64_t r = keys[s] >> dbits;
    const bool k = e - s >= min_votes;
    keep[u] = k ? 1u : 0u;
    if (k) atomicAdd(&lcount[r], 1u);
    if (u == 0 || (keys[hstart[u - 1]] >> dbits) != r) ufirst[r] = u;
}

__global__ __launch_bounds__(kBlock) void k_vote_large_write(VoteIn A, const uint64_t* __restrict__ keys, const uint64_t* __restrict__ hstart,
                                                             uint64_t n_u, uint64_t n_v, uint32_t dbits, const uint32_t* __restrict__ keep,
                                                             const uint64_t* __restrict__ krank, const uint64_t* __restrict__ ufirst,
                                                             const uint64_t* __restrict__ locus_off, int64_t* __restrict__ diag,
                                                             uint32_t* __restrict__ span, uint32_t* __restrict__ votes)
{
    const uint64_t u = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (u >= n_u || !keep[u]) return;
    const uint64_t s = hstart[u], e = u + 1 < n_u ? hstart[u + 1] : n_v;
    const uint64_t k0 = keys[s], r = k0 >> dbits, mask = (uint64_t(1) << dbits) - 1;
    const uint64_t bias = (A.win_off[r + 1] - A.win_off[r] - 1) * A.stride;
    const uint64_t dst = locus_off[r] + (krank[u] - krank[ufirst[r]]);
    const uint64_t sp = keys[e - 1] - k0;
    diag[dst] = int64_t(k0 & mask) - int64_t(bias);
    span[dst] = sp > 0xFFFFFFFFull ? 0xFFFFFFFFu : uint32_t(sp);
    votes[dst] = uint32_t(e - s);
}

} // namespace

struct kmx_loci {
    int device = 0;
    hipStream_t stream = nullptr;          // the stream of the vote that filled the handle (the host view copies on it)
    uint64_t nr = 0, n_loci = 0, n_votes = 0, n_small = 0, n_large = 0;
    // results; locus_off and skipped are handed out whatever the handle holds, and a handle that a vote has ever filled keeps the one
    // offset 0 (kmx_windows_vote writes it on the device after an error)
    kmx::ArrOf<uint64_t> locus_off{kmx::ARR_OFFSETS};
    kmx::ArrOf<int64_t> diag;
    kmx::ArrOf<uint32_t> span, votes, skipped;
    // scratch
    Buf vcnt, cls, smax, lcnt, lcount, sc_off, lvote_off, bsum, ctr, sc_diag, sc_span, sc_votes, ka, kb, va, vb, hstart, keep, krank, ufirst;
    const uint64_t* sorted_keys = nullptr; // the large reads' keys behind the sort: ka or kb
    Pinned h_ctr;
    bool host_valid = false;
    std::vector<kmx::Arr*> results() { return {&locus_off, &diag, &span, &votes, &skipped}; }
    std::vector<Buf*> scratch()
    {
        return {&vcnt, &cls, &smax, &lcnt, &lcount, &sc_off, &lvote_off, &bsum, &ctr, &sc_diag, &sc_span, &sc_votes, &ka, &kb, &va, &vb, &hstart, &keep,
                &krank, &ufirst};
    }
    void release() { kmx::release_arrays(*this); }
    void clear()
    {
        nr = n_loci = n_votes = n_small = n_large = 0;
        kmx::clear_arrays(*this);
        locus_off.n = locus_off.p ? 1 : 0;
    }
};

namespace {

// the cap on the votes of a small read: kCapB, lowered by KMX_VOTE_SMALL_CAP (read at every call; 0: every read is large)
uint32_t small_cap()
{
    const char* e = getenv("KMX_VOTE_SMALL_CAP");
    if (!e || !*e) return kCapB;
    char* end = nullptr;
    const unsigned long long x = strtoull(e, &end, 10);
    if (end == e || *end) return kCapB;
    return uint32_t(std::min<unsigned long long>(x, kCapB));
}

// the large reads: keys, sort, heads, starts, keep + its scan (lcount[r] counts their kept loci; the final write follows the scan)
kmx_status vote_large(const kmx::WindowsAccess& W, const VoteIn& A, kmx_loci* L, uint64_t n_v, uint32_t dbits, uint64_t* n_u_out)
{
    hipStream_t s = W.stream;
    const uint64_t nr = A.nr;
    unsigned long long* d_total = L->ctr.as<unsigned long long>() + CTR_COUNT;
    TRY_HIP(L->lvote_off.ensure((nr + 1) * 8));
    TRY_HIP(L->ka.ensure((n_v + 1) * 8));
    TRY_HIP(L->kb.ensure((n_v + 1) * 8));
    TRY_HIP(L->va.ensure(n_v * 4 + 16));
    TRY_HIP(L->vb.ensure(n_v * 4 + 16));
    TRY_HIP(L->ufirst.ensure(nr * 8));
    TRY_HIP(L->bsum.ensure(std::max(kmx::scan_blocks(n_v), kmx::scan_blocks(nr)) * 8 + 16));
    kmx::vote_timed(W.index, s, [&] {
        kmx::launch_scan(s, L->lcnt.as<uint32_t>(), nr, L->bsum.as<uint64_t>(), L->lvote_off.as<uint64_t>(), d_total);
        hipLaunchKernelGGL(k_vote_emit, dim3(unsigned(nr)), dim3(kBlock), 0, s, A, L->cls.as<uint8_t>(), L->vcnt.as<uint32_t>(),
                           L->lvote_off.as<uint64_t>(), dbits, L->ka.as<uint64_t>());
    });
    TRY_HIP(hipGetLastError());
    bool in_b = false;
    hipError_t se = hipSuccess;
    kmx::vote_timed(W.index, s, [&] {                          // (the value arrays carry nothing: only the keys are read afterwards)
        se = kmx::sort_pairs_u64(s, L->ka.as<uint64_t>(), L->va.as<uint32_t>(), L->kb.as<uint64_t>(), L->vb.as<uint32_t>(), n_v,
                                 dbits + std::max(bit_width(nr - 1), 1u), &in_b);
    });
    TRY_HIP(se);
    const uint64_t* keys = L->sorted_keys = in_b ? L->kb.as<uint64_t>() : L->ka.as<uint64_t>();
    uint64_t* rank = in_b ? L->ka.as<uint64_t>() : L->kb.as<uint64_t>();          // the other pair of arrays is free again
    uint32_t* head = L->va.as<uint32_t>();
    kmx::vote_timed(W.index, s, [&] {
        hipLaunchKernelGGL(k_vote_heads, dim3(grid_for(n_v, kBlock)), dim3(kBlock), 0, s, keys, n_v, dbits, A.band, head);
        kmx::launch_scan(s, head, n_v, L->bsum.as<uint64_t>(), rank, d_total);
    });
    TRY_HIP(hipGetLastError());
    TRY_KMX(kmx::read_back("kmx_windows_vote", s, d_total, L->h_ctr, 8));
    const uint64_t n_u = L->h_ctr.as<uint64_t>()[0];          // (>= 1: the first vote heads a locus)
    TRY_HIP(L->hstart.ensure(n_u * 8));
    TRY_HIP(L->keep.ensure(n_u * 4 + 16));
    TRY_HIP(L->krank.ensure((n_u + 1) * 8));
    TRY_HIP(L->bsum.ensure(std::max(kmx::scan_blocks(n_u), kmx::scan_blocks(nr)) * 8 + 16));
    kmx::vote_timed(W.index, s, [&] {
        hipLaunchKernelGGL(k_vote_starts, dim3(grid_for(n_v, kBlock)), dim3(kBlock), 0, s, head, rank, n_v, L->hstart.as<uint64_t>());
        hipLaunchKernelGGL(k_vote_keep, dim3(grid_for(n_u, kBlock)), dim3(kBlock), 0, s, keys, L->hstart.as<uint64_t>(), n_u, n_v, dbits,
                           A.min_votes, L->keep.as<uint32_t>(), L->lcount.as<uint32_t>(), L->ufirst.as<uint64_t>());
        kmx::launch_scan(s, L->keep.as<uint32_t>(), n_u, L->bsum.as<uint64_t>(), L->krank.as<uint64_t>(), d_total);
    });
    TRY_HIP(hipGetLastError());
    *n_u_out = n_u;
    return KMX_OK;
}

kmx_status vote_run(const kmx::WindowsAccess& W, const kmx_vote_options& o, kmx_loci* L)
{
    hipStream_t s = W.stream;
    const uint64_t nr = W.nr;
    L->stream = s;
    L->clear();
    L->nr = nr;
    (void)hipGetLastError();
    TRY_HIP(L->locus_off.ensure((nr + 1) * 8));
    TRY_HIP(L->skipped.ensure(std::max<uint64_t>(nr, 1) * 4));
    L->locus_off.n = nr + 1;
    L->skipped.n = nr;
    TRY_HIP(hipMemsetAsync(L->locus_off.p, 0, (nr + 1) * 8, s));
    if (nr == 0) return KMX_OK;
    if (nr >= (uint64_t(1) << 31))
        return kmx::set_error(KMX_ERR_TOO_LARGE, "kmx_windows_vote: at most 2^31-1 reads per call (a workgroup per read): split the reads");
    if (W.nq == 0) {                                           // no read has a window
        TRY_HIP(hipMemsetAsync(L->skipped.p, 0, nr * 4, s));
        return KMX_OK;
    }
    const VoteIn A{W.win_off, W.hit_off, W.positions, nr, W.n, W.stride, o.band, o.min_votes, o.max_occ};
    const uint32_t cap = small_cap(), cap_a = std::min(cap, kCapA);
    for (Buf* b : {&L->vcnt, &L->smax, &L->lcnt, &L->lcount}) TRY_HIP(b->ensure(nr * 4 + 16));
    TRY_HIP(L->cls.ensure(nr));
    TRY_HIP(L->sc_off.ensure((nr + 1) * 8));
    TRY_HIP(L->bsum.ensure(kmx::scan_blocks(nr) * 8 + 16));
    TRY_HIP(L->ctr.ensure((CTR_COUNT + 1) * 8));
    unsigned long long* ctr = L->ctr.as<unsigned long long>();
    unsigned long long* d_total = ctr + CTR_COUNT;
    TRY_HIP(hipMemsetAsync(ctr, 0, (CTR_COUNT + 1) * 8, s));
    TRY_HIP(hipMemsetAsync(L->lcount.p, 0, nr * 4, s));
    kmx::vote_timed(W.index, s, [&] {
        hipLaunchKernelGGL(k_vote_count, dim3(grid_for(nr, (kBlock / kWave) * kCountReads)), dim3(kBlock), 0, s, A, cap, cap_a,
                           L->vcnt.as<uint32_t>(), L->skipped.as<uint32_t>(), L->cls.as<uint8_t>(), L->smax.as<uint32_t>(),
                           L->lcnt.as<uint32_t>(), ctr);
    });
    TRY_HIP(hipGetLastError());
    TRY_KMX(kmx::read_back("kmx_windows_vote", s, ctr, L->h_ctr, CTR_COUNT * 8));
    uint64_t c[CTR_COUNT];
    std::memcpy(c, L->h_ctr.p, sizeof c);
    if (c[CTR_OVERFLOW]) return kmx::set_error(KMX_ERR_TOO_LARGE, "kmx_windows_vote: a read casts 2^32 or more votes: set max_occ or split the read");
    L->n_votes = c[CTR_VOTES];
    L->n_small = c[CTR_SMALL_A] + c[CTR_SMALL_B];
    L->n_large = c[CTR_LARGE];
    if (!L->n_votes) return KMX_OK;

    if (L->n_small) {
        const uint64_t bound = std::max<uint64_t>(c[CTR_SMALL_BOUND], 1);
        TRY_HIP(L->sc_diag.ensure(bound * 8));
        TRY_HIP(L->sc_span.ensure(bound * 4));
        TRY_HIP(L->sc_votes.ensure(bound * 4));
        const SmallOut O{L->vcnt.as<uint32_t>(), L->cls.as<uint8_t>(), L->sc_off.as<uint64_t>(), L->sc_diag.as<int64_t>(), L->sc_span.as<uint32_t>(),
                         L->sc_votes.as<uint32_t>(), L->lcount.as<uint32_t>()};
        kmx::vote_timed(W.index, s, [&] {
            kmx::launch_scan(s, L->smax.as<uint32_t>(), nr, L->bsum.as<uint64_t>(), L->sc_off.as<uint64_t>(), d_total);
            if (c[CTR_SMALL_A])
                hipLaunchKernelGGL((k_vote_small<kBlock, kCapA, CLS_SMALL_A>), dim3(unsigned(nr)), dim3(kBlock), 0, s, A, O);
            if (c[CTR_SMALL_B])
                hipLaunchKernelGGL((k_vote_small<kBigThreads, kCapB, CLS_SMALL_B>), dim3(unsigned(nr)), dim3(kBigThreads), 0, s, A, O);
        });
        TRY_HIP(hipGetLastError());
    }
    uint64_t n_u = 0;
    uint32_t dbits = 0;
    if (L->n_large) {
        dbits = std::max(bit_width(W.n - 1 + c[CTR_LARGE_MAXB]), 1u);
        if (dbits + std::max(bit_width(nr - 1), 1u) > 64)
            return kmx::set_error(KMX_ERR_TOO_LARGE, "kmx_windows_vote: read number and diagonal do not fit a 64-bit sort key: split the reads");
        TRY_KMX(vote_large(W, A, L, c[CTR_LARGE_VOTES], dbits, &n_u));
    }
    kmx::vote_timed(W.index, s, [&] {
        kmx::launch_scan(s, L->lcount.as<uint32_t>(), nr, L->bsum.as<uint64_t>(), L->locus_off.as<uint64_t>(),
                         L->locus_off.as<unsigned long long>() + nr);
    });
    TRY_HIP(hipGetLastError());
    TRY_KMX(kmx::read_back("kmx_windows_vote", s, L->locus_off.as<uint64_t>() + nr, L->h_ctr, 8));
    L->n_loci = L->h_ctr.as<uint64_t>()[0];
    if (!L->n_loci) return KMX_OK;
    TRY_HIP(L->diag.ensure(L->n_loci * 8));
    TRY_HIP(L->span.ensure(L->n_loci * 4));
    TRY_HIP(L->votes.ensure(L->n_loci * 4));
    kmx::vote_timed(W.index, s, [&] {
        if (L->n_small)
            hipLaunchKernelGGL(k_vote_compact, dim3(grid_for(nr, kBlock / kWave)), dim3(kBlock), 0, s, nr, L->cls.as<uint8_t>(), L->sc_off.as<uint64_t>(),
                               L->lcount.as<uint32_t>(), L->locus_off.as<uint64_t>(), L->sc_diag.as<int64_t>(), L->sc_span.as<uint32_t>(),
                               L->sc_votes.as<uint32_t>(), L->diag.as<int64_t>(), L->span.as<uint32_t>(), L->votes.as<uint32_t>());
        if (L->n_large)
            hipLaunchKernelGGL(k_vote_large_write, dim3(grid_for(n_u, kBlock)), dim3(kBlock), 0, s, A, L->sorted_keys, L->hstart.as<uint64_t>(), n_u,
                               c[CTR_LARGE_VOTES], dbits, L->keep.as<uint32_t>(), L->krank.as<uint64_t>(), L->ufirst.as<uint64_t>(),
                               L->locus_off.as<uint64_t>(), L->diag.as<int64_t>(), L->span.as<uint32_t>(), L->votes.as<uint32_t>());
    });
    TRY_HIP(hipGetLastError());
    kmx::expose({&L->diag, &L->span, &L->votes}, L->n_loci);
    return KMX_OK;
}

} // namespace

kmx::LociAccess kmx::loci_access(const kmx_loci* l)
{
    const bool filled = l->locus_off.p != nullptr;
    return kmx::LociAccess{l->device, l->stream, filled ? l->nr : 0, filled ? l->n_loci : 0, l->locus_off.as<uint64_t>(),
                           l->diag.as<int64_t>(), l->span.as<uint32_t>(), l->votes.as<uint32_t>()};
}

extern "C" {

kmx_status kmx_windows_vote(kmx_result* windows, const kmx_vote_options* o, kmx_loci** inout)
{
    if (!windows || !o || !inout) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_windows_vote: NULL argument");
    if (o->struct_size < sizeof(kmx_vote_options)) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_windows_vote: options->struct_size is too small");
    if (o->flags != 0) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_windows_vote: flags must be 0");
    if (o->min_votes == 0) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_windows_vote: min_votes must be at least 1");
    kmx::WindowsAccess W{};
    TRY_KMX(kmx::windows_access(windows, &W));
    kmx::DeviceGuard dg;
    TRY_KMX(kmx::bind_handle(inout, W.device));
    kmx_loci* L = *inout;
    const kmx_status st = vote_run(W, *o, L);
    if (st != KMX_OK) {                                        // the handle holds an empty result, not half of this one
        L->clear();
        if (L->locus_off.p) (void)hipMemsetAsync(L->locus_off.p, 0, 8, W.stream);
        (void)hipStreamSynchronize(W.stream);
    }
    return st;
}

kmx_status kmx_loci_counts(const kmx_loci* l, uint64_t* nr, uint64_t* n_loci, uint64_t* n_votes, uint64_t* n_small, uint64_t* n_large)
{
    if (!l) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_loci_counts: loci handle is NULL");
    if (nr) *nr = l->nr;
    if (n_loci) *n_loci = l->n_loci;
    if (n_votes) *n_votes = l->n_votes;
    if (n_small) *n_small = l->n_small;
    if (n_large) *n_large = l->n_large;
    return KMX_OK;
}

kmx_status kmx_loci_view_device(const kmx_loci* l, const uint64_t** d_locus_off, const int64_t** d_diag, const uint32_t** d_span,
                                const uint32_t** d_votes, const uint32_t** d_skipped)
{
    if (!l) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_loci_view_device: loci handle is NULL");
    if (d_locus_off) *d_locus_off = l->locus_off.as<uint64_t>();
    if (d_diag) *d_diag = l->diag.dev();
    if (d_span) *d_span = l->span.dev();
    if (d_votes) *d_votes = l->votes.dev();
    if (d_skipped) *d_skipped = l->skipped.as<uint32_t>();
    return KMX_OK;
}

kmx_status kmx_loci_view(kmx_loci* l, const uint64_t** locus_off, const int64_t** diag, const uint32_t** span, const uint32_t** votes,
                         const uint32_t** skipped)
{
    if (!l) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_loci_view: loci handle is NULL");
    TRY_KMX(kmx::host_view("kmx_loci_view", *l));
    if (locus_off) *locus_off = l->locus_off.host();
    if (diag) *diag = l->diag.host();
    if (span) *span = l->span.host();
    if (votes) *votes = l->votes.host();
    if (skipped) *skipped = l->skipped.host();
    return KMX_OK;
}

void kmx_loci_free(kmx_loci* l) { kmx::free_handle(l); }

} // extern "C"
