// What the edit scripts (kmx_script.hip) and the realignment (kmx_realign.hip) share: both run a wave per entry over the band
// |j - i| <= d of read x text[start, end), in classes of NPL diagonals per lane, with the letters of the entry staged in LDS and the
// traceback codes in an arena that is cut into chunks.  Everything here has internal linkage: each of the two sources compiles its own.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kmx_handle.h"

namespace {

constexpr uint32_t kWave = 64;
constexpr int kClasses = 4;                                   // NPL = 1, 2, 4, 8
constexpr uint32_t kNoRead = 0x1FF, kNoText = 0x2FF;          // letters that equal nothing
constexpr uint32_t kTextLds = KMX_ALIGN_MAX_READ + 256;       // L <= m + d <= 1024 + 250
constexpr uint64_t kDefaultScratch = uint64_t(256) << 20;
constexpr uint64_t kMaxChunk = uint64_t(1) << 30;             // entries of one chunk: the grid of the band kernels
// the counters that k_script_cut reads; a source goes on from CTR_SHARED with its own
enum { CTR_N_SEL = 0, CTR_CODE_BYTES, CTR_RES_RUNS, CTR_MAX_CODE, CTR_CUT, CTR_CLASS, CTR_SHARED = CTR_CLASS + kClasses };

// what every kernel reads
struct ScriptIn {
    const uint8_t* ranks;
    const uint64_t* roff;          // [nr + 1]
    uint64_t ranks_len;            // letters that may be read (host form: roff[nr]; device form: no bound of ours)
    const uint64_t* locus_off;     // [nr + 1]
    const uint8_t* dist;           // [n_loci]
    const uint32_t* start;
    const uint32_t* end;
    const uint32_t* best;          // [nr]
    uint64_t nr, n_loci, n;
    const uint64_t* text;          // packed at w bits per letter
    uint32_t w, sigma, flags;
};

// Read, text substring and distance of an entry; ok == false: the entry gets no script (kmx.h, "foreign reads").  With ok,
// m <= KMX_ALIGN_MAX_READ, d <= KMX_ALIGN_MAX_EDITS, |m - L| <= d and text[start, start + L) lies inside the text.
struct Entry {
    uint64_t r0;
    uint32_t m, L, d, start;
    bool ok;
};

__device__ __forceinline__ Entry entry_of(const ScriptIn& S, uint32_t r, uint32_t l)
{
    Entry en{};
    const uint64_t r0 = S.roff[r], r1 = S.roff[r + 1];
    const uint32_t s = S.start[l], e = S.end[l], d = S.dist[l];
    en.r0 = r0;
    en.start = s;
    en.d = d;
    if (!(r1 >= r0 && r1 <= S.ranks_len && r1 - r0 <= KMX_ALIGN_MAX_READ && s <= e && e <= S.n && d <= KMX_ALIGN_MAX_EDITS)) return en;
    en.m = uint32_t(r1 - r0);
    en.L = e - s;
    const uint32_t gap = en.m > en.L ? en.m - en.L : en.L - en.m;
    en.ok = gap <= d && (en.m > 0 || en.L == d);               // (the empty read: H[0][L] = L)
    return en;
}

__device__ __forceinline__ uint32_t class_of(uint32_t d) { return d < 32 ? 0u : d < 64 ? 1u : d < 128 ? 2u : 3u; }   // 64 << class >= 2d + 1

// The letters of an entry into LDS by one wave: s_q[m] from the reads, s_t[L] from the packed copy of the text, one 64-bit word per
// lane at a time.  The caller synchronises.
__device__ __forceinline__ void stage_entry(const ScriptIn& S, const Entry& en, uint32_t lane, uint8_t* s_q, uint8_t* s_t)
{
    const uint32_t m = en.m, L = en.L;
    for (uint32_t i = lane; i < m; i += kWave) s_q[i] = S.ranks[en.r0 + i];
    if (L) {
        const uint32_t w = S.w, per = 64 / w;
        const uint64_t mask = (uint64_t(1) << w) - 1;          // (w <= 8)
        const uint64_t lo = en.start, hi = lo + L;
        for (uint64_t wi = lo / per + lane; wi <= (hi - 1) / per; wi += kWave) {
            const uint64_t word = S.text[wi];
            for (uint32_t k = 0; k < per; ++k) {
                const uint64_t p = wi * per + k;
                if (p >= lo && p < hi) s_t[p - lo] = uint8_t((word >> (k * w)) & mask);
            }
        }
    }
}

// ctr[CTR_CUT] = the end of the chunk that starts at e0: the most entries whose codes fit `cap` bytes (clamped up to the largest
// entry of the batch, so a chunk never is empty)
__global__ void k_script_cut(const uint64_t* __restrict__ code_off, uint64_t e0, uint64_t cap, unsigned long long* __restrict__ ctr)
{
    const uint64_t n_sel = ctr[CTR_N_SEL];
    cap = max(cap, uint64_t(ctr[CTR_MAX_CODE]));
    uint64_t lo = min(e0, n_sel), hi = min(n_sel, lo + kMaxChunk);   // the largest e in [lo, hi] with code_off[e] - code_off[e0] <= cap
    const uint64_t base = code_off[lo];
    while (lo < hi) {
        const uint64_t mid = (lo + hi + 1) >> 1;
        if (code_off[mid] - base <= cap) lo = mid; else hi = mid - 1;
    }
    ctr[CTR_CUT] = lo;
}

inline hipError_t ensure_exact(kmx::Buf& b, size_t bytes)      // (Buf::ensure leaves headroom; the arena keeps to its bound)
{
    if (bytes <= b.cap) return hipSuccess;
    b.release();
    hipError_t e = hipMalloc(&b.p, bytes);
    if (e != hipSuccess) { b.p = nullptr; return e; }
    b.cap = bytes;
    return hipSuccess;
}

} // namespace
