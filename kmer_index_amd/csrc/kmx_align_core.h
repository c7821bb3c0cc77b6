// What the bit-vector alignments share (kmx_align.hip: kmx_loci_align; kmx_rescue.hip: kmx_pairs_rescue): the reads as the kernels see
// them, the match tables and one column of the block recurrence.  Private to those two translation units: everything lives in
// the unnamed namespace of the unit that includes it, like the kernels that use it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kmx_handle.h"

namespace {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kWave = 64;
constexpr uint32_t kAlignBlock = 64;      // a wave per workgroup in the passes: the lanes run loops of different length
constexpr int kClasses = 5;               // NW = 1, 2, 4, 8, 16
constexpr uint8_t CLS_OUT = 255;          // a locus that no pass looks at (skipped, or an empty read)

// what every kernel reads
struct AlignIn {
    const uint8_t* ranks;
    const uint64_t* roff;          // [nr + 1]
    uint64_t ranks_len;            // letters that may be read (host form: roff[nr]; device form: no bound of ours)
    const uint64_t* locus_off;     // [nr + 1]
    const int64_t* diag;
    const uint32_t* span;
    uint64_t nr, n_loci, n;
    const uint64_t* text;          // packed at w bits per letter
    uint32_t w, sigma, max_edits, max_span;
    const uint64_t* ctg_off;       // [nc + 1]: the index's contig table; nullptr without one (kmx_loci_align only)
    const uint32_t* ctg;           // [n_loci]: the contig of every locus, as k_align_classify stored it; nullptr without a table
    uint64_t nc;
};

constexpr uint32_t kNoContig = 0xFFFFFFFFu;

// letters of read r, 0 when the read is not served: empty, longer than KMX_ALIGN_MAX_READ or outside the letters that may be read
// (*too_long tells the last two from the first)
__device__ __forceinline__ uint32_t read_letters(const AlignIn& A, uint64_t r, uint64_t* r0_out, bool* too_long)
{
    const uint64_t r0 = A.roff[r], r1 = A.roff[r + 1];
    *r0_out = r0;
    const bool ok = r1 >= r0 && r1 <= A.ranks_len && r1 - r0 <= KMX_ALIGN_MAX_READ;
    *too_long = !ok;
    return ok ? uint32_t(r1 - r0) : 0u;
}

__device__ __forceinline__ uint32_t class_of(uint32_t nw) { return nw <= 1 ? 0u : nw <= 2 ? 1u : nw <= 4 ? 2u : nw <= 8 ? 3u : 4u; }

// ---- the match tables ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_align_count(AlignIn A, uint32_t* __restrict__ pcnt)
{
    const uint64_t r = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (r >= A.nr) return;
    uint64_t r0;
    bool too_long;
    const uint32_t m = read_letters(A, r, &r0, &too_long);
    const bool has_loci = A.locus_off[r + 1] > A.locus_off[r];  // (a read without loci needs no tables)
    pcnt[r] = has_loci ? A.sigma * ((m + 63) / 64) : 0u;
}

// thread t owns word t of the forward table and of the reverse table (the second half of peq)
__global__ __launch_bounds__(kBlock) void k_align_peq(AlignIn A, const uint64_t* __restrict__ peq_off, uint64_t n_words, uint64_t* __restrict__ peq)
{
    const uint64_t t = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (t >= n_words) return;
    uint64_t lo = 0, hi = A.nr;                                // the last read whose table starts at or before t (it has one)
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (peq_off[mid] <= t) lo = mid; else hi = mid;
    }
    uint64_t r0;
    bool too_long;
    const uint32_t m = read_letters(A, lo, &r0, &too_long);
    const uint32_t nw = (m + 63) / 64;
    const uint64_t rem = t - peq_off[lo];
    if (nw == 0 || rem >= uint64_t(A.sigma) * nw) return;      // (cannot happen: the scan counted these very words)
    const uint32_t c = uint32_t(rem / nw), b = uint32_t(rem % nw);
    const uint8_t* q = A.ranks + r0;
    uint64_t fw = 0, rv = 0;
    const uint32_t i0 = b * 64, i1 = min(i0 + 64, m);
    for (uint32_t i = i0; i < i1; ++i) {
        fw |= uint64_t(q[i] == c) << (i - i0);
        rv |= uint64_t(q[m - 1 - i] == c) << (i - i0);
    }
    peq[t] = fw;
    peq[n_words + t] = rv;
}

// ---- the recurrence ------------------------------------------------------------------------------------------------------------------
// One column of the block recurrence over NW words: eq(b) is the match word of the column's letter, (hp, hm) the horizontal delta
// that enters word 0 (+1, -1 or neither).  Returns the delta of the score row: bit `lastbit` of word `lastw`.
template <int NW, typename Eq>
__device__ __forceinline__ int column(uint64_t (&Pv)[NW], uint64_t (&Mv)[NW], Eq eq, uint64_t hp, uint64_t hm, uint32_t lastw, uint32_t lastbit)
{
    uint64_t ph_last = 0, mh_last = 0;
#pragma unroll
    for (int b = 0; b < NW; ++b) {
        uint64_t e = eq(b);
        const uint64_t pv = Pv[b], mv = Mv[b];
        const uint64_t xv = e | mv;
        e |= hm;
        const uint64_t xh = (((e & pv) + pv) ^ pv) | e;
        uint64_t ph = mv | ~(xh | pv);
        uint64_t mh = pv & xh;
        if (uint32_t(b) == lastw) { ph_last = ph; mh_last = mh; }
        const uint64_t op = ph >> 63, om = mh >> 63;
        ph = (ph << 1) | hp;
        mh = (mh << 1) | hm;
        Pv[b] = mh | ~(xv | ph);
        Mv[b] = ph & xv;
        hp = op;
        hm = om;
    }
    return int((ph_last >> lastbit) & 1) - int((mh_last >> lastbit) & 1);
}

} // namespace
