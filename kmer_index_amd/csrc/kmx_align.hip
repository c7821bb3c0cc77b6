// Alignment at the voted loci (kmx_loci_align, include/kmx.h): every read against the text around each of its loci, semi-global
// edit distance by Myers' bit-vector recurrence in its block form (Hyyro), one thread per locus.
//
//   k_align_count      a thread per read: the words of its two match tables (sigma * ceil(m / 64), 0 for a read that is not served
//                      or has no locus)
//   k_align_peq        a thread per table word: bit i of Peq[read][letter][word] = (q[64 * word + i] == letter), and the same for the
//                      reversed read; letters >= sigma set no bit
//   k_align_classify   a thread per locus: its read (binary search of locus_off), skipped or not, its class NW in {1, 2, 4, 8, 16}
//                      (the smallest that holds the read), counted per class; when the index has a contig table (KMX_MAP_CONTIGS), the
//                      contig of the locus, found once by binary search and kept in ctg[] for the passes and the later stages
//   k_align_place      the loci of every class listed together (a workgroup reserves its part of each class with one atomic)
//   k_align_fwd<NW>    forward pass over T = text[lo, hi): carry-in 0 (the alignment may start anywhere), the score followed at bit
//                      (m - 1) % 64 of word (m - 1) / 64, the minimum and the first column that reaches it kept; loci with d <= E are
//                      listed for the reverse pass
//   k_align_rev<NW>    the same recurrence on the reversed read and the text read backwards from `end`, carry-in +1 (anchored): stops
//                      at the first column whose score equals d
//   k_align_best       a wave per read: aligned[r], best[r]; the batch totals
// k_align_count, k_align_peq and the column of the recurrence live in kmx_align_core.h, which kmx_rescue.hip shares.
// Pv / Mv live in registers under compile-time indices; the words of a class beyond the read's own get Eq = 0 and are never looked
// at (carries only travel upwards).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "kmx_approx.h"
#include "kmx_align_core.h"
#include "kmx_kernels.h"
#include "kmx_vote.h"

namespace {

enum { CTR_CLASS = 0, CTR_ALIGNED_CLASS = kClasses, CTR_CURSOR = 2 * kClasses, CTR_N_ALIGNED = 3 * kClasses, CTR_N_SKIPPED, CTR_PEQ_WORDS, CTR_COUNT };

using kmx::Buf;
using Pinned = kmx::PinnedArr;
using kmx::grid_for;

// T = text[lo, hi) of a locus (kmx.h), inside contig c of the index's table or, when c names none, inside the text; lo <= hi <= n
__device__ __forceinline__ void text_window(const AlignIn& A, uint32_t c, int64_t D, uint32_t S, uint32_t m, uint64_t* lo, uint64_t* hi)
{
    const int64_t n = int64_t(A.n), E = int64_t(A.max_edits);
    int64_t b0 = 0, b1 = n;
    if (A.ctg_off && c < A.nc) {                               // (uniform across the wave: a batch has a table or has none)
        b1 = min(int64_t(A.ctg_off[c + 1]), n);
        b0 = min(int64_t(A.ctg_off[c]), b1);
    }
    const int64_t l = min(max(b0, D - E), b1);                 // (diagonals of a vote lie below n: without a table the second bound never binds)
    const int64_t h = max(l, min(b1, D + int64_t(S) + int64_t(m) + E));
    *lo = uint64_t(l);
    *hi = uint64_t(h);
}

// c(l) of kmx.h: the contig that holds the middle of the locus's band, by binary search of the table (nc >= 1, n >= 1)
__device__ __forceinline__ uint32_t contig_of(const AlignIn& A, int64_t D, uint32_t S, uint32_t m)
{
    const int64_t mid = min(max(D + int64_t((uint64_t(S) + m) / 2), int64_t(0)), int64_t(A.n) - 1);
    uint64_t lo = 0, hi = A.nc;                                // the last contig that starts at or before mid
    while (hi - lo > 1) {
        const uint64_t c = (lo + hi) >> 1;
        if (int64_t(A.ctg_off[c]) <= mid) lo = c; else hi = c;
    }
    return uint32_t(lo);
}

// ---- classes -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_align_classify(AlignIn A, uint32_t* __restrict__ lread, uint8_t* __restrict__ cls,
                                                           uint8_t* __restrict__ dist, uint32_t* __restrict__ start, uint32_t* __restrict__ end,
                                                           uint32_t* __restrict__ ctg, unsigned long long* __restrict__ ctr)
{
    __shared__ uint32_t s_cnt[kClasses];
    if (threadIdx.x < kClasses) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t l = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (l < A.n_loci) {
        uint64_t lo = 0, hi = A.nr;                            // the last read whose loci start at or before l
        while (hi - lo > 1) {
            const uint64_t mid = (lo + hi) >> 1;
            if (A.locus_off[mid] <= l) lo = mid; else hi = mid;
        }
        uint64_t r0;
        bool too_long;
        const uint32_t m = read_letters(A, lo, &r0, &too_long);
        const uint32_t S = A.span[l];
        uint8_t c = CLS_OUT, d = KMX_ALIGN_SKIPPED;
        uint32_t at = 0, cg = kNoContig;
        if (S <= A.max_span && !too_long) {
            if (ctg) cg = contig_of(A, A.diag[l], S, m);       // (with a table: found once, the passes read it back)
            if (m == 0) {                                      // the empty read aligns with the empty substring at lo
                uint64_t tlo, thi;
                text_window(A, cg, A.diag[l], S, 0, &tlo, &thi);
                d = 0;
                at = uint32_t(tlo);
            } else {
                c = uint8_t(class_of((m + 63) / 64));
                d = KMX_ALIGN_NONE;
                atomicAdd(&s_cnt[c], 1u);
            }
        }
        lread[l] = uint32_t(lo);
        cls[l] = c;
        dist[l] = d;                                           // (the forward pass overwrites the loci it aligns)
        start[l] = at;
        end[l] = at;
        if (ctg) ctg[l] = cg;
    }
    __syncthreads();
    if (threadIdx.x < kClasses && s_cnt[threadIdx.x]) atomicAdd(&ctr[CTR_CLASS + threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
}

struct ClassBase { uint64_t at[kClasses]; };

__global__ __launch_bounds__(kBlock) void k_align_place(uint64_t n_loci, const uint8_t* __restrict__ cls, ClassBase base,
                                                        unsigned long long* __restrict__ ctr, uint32_t* __restrict__ list)
{
    __shared__ uint32_t s_cnt[kClasses];
    __shared__ unsigned long long s_base[kClasses];
    if (threadIdx.x < kClasses) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t l = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    const uint8_t c = l < n_loci ? cls[l] : CLS_OUT;
    uint32_t rank = 0;
    if (c < kClasses) rank = atomicAdd(&s_cnt[c], 1u);
    __syncthreads();
    if (threadIdx.x < kClasses && s_cnt[threadIdx.x])
        s_base[threadIdx.x] = base.at[threadIdx.x] + atomicAdd(&ctr[CTR_CURSOR + threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
    __syncthreads();
    if (c < kClasses) list[s_base[c] + rank] = uint32_t(l);
}


struct PassIn {
    const uint32_t* lread;
    const uint64_t* peq_off;
    const uint64_t* peq;           // the table of this pass (forward, or the reversed reads')
};

template <int NW>
__global__ __launch_bounds__(kAlignBlock) void k_align_fwd(AlignIn A, PassIn P, const uint32_t* __restrict__ list, uint64_t cnt,
                                                           uint8_t* __restrict__ dist, uint32_t* __restrict__ start, uint32_t* __restrict__ end,
                                                           uint32_t* __restrict__ alist, unsigned long long* __restrict__ acnt)
{
    const uint64_t i = uint64_t(blockIdx.x) * kAlignBlock + threadIdx.x;
    if (i >= cnt) return;
    const uint32_t l = list[i];
    const uint64_t r = P.lread[l];
    uint64_t r0;
    bool too_long;
    const uint32_t m = read_letters(A, r, &r0, &too_long);
    const uint32_t nw = (m + 63) / 64;
    if (m == 0 || nw > uint32_t(NW)) return;                    // (cannot happen: k_align_classify read the same offsets)
    uint64_t lo, hi;
    text_window(A, A.ctg ? A.ctg[l] : kNoContig, A.diag[l], A.span[l], m, &lo, &hi);
    const uint64_t* pq = P.peq + P.peq_off[r];
    const uint32_t lastw = (m - 1) >> 6, lastbit = (m - 1) & 63;
    const uint32_t w = A.w, per = 64 / w, sigma = A.sigma;
    const uint64_t mask = (uint64_t(1) << w) - 1;               // (w <= 8)
    uint64_t Pv[NW], Mv[NW];
#pragma unroll
    for (int b = 0; b < NW; ++b) { Pv[b] = ~uint64_t(0); Mv[b] = 0; }
    uint32_t score = m, best = m;
    uint64_t best_at = lo;
    uint64_t word = lo < hi ? A.text[lo / per] : 0;
    for (uint64_t p = lo; p < hi; ++p) {
        const uint32_t k = uint32_t(p % per);
        if (k == 0) word = A.text[p / per];
        const uint32_t c = uint32_t((word >> (k * w)) & mask);
        const uint64_t* row = pq + uint64_t(c) * nw;
        const bool known = c < sigma;
        score += column<NW>(Pv, Mv, [&](int b) { return known && uint32_t(b) < nw ? row[b] : uint64_t(0); }, 0, 0, lastw, lastbit);
        if (score < best) { best = score; best_at = p + 1; }
    }
    if (best > A.max_edits) return;                             // dist[l] is KMX_ALIGN_NONE already
    dist[l] = uint8_t(best);
    end[l] = uint32_t(best_at);
    start[l] = uint32_t(best_at);                               // (the reverse pass moves it when best < m)
    if (best < m) alist[atomicAdd(acnt, 1ull)] = l;            // best == m: the empty substring at lo, there is nothing to walk back
}

template <int NW>
__global__ __launch_bounds__(kAlignBlock) void k_align_rev(AlignIn A, PassIn P, const uint32_t* __restrict__ alist,
                                                           const unsigned long long* __restrict__ acnt, const uint8_t* __restrict__ dist,
                                                           uint32_t* __restrict__ start, const uint32_t* __restrict__ end)
{
    const uint64_t i = uint64_t(blockIdx.x) * kAlignBlock + threadIdx.x;
    if (i >= *acnt) return;
    const uint32_t l = alist[i];
    const uint64_t r = P.lread[l];
    uint64_t r0;
    bool too_long;
    const uint32_t m = read_letters(A, r, &r0, &too_long);
    const uint32_t nw = (m + 63) / 64;
    if (m == 0 || nw > uint32_t(NW)) return;
    uint64_t lo, hi;
    text_window(A, A.ctg ? A.ctg[l] : kNoContig, A.diag[l], A.span[l], m, &lo, &hi);
    const uint64_t e = min(uint64_t(end[l]), hi);               // (end lies in [lo, hi]: the forward pass wrote it)
    const uint32_t d = dist[l];
    const uint64_t* pq = P.peq + P.peq_off[r];
    const uint32_t lastw = (m - 1) >> 6, lastbit = (m - 1) & 63;
    const uint32_t w = A.w, per = 64 / w, sigma = A.sigma;
    const uint64_t mask = (uint64_t(1) << w) - 1;
    uint64_t Pv[NW], Mv[NW];
#pragma unroll
    for (int b = 0; b < NW; ++b) { Pv[b] = ~uint64_t(0); Mv[b] = 0; }
    uint32_t score = m;
    uint64_t p = e;
    uint64_t word = p > lo ? A.text[(p - 1) / per] : 0;
    while (score != d && p > lo) {
        --p;
        const uint32_t k = uint32_t(p % per);
        if (k == per - 1) word = A.text[p / per];
        const uint32_t c = uint32_t((word >> (k * w)) & mask);
        const uint64_t* row = pq + uint64_t(c) * nw;
        const bool known = c < sigma;
        score += column<NW>(Pv, Mv, [&](int b) { return known && uint32_t(b) < nw ? row[b] : uint64_t(0); }, 1, 0, lastw, lastbit);
    }
    start[l] = uint32_t(p);
}

// ---- per read ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_align_best(uint64_t nr, const uint64_t* __restrict__ locus_off, const uint8_t* __restrict__ dist,
                                                       uint32_t max_edits, uint32_t* __restrict__ best, uint32_t* __restrict__ aligned,
                                                       unsigned long long* __restrict__ ctr)
{
    __shared__ unsigned long long s_al, s_sk;
    if (threadIdx.x == 0) { s_al = 0; s_sk = 0; }
    __syncthreads();
    const uint32_t lane = threadIdx.x % kWave;
    const uint64_t r = uint64_t(blockIdx.x) * (kBlock / kWave) + threadIdx.x / kWave;
    if (r < nr) {
        const uint64_t a = locus_off[r], b = locus_off[r + 1];
        uint32_t al = 0, sk = 0;
        uint64_t key = ~uint64_t(0);                            // (dist, index in the read)
        for (uint64_t l = a + lane; l < b; l += kWave) {
            const uint32_t d = dist[l];
            if (d <= max_edits) { ++al; key = min(key, (uint64_t(d) << 32) | uint64_t(min(l - a, uint64_t(0xFFFFFFFEu)))); }
            else if (d == KMX_ALIGN_SKIPPED) ++sk;
        }
        for (int off = kWave / 2; off > 0; off >>= 1) {
            al += __shfl_xor(al, off);
            sk += __shfl_xor(sk, off);
            key = min(key, (uint64_t)__shfl_xor((unsigned long long)key, off));
        }
        if (lane == 0) {
            aligned[r] = al;
            best[r] = al ? uint32_t(key) : 0xFFFFFFFFu;
            if (al) atomicAdd(&s_al, (unsigned long long)al);
            if (sk) atomicAdd(&s_sk, (unsigned long long)sk);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_al) atomicAdd(&ctr[CTR_N_ALIGNED], s_al);
        if (s_sk) atomicAdd(&ctr[CTR_N_SKIPPED], s_sk);
    }
}

} // namespace

struct kmx_alignments {
    int device = 0;
    hipStream_t stream = nullptr;          // the stream of the call that filled the handle (the host view copies on it)
    uint64_t nr = 0, n_loci = 0, n_aligned = 0, n_skipped = 0;
    uint64_t nc = 0, ctg_gen = 0;          // the contig table of the index the call saw: its contigs (0: none) and its generation
    // results; best and aligned are handed out whatever the handle holds; ctg is only filled when nc > 0 and has a pair of views of its own
    kmx::ArrOf<uint8_t> dist;
    kmx::ArrOf<uint32_t> start, end, best, aligned, ctg{kmx::ARR_OWN_VIEW};
    // scratch
    Buf ranks, roff, pcnt, peq_off, bsum, peq, lread, cls, list, alist, ctr;
    Pinned h_ctr;
    bool host_valid = false, host_ctg_valid = false;
    std::vector<kmx::Arr*> results() { return {&dist, &start, &end, &best, &aligned, &ctg}; }
    std::vector<Buf*> scratch() { return {&ranks, &roff, &pcnt, &peq_off, &bsum, &peq, &lread, &cls, &list, &alist, &ctr}; }
    void release() { kmx::release_arrays(*this); }
    void clear() { nr = n_loci = n_aligned = n_skipped = nc = ctg_gen = 0; kmx::clear_arrays(*this); host_ctg_valid = false; }
};

kmx::AlignAccess kmx::alignments_access(const kmx_alignments* a)
{
    return AlignAccess{a->device, a->stream, a->nr, a->n_loci, a->dist.as<uint8_t>(), a->start.as<uint32_t>(), a->end.as<uint32_t>(),
                       a->best.as<uint32_t>(), a->ctg.dev(), a->nc, a->ctg_gen};
}

namespace {

template <int NW>
void launch_passes(hipStream_t s, const AlignIn& A, const PassIn& F, const PassIn& R, const uint32_t* list, uint32_t* alist, uint64_t cnt,
                   unsigned long long* acnt, kmx_alignments* a)
{
    const dim3 grid(grid_for(cnt, kAlignBlock)), block(kAlignBlock);
    hipLaunchKernelGGL(k_align_fwd<NW>, grid, block, 0, s, A, F, list, cnt, a->dist.as<uint8_t>(), a->start.as<uint32_t>(), a->end.as<uint32_t>(),
                       alist, acnt);
    hipLaunchKernelGGL(k_align_rev<NW>, grid, block, 0, s, A, R, alist, acnt, a->dist.as<uint8_t>(), a->start.as<uint32_t>(), a->end.as<uint32_t>());
}

// d_ranks / d_roff: the reads on the device of the loci; ranks_len: the letters that may be read
kmx_status align_run(const kmx::IndexAccess& X, const kmx::LociAccess& L, const void* d_ranks, const void* d_roff, uint64_t ranks_len,
                     const kmx_align_options& o, hipStream_t s, kmx_alignments* a)
{
    const uint64_t nr = L.nr, nl = L.n_loci;
    a->nc = X.ctg_off ? X.nc : 0;
    a->ctg_gen = X.ctg_gen;
    TRY_HIP(a->best.ensure(std::max<uint64_t>(nr, 1) * 4));
    TRY_HIP(a->aligned.ensure(std::max<uint64_t>(nr, 1) * 4));
    a->nr = a->best.n = a->aligned.n = nr;
    if (nr == 0) return KMX_OK;
    if (nl == 0) {                                             // no locus: no launch indexes an empty array
        TRY_HIP(hipMemsetAsync(a->best.p, 0xFF, nr * 4, s));
        TRY_HIP(hipMemsetAsync(a->aligned.p, 0, nr * 4, s));
        return KMX_OK;
    }
    if (nl > 0xFFFFFFFFull) return kmx::set_error(KMX_ERR_TOO_LARGE, "kmx_loci_align: 2^32 or more loci: split the reads");
    TRY_KMX(kmx::ensure_text(X, s));
    TRY_HIP(a->dist.ensure(nl));
    TRY_HIP(a->start.ensure(nl * 4));
    TRY_HIP(a->end.ensure(nl * 4));
    TRY_HIP(a->lread.ensure(nl * 4));
    TRY_HIP(a->cls.ensure(nl));
    if (a->nc) TRY_HIP(a->ctg.ensure(nl * 4));
    uint32_t* ctg = a->nc ? a->ctg.as<uint32_t>() : nullptr;
    TRY_HIP(a->pcnt.ensure(nr * 4 + 16));
    TRY_HIP(a->peq_off.ensure((nr + 1) * 8));
    TRY_HIP(a->bsum.ensure(kmx::scan_blocks(nr) * 8 + 16));
    TRY_HIP(a->ctr.ensure(CTR_COUNT * 8));
    unsigned long long* ctr = a->ctr.as<unsigned long long>();
    TRY_HIP(hipMemsetAsync(ctr, 0, CTR_COUNT * 8, s));
    const AlignIn A{static_cast<const uint8_t*>(d_ranks), static_cast<const uint64_t*>(d_roff), ranks_len, L.locus_off, L.diag, L.span, nr, nl, X.n,
                    X.text->d_words, X.text->w, X.sigma, o.max_edits, o.max_span, a->nc ? X.ctg_off : nullptr, ctg, a->nc};
    hipLaunchKernelGGL(k_align_count, dim3(grid_for(nr, kBlock)), dim3(kBlock), 0, s, A, a->pcnt.as<uint32_t>());
    kmx::launch_scan(s, a->pcnt.as<uint32_t>(), nr, a->bsum.as<uint64_t>(), a->peq_off.as<uint64_t>(), ctr + CTR_PEQ_WORDS);
    hipLaunchKernelGGL(k_align_classify, dim3(grid_for(nl, kBlock)), dim3(kBlock), 0, s, A, a->lread.as<uint32_t>(), a->cls.as<uint8_t>(),
                       a->dist.as<uint8_t>(), a->start.as<uint32_t>(), a->end.as<uint32_t>(), ctg, ctr);
    TRY_HIP(hipGetLastError());
    TRY_KMX(kmx::read_back("kmx_loci_align", s, ctr, a->h_ctr, CTR_COUNT * 8));
    uint64_t c[CTR_COUNT];
    std::memcpy(c, a->h_ctr.p, sizeof c);
    ClassBase base{};
    uint64_t listed = 0;
    for (int k = 0; k < kClasses; ++k) { base.at[k] = listed; listed += c[CTR_CLASS + k]; }
    if (listed > nl) return kmx::set_error(KMX_ERR_HIP, "kmx_loci_align: the class counts exceed the loci");     // (never: a guard for the lists)
    if (listed) {
        const uint64_t n_words = c[CTR_PEQ_WORDS];
        TRY_HIP(a->peq.ensure(std::max<uint64_t>(n_words, 1) * 16));
        TRY_HIP(a->list.ensure(listed * 4));
        TRY_HIP(a->alist.ensure(listed * 4));
        if (n_words)
            hipLaunchKernelGGL(k_align_peq, dim3(grid_for(n_words, kBlock)), dim3(kBlock), 0, s, A, a->peq_off.as<uint64_t>(), n_words, a->peq.as<uint64_t>());
        hipLaunchKernelGGL(k_align_place, dim3(grid_for(nl, kBlock)), dim3(kBlock), 0, s, nl, a->cls.as<uint8_t>(), base, ctr, a->list.as<uint32_t>());
        const PassIn F{a->lread.as<uint32_t>(), a->peq_off.as<uint64_t>(), a->peq.as<uint64_t>()};
        const PassIn R{a->lread.as<uint32_t>(), a->peq_off.as<uint64_t>(), a->peq.as<uint64_t>() + n_words};
        for (int k = 0; k < kClasses; ++k) {
            const uint64_t cnt = c[CTR_CLASS + k];
            if (!cnt) continue;
            const uint32_t* list = a->list.as<uint32_t>() + base.at[k];
            uint32_t* alist = a->alist.as<uint32_t>() + base.at[k];
            unsigned long long* acnt = ctr + CTR_ALIGNED_CLASS + k;
            switch (k) {
            case 0: launch_passes<1>(s, A, F, R, list, alist, cnt, acnt, a); break;
            case 1: launch_passes<2>(s, A, F, R, list, alist, cnt, acnt, a); break;
            case 2: launch_passes<4>(s, A, F, R, list, alist, cnt, acnt, a); break;
            case 3: launch_passes<8>(s, A, F, R, list, alist, cnt, acnt, a); break;
            default: launch_passes<16>(s, A, F, R, list, alist, cnt, acnt, a); break;
            }
        }
    }
    hipLaunchKernelGGL(k_align_best, dim3(grid_for(nr, kBlock / kWave)), dim3(kBlock), 0, s, nr, L.locus_off, a->dist.as<uint8_t>(), o.max_edits,
                       a->best.as<uint32_t>(), a->aligned.as<uint32_t>(), ctr);
    TRY_HIP(hipGetLastError());
    TRY_KMX(kmx::read_back("kmx_loci_align", s, ctr, a->h_ctr, CTR_COUNT * 8));
    a->n_loci = nl;
    kmx::expose({&a->dist, &a->start, &a->end}, nl);
    if (a->nc) a->ctg.n = nl;
    a->n_aligned = a->h_ctr.as<uint64_t>()[CTR_N_ALIGNED];
    a->n_skipped = a->h_ctr.as<uint64_t>()[CTR_N_SKIPPED];
    return KMX_OK;
}

kmx_status check_front(const char* fn, const kmx_index* index, const kmx_loci* loci, const void* roff, const kmx_align_options* o,
                       kmx_alignments** inout)
{
    const std::string who = std::string(fn) + ": ";
    if (!index) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "index is NULL");
    if (!loci) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "loci handle is NULL");
    if (!o) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "options is NULL");
    if (!inout) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "inout is NULL");
    if (!roff) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "roff is NULL");
    if (o->struct_size < sizeof(kmx_align_options)) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "options->struct_size is too small");
    if (o->flags != 0) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "flags must be 0");
    if (o->max_edits > KMX_ALIGN_MAX_EDITS) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "max_edits > KMX_ALIGN_MAX_EDITS");
    return KMX_OK;
}

// host == true: ranks / roff are host arrays that go up on the stream of the vote; else device arrays and the caller's stream
kmx_status align_call(const char* fn, const kmx_index* index, const kmx_loci* loci, const void* ranks, const void* roff, uint64_t nr,
                      const kmx_align_options* o, bool host, hipStream_t stream, kmx_alignments** inout)
{
    TRY_KMX(check_front(fn, index, loci, roff, o, inout));
    const std::string who = std::string(fn) + ": ";
    const kmx::LociAccess L = kmx::loci_access(loci);
    kmx_alignments* a = *inout;
    auto refuse = kmx::refuser(who, a);
    if (nr != L.nr) return refuse(KMX_ERR_INVALID_ARGUMENT, "nr differs from the loci handle's");
    kmx::IndexAccess X{};
    kmx_status no_st;
    std::string no_index;
    if (!kmx::index_for(index, L.device, "the loci", &X, &no_st, &no_index)) return refuse(no_st, no_index);
    uint64_t n_letters = ~uint64_t(0);
    if (host) {
        const char* why = kmx::check_host_reads(ranks, static_cast<const uint64_t*>(roff), nr, &n_letters);
        if (why) return refuse(KMX_ERR_INVALID_ARGUMENT, why);
    }
    kmx::DeviceGuard dg;
    TRY_KMX(kmx::bind_handle(inout, L.device));
    a = *inout;
    hipStream_t s = host ? L.stream : stream;
    const kmx_status st = kmx::run_into(a, s, [&] {
        const void* d_ranks = ranks;
        const void* d_roff = roff;
        if (host && nr && L.n_loci) {
            TRY_KMX(kmx::upload_reads(ranks, roff, nr, n_letters, a->ranks, a->roff, s));
            d_ranks = a->ranks.p;
            d_roff = a->roff.p;
        }
        return align_run(X, L, d_ranks, d_roff, n_letters, *o, s, a);
    });
    if (host && st == KMX_OK) (void)hipStreamSynchronize(s);   // the caller's arrays are free again
    return st;
}

} // namespace

extern "C" {

kmx_status kmx_loci_align(const kmx_index* index, const kmx_loci* loci, const uint8_t* ranks, const uint64_t* roff, uint64_t nr,
                          const kmx_align_options* options, kmx_alignments** inout)
{
    return align_call("kmx_loci_align", index, loci, ranks, roff, nr, options, true, nullptr, inout);
}

kmx_status kmx_loci_align_device(const kmx_index* index, const kmx_loci* loci, const void* d_ranks, const void* d_roff, uint64_t nr,
                                 const kmx_align_options* options, void* stream, kmx_alignments** inout)
{
    return align_call("kmx_loci_align_device", index, loci, d_ranks, d_roff, nr, options, false, static_cast<hipStream_t>(stream), inout);
}

kmx_status kmx_alignments_counts(const kmx_alignments* a, uint64_t* nr, uint64_t* n_loci, uint64_t* n_aligned, uint64_t* n_skipped)
{
    if (!a) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_alignments_counts: alignments handle is NULL");
    if (nr) *nr = a->nr;
    if (n_loci) *n_loci = a->n_loci;
    if (n_aligned) *n_aligned = a->n_aligned;
    if (n_skipped) *n_skipped = a->n_skipped;
    return KMX_OK;
}

kmx_status kmx_alignments_view_device(const kmx_alignments* a, const uint8_t** d_dist, const uint32_t** d_start, const uint32_t** d_end,
                                      const uint32_t** d_best, const uint32_t** d_aligned)
{
    if (!a) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_alignments_view_device: alignments handle is NULL");
    if (d_dist) *d_dist = a->dist.dev();
    if (d_start) *d_start = a->start.dev();
    if (d_end) *d_end = a->end.dev();
    if (d_best) *d_best = a->best.as<uint32_t>();
    if (d_aligned) *d_aligned = a->aligned.as<uint32_t>();
    return KMX_OK;
}

kmx_status kmx_alignments_view(kmx_alignments* a, const uint8_t** dist, const uint32_t** start, const uint32_t** end, const uint32_t** best,
                               const uint32_t** aligned)
{
    if (!a) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_alignments_view: alignments handle is NULL");
    TRY_KMX(kmx::host_view("kmx_alignments_view", *a));
    if (dist) *dist = a->dist.host();
    if (start) *start = a->start.host();
    if (end) *end = a->end.host();
    if (best) *best = a->best.host();
    if (aligned) *aligned = a->aligned.host();
    return KMX_OK;
}

kmx_status kmx_alignments_contigs_view_device(const kmx_alignments* a, const uint32_t** d_ctg, uint64_t* nc)
{
    if (!a) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_alignments_contigs_view_device: alignments handle is NULL");
    if (d_ctg) *d_ctg = a->ctg.dev();
    if (nc) *nc = a->nc;
    return KMX_OK;
}

kmx_status kmx_alignments_contigs_view(kmx_alignments* a, const uint32_t** ctg, uint64_t* nc)
{
    if (!a) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_alignments_contigs_view: alignments handle is NULL");
    if (nc) *nc = a->nc;
    if (!a->nc) {                                              // made without a table: no array
        if (ctg) *ctg = nullptr;
        return KMX_OK;
    }
    if (!a->host_ctg_valid) {                                  // 4 bytes per locus
        TRY_KMX(kmx::copy_to_host("kmx_alignments_contigs_view", a->device, a->stream, {&a->ctg}));
        a->host_ctg_valid = true;
    }
    if (ctg) *ctg = a->ctg.host();
    return KMX_OK;
}

void kmx_alignments_free(kmx_alignments* a) { kmx::free_handle(a); }

} // extern "C"
