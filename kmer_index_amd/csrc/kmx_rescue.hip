// Mate rescue of the read-mapping chain (kmx_pairs_rescue, kmx_rescues_scripts; include/kmx.h, KMX_PAIR_RESCUE).  A mate without an
// intact seed window casts no vote and gets no locus, although its placed partner pins it to an insert window of the text.  The
// rescue aligns such a mate against that window directly, without seeds, by the recurrence of kmx_loci_align (kmx_align_core.h), and
// where the alignment is concordant with the partner's it rewrites the placements and the pairs in place.
//
//   k_rescue_plan      a thread per internal read: 1 when the read is the looked-for strand of a mate that has a job
//                      (kmx::launch_scan over the flags gives job_off)
//   k_rescue_jobs      a thread per internal read: the record of its job (read, window, served or not, the class NW in
//                      {1, 2, 4, 8, 16} as k_align_classify has it), the jobs per class, best[] of the scripts cleared
//                      (k_align_count and k_align_peq of kmx_align_core.h then make the match tables of the job reads only)
//   k_rescue_fwd<NW>   a thread per (job, segment): segment g owns the end columns (lo + g G, lo + (g + 1) G]; it starts with a fresh
//                      state m + E columns earlier (clamped at lo), follows the score everywhere but looks at it only inside its
//                      own range, and leaves (dist << 32 | end) through one 64-bit atomicMin on the job's key.  A thread of
//                      another class leaves at once (the jobs are few: they are not listed by class)
//   k_rescue_rev<NW>   a thread per found job: the anchored pass of k_align_rev from `end`; writes dist / start / end of the job
//   k_rescue_fold      a wave per pair: the concordance test of k_pair_fold on (anchor, rescued mate), the choice, the lanes striding
//                      over the rescued read's loci for `second`, lane 0 writes the placements, the pair and the status of the
//                      jobs; every counter of the two handles is recounted from the final values, through LDS and one atomic per
//                      workgroup and counter
// Why the segments are exact: a fresh start only restricts where an alignment may begin, so no computed score lies below the true
// one; an alignment at distance <= E spans at most m + E text letters, so every score <= E inside the segment's own range is the
// true one.  The least key over the segments therefore is the (dist, end) of one serial pass whenever dist <= E.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "kmx_approx.h"
#include "kmx_align_core.h"
#include "kmx_fold_core.h"
#include "kmx_kernels.h"
#include "kmx_strands.h"
#include "kmx_vote.h"

namespace {

constexpr uint32_t kNoBest = 0xFFFFFFFFu;
constexpr uint32_t kNoScore = 0xFFFFu;
constexpr uint64_t kNoKey = ~uint64_t(0);
constexpr uint64_t kDefaultSegment = 512;
// the counters of the plan, then what the fold recounts: the rescue's own, then the placements' and the pairs' (kmx::PL_*, kmx::PR_*)
enum { CTR_N_JOBS = 0, CTR_PEQ_WORDS, CTR_CLASS, CTR_N_FOUND = CTR_CLASS + kClasses, CTR_N_JOB_CONCORDANT, CTR_N_TAKEN, CTR_FOLD,
       CTR_COUNT = CTR_FOLD + kmx::PR_COUNT };

using kmx::Buf;
using Pinned = kmx::PinnedArr;
using kmx::grid_for;

// the placements and the pairs as the fold reads and rewrites them, and the options
struct RescueIn {
    uint32_t* pl_locus;            // [2 np]
    uint8_t* pl_strand;
    uint8_t* pl_dist;
    uint32_t* pl_start;
    uint32_t* pl_end;
    uint8_t* pl_second;
    uint32_t* pl_best2;            // [4 np]
    uint8_t* cls;                  // [np]
    int32_t* tlen;
    uint16_t* score;
    uint16_t* second_score;
    uint64_t np, n;
    uint64_t penalty;
    Insert ins;
    uint32_t max_edits, flags;
    const uint64_t* ctg_off;       // [nc + 1]: the index's contig table; nullptr without one
    const uint32_t* ctg;           // [n_loci]: the contig of every locus (the alignments'); nullptr without a table
    uint64_t nc, n_loci;
};

// the job arrays; job_off[nr2 + 1] delimits them per internal read
struct Jobs {
    const uint64_t* job_off;
    uint32_t* read;                // [cap]
    uint32_t* lo;
    uint32_t* hi;
    uint8_t* dist;
    uint32_t* start;
    uint32_t* end;
    uint8_t* status;
    uint8_t* cls;                  // the class of the passes, CLS_OUT when the job is not served
    unsigned long long* key;       // dist << 32 | end of the forward pass
    uint64_t cap, n_jobs;          // room (2 np); the jobs there are (known after the plan)
};

// Internal read r is the looked-for strand of a mate with a job: its window [lo, hi) (kmx.h), clamped to the contig of the anchor's
// locus when the index has a table.
__device__ __forceinline__ bool job_window(const RescueIn& R, uint64_t r, uint32_t* lo, uint32_t* hi)
{
    const uint64_t p = r >> 2;
    const uint32_t b = uint32_t(r >> 1) & 1u, s = uint32_t(r) & 1u, a = 1u - b;
    const uint32_t c = R.cls[p];
    const bool only = c == (a == 0 ? KMX_PAIR_MATE1_ONLY : KMX_PAIR_MATE2_ONLY);
    if (!only && !(c == KMX_PAIR_DISCORDANT && (R.flags & KMX_RESCUE_DISCORDANT))) return false;
    const uint32_t sa = R.pl_strand[2 * p + a];
    if (sa > 1) return false;                                  // (cannot happen: the anchor is placed)
    if (s != (R.ins.orientation == KMX_PAIR_FF ? sa : 1u - sa)) return false;
    const bool up = R.ins.orientation == KMX_PAIR_FR ? sa == 0 : R.ins.orientation == KMX_PAIR_RF ? sa == 1 : (a == 0) == (sa == 0);
    const int64_t n = int64_t(R.n);
    int64_t b0 = 0, b1 = n;                                    // the bounds: the text, or the anchor's contig
    if (R.ctg) {                                               // (uniform across the grid)
        const uint32_t al = R.pl_locus[2 * p + a];             // (an anchor is always placed by a locus)
        const uint32_t cg = al < R.n_loci ? R.ctg[al] : 0xFFFFFFFFu;
        if (cg < R.nc) {
            b1 = min(int64_t(R.ctg_off[cg + 1]), n);
            b0 = min(int64_t(R.ctg_off[cg]), b1);
        }
    }
    int64_t l, h;
    if (up) {
        l = min(max(int64_t(R.pl_start[2 * p + a]), b0), b1);
        h = min(b1, l + R.ins.max_insert);
    } else {
        h = max(min(int64_t(R.pl_end[2 * p + a]), b1), b0);
        l = max(b0, h - R.ins.max_insert);
    }
    *lo = uint32_t(l);
    *hi = uint32_t(h);
    return true;
}

// ---- the plan ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_rescue_plan(RescueIn R, uint32_t* __restrict__ flag)
{
    const uint64_t r = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (r >= 4 * R.np) return;
    uint32_t lo, hi;
    flag[r] = job_window(R, r, &lo, &hi) ? 1u : 0u;
}

// A.locus_off is job_off: the jobs are shaped like the loci of the doubled batch
__global__ __launch_bounds__(kBlock) void k_rescue_jobs(RescueIn R, AlignIn A, Jobs J, uint32_t* __restrict__ best, unsigned long long* __restrict__ ctr)
{
    __shared__ uint32_t s_cnt[kClasses];
    if (threadIdx.x < kClasses) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t r = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (r < A.nr) {
        best[r] = kNoBest;                                     // (the fold marks the reads of the taken jobs)
        uint32_t lo, hi;
        const uint64_t j = J.job_off[r];
        if (job_window(R, r, &lo, &hi) && j < J.cap) {
            uint64_t r0;
            bool too_long;
            const uint32_t m = read_letters(A, r, &r0, &too_long);
            const bool served = m > A.max_edits;               // (m == 0: an empty read, or one longer than KMX_ALIGN_MAX_READ)
            const uint8_t c = served ? uint8_t(class_of((m + 63) / 64)) : CLS_OUT;
            if (served) atomicAdd(&s_cnt[c], 1u);
            J.read[j] = uint32_t(r);
            J.lo[j] = lo;
            J.hi[j] = hi;
            J.dist[j] = served ? KMX_ALIGN_NONE : KMX_ALIGN_SKIPPED;   // (the reverse pass overwrites the jobs that are found)
            J.start[j] = 0;
            J.end[j] = 0;
            J.status[j] = 0;
            J.cls[j] = c;
            J.key[j] = kNoKey;
        }
    }
    __syncthreads();
    if (threadIdx.x < kClasses && s_cnt[threadIdx.x]) atomicAdd(&ctr[CTR_CLASS + threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
}

// ---- the passes ----------------------------------------------------------------------------------------------------------------------
struct RescuePass {
    const uint64_t* peq_off;
    const uint64_t* peq;           // the table of this pass (forward, or the reversed reads')
};

template <int NW>
__global__ __launch_bounds__(kAlignBlock) void k_rescue_fwd(AlignIn A, Jobs J, RescuePass P, uint64_t G, uint64_t segs)
{
    const uint64_t t = uint64_t(blockIdx.x) * kAlignBlock + threadIdx.x;
    const uint64_t j = t / segs, g = t % segs;
    if (j >= J.n_jobs || J.cls[j] != class_of(uint32_t(NW))) return;
    const uint64_t lo = J.lo[j], hi = min(uint64_t(J.hi[j]), A.n);
    const uint64_t c0 = lo + g * G;                             // the first column of the segment's own (g < 2^17, G < 2^32)
    if (c0 >= hi) return;
    const uint64_t c1 = min(hi, c0 + G);
    const uint64_t r = J.read[j];
    uint64_t r0;
    bool too_long;
    const uint32_t m = read_letters(A, r, &r0, &too_long);
    const uint32_t nw = (m + 63) / 64;
    if (m == 0 || nw > uint32_t(NW)) return;                    // (cannot happen: k_rescue_jobs read the same offsets)
    const uint64_t warm = uint64_t(m) + A.max_edits;
    const uint64_t ws = c0 - lo > warm ? c0 - warm : lo;        // the fresh start
    const uint64_t* pq = P.peq + P.peq_off[r];
    const uint32_t lastw = (m - 1) >> 6, lastbit = (m - 1) & 63;
    const uint32_t w = A.w, per = 64 / w, sigma = A.sigma;
    const uint64_t mask = (uint64_t(1) << w) - 1;               // (w <= 8)
    uint64_t Pv[NW], Mv[NW];
#pragma unroll
    for (int b = 0; b < NW; ++b) { Pv[b] = ~uint64_t(0); Mv[b] = 0; }
    uint32_t score = m, best = m;                               // (m > E: a score of m is never reported)
    uint64_t best_at = c0;
    uint64_t word = A.text[ws / per];
    for (uint64_t p = ws; p < c1; ++p) {
        const uint32_t k = uint32_t(p % per);
        if (k == 0) word = A.text[p / per];
        const uint32_t c = uint32_t((word >> (k * w)) & mask);
        const uint64_t* row = pq + uint64_t(c) * nw;
        const bool known = c < sigma;
        score += column<NW>(Pv, Mv, [&](int b) { return known && uint32_t(b) < nw ? row[b] : uint64_t(0); }, 0, 0, lastw, lastbit);
        if (p >= c0 && score < best) { best = score; best_at = p + 1; }
    }
    if (best <= A.max_edits) atomicMin(&J.key[j], (unsigned long long)((uint64_t(best) << 32) | best_at));
}

template <int NW>
__global__ __launch_bounds__(kAlignBlock) void k_rescue_rev(AlignIn A, Jobs J, RescuePass P)
{
    const uint64_t j = uint64_t(blockIdx.x) * kAlignBlock + threadIdx.x;
    if (j >= J.n_jobs || J.cls[j] != class_of(uint32_t(NW))) return;
    const uint64_t key = J.key[j];
    if (key == kNoKey) return;                                  // dist[j] is KMX_ALIGN_NONE already
    const uint64_t r = J.read[j];
    uint64_t r0;
    bool too_long;
    const uint32_t m = read_letters(A, r, &r0, &too_long);
    const uint32_t nw = (m + 63) / 64;
    if (m == 0 || nw > uint32_t(NW)) return;
    const uint64_t hi = min(uint64_t(J.hi[j]), A.n), lo = min(uint64_t(J.lo[j]), hi);
    const uint64_t e = min(max(key & 0xFFFFFFFFull, lo), hi);   // (end lies in (lo, hi]: the forward pass wrote it)
    const uint32_t d = uint32_t(key >> 32);
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
    J.dist[j] = uint8_t(d);
    J.start[j] = uint32_t(p);
    J.end[j] = uint32_t(e);
}

// ---- the fold ------------------------------------------------------------------------------------------------------------------------
// the loci and alignments of the doubled batch, for `second`
struct LociIn {
    const uint64_t* locus_off;     // [4 np + 1]
    const uint8_t* dist;           // [n_loci]
    const uint32_t* start;
    const uint32_t* end;
    uint64_t n_loci;
};

__global__ __launch_bounds__(kBlock) void k_rescue_fold(RescueIn R, LociIn L, Jobs J, uint32_t* __restrict__ best, unsigned long long* __restrict__ ctr)
{
    __shared__ unsigned int s_ctr[CTR_COUNT];
    if (threadIdx.x < CTR_COUNT) s_ctr[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x % kWave;
    const uint64_t p = uint64_t(blockIdx.x) * (kBlock / kWave) + threadIdx.x / kWave;
    if (p < R.np) {
        // the pair and its two reads as the pair fold (or an earlier rescue) left them
        uint32_t cls = R.cls[p], score = R.score[p], second_score = R.second_score[p];
        uint32_t st[2], sd[2], ss[2], se[2], sec[2];
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            st[m] = R.pl_strand[2 * p + m];
            sd[m] = R.pl_dist[2 * p + m];
            ss[m] = R.pl_start[2 * p + m];
            se[m] = R.pl_end[2 * p + m];
            sec[m] = R.pl_second[2 * p + m];
        }
        // the jobs of the pair: at most one per looked-for mate b, the other mate its anchor
        bool has[2];
        uint64_t jb[2];
        uint32_t status[2] = {0, 0}, jd[2] = {0, 0}, js[2] = {0, 0}, je[2] = {0, 0}, jstrand[2] = {0, 0}, jscore[2] = {0, 0};
        int64_t jt[2] = {0, 0};
        int take = -1;
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const uint64_t j0 = min(J.job_off[4 * p + 2 * b], J.n_jobs), j1 = min(J.job_off[4 * p + 2 * b + 2], J.n_jobs);
            has[b] = j1 > j0;
            jb[b] = j0;
            if (!has[b]) continue;
            const uint32_t d = J.dist[j0];
            if (d > R.max_edits) continue;                     // skipped or none
            status[b] = 1;
            jd[b] = d;
            js[b] = J.start[j0];
            je[b] = J.end[j0];
            jstrand[b] = J.read[j0] & 1u;
            const int a = 1 - b;
            bool first;
            const int64_t t = b == 0 ? concordant_tlen(R.ins, jstrand[b], js[b], je[b], st[a], ss[a], se[a], &first)
                                     : concordant_tlen(R.ins, st[a], ss[a], se[a], jstrand[b], js[b], je[b], &first);
            if (t < 0) continue;
            status[b] = 2;
            jt[b] = first ? t : -t;
            jscore[b] = sd[a] + d;
            if (take < 0 || jscore[b] < jscore[take]) take = b;  // the least (score, b)
        }
        if (take >= 0 && cls == KMX_PAIR_DISCORDANT && uint64_t(jscore[take]) > uint64_t(sd[0]) + sd[1] + R.penalty) take = -1;
        if (take >= 0) {                                       // (the same in every lane)
            // the least distance of an aligned locus of the rescued read elsewhere from the new placement
            uint64_t a, b, c;
            strand_ranges(L.locus_off, L.n_loci, 4 * p + 2 * take, &a, &b, &c);
            const uint32_t sw = jstrand[take], ws = js[take], we = je[take];
            const uint32_t second = second_elsewhere(L.dist, L.start, L.end, a, b, c, lane, kNoLocus, sw, ws, we);   // (the placement is no locus)
            status[take] = 3;
            st[take] = sw;
            sd[take] = jd[take];
            sec[take] = second;
            cls = KMX_PAIR_CONCORDANT;
            score = jscore[take];
            second_score = kNoScore;                           // no runner-up pair is searched for
            if (lane == 0) {
                const uint64_t i = 2 * p + take;
                R.pl_locus[i] = kNoBest;                       // the placement is no locus
                R.pl_strand[i] = uint8_t(sw);
                R.pl_dist[i] = uint8_t(jd[take]);
                R.pl_start[i] = ws;
                R.pl_end[i] = we;
                R.pl_second[i] = uint8_t(second);
                R.pl_best2[2 * i] = kNoBest;
                R.pl_best2[2 * i + 1] = kNoBest;
                R.cls[p] = uint8_t(cls);
                R.tlen[p] = int32_t(jt[take]);
                R.score[p] = uint16_t(score);
                R.second_score[p] = uint16_t(second_score);
                best[J.read[jb[take]]] = 0;                    // (an internal read of this pair: below nr2)
            }
        }
        if (lane == 0) {
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                if (!has[b]) continue;
                J.status[jb[b]] = uint8_t(status[b]);
                if (status[b] >= 1) atomicAdd(&s_ctr[CTR_N_FOUND], 1u);
                if (status[b] >= 2) atomicAdd(&s_ctr[CTR_N_JOB_CONCORDANT], 1u);
                if (status[b] == 3) atomicAdd(&s_ctr[CTR_N_TAKEN], 1u);
            }
            // the counters of the two handles, from the final values
#pragma unroll
            for (int m = 0; m < 2; ++m) count_placement(s_ctr + CTR_FOLD, st[m] != 255u, st[m], sec[m], sd[m]);
            count_pair(s_ctr + CTR_FOLD, cls, score, second_score);
        }
    }
    __syncthreads();
    if (threadIdx.x >= CTR_N_FOUND && threadIdx.x < CTR_COUNT && s_ctr[threadIdx.x]) atomicAdd(&ctr[threadIdx.x], (unsigned long long)s_ctr[threadIdx.x]);
}

} // namespace

struct kmx_rescues {
    int device = 0;
    hipStream_t stream = nullptr;          // the stream of the call that filled the handle (the host view copies on it)
    uint64_t nr2 = 0, n_jobs = 0, n_found = 0, n_concordant = 0, n_taken = 0;
    // results: the offsets per internal read, then one entry per job
    kmx::ArrOf<uint64_t> job_off{kmx::ARR_OFFSETS};
    kmx::ArrOf<uint32_t> read, lo, hi, start, end;
    kmx::ArrOf<uint8_t> dist, status;
    // scratch; best[nr2] selects the taken jobs for kmx_rescues_scripts
    Buf flag, bsum, pcnt, peq_off, peq, cls, key, best, ctr;
    Pinned h_ctr;
    bool host_valid = false;
    std::vector<kmx::Arr*> results() { return {&job_off, &read, &lo, &hi, &dist, &start, &end, &status}; }
    std::vector<Buf*> scratch() { return {&flag, &bsum, &pcnt, &peq_off, &peq, &cls, &key, &best, &ctr}; }
    void release() { kmx::release_arrays(*this); }
    void clear() { nr2 = n_jobs = n_found = n_concordant = n_taken = 0; kmx::clear_arrays(*this); }
    // a call has succeeded: the arrays expose what the counters say
    void expose()
    {
        kmx::expose(results(), n_jobs);
        job_off.n = nr2 + 1;
    }
};

kmx::JobsAccess kmx::rescues_access(const kmx_rescues* r)
{
    return JobsAccess{r->device, r->stream, r->n_jobs, r->start.as<uint32_t>(), r->end.as<uint32_t>()};
}

namespace {

template <int NW>
void launch_passes(hipStream_t s, const AlignIn& A, const Jobs& J, const RescuePass& F, const RescuePass& R, uint64_t G, uint64_t segs)
{
    hipLaunchKernelGGL(k_rescue_fwd<NW>, dim3(grid_for(J.n_jobs * segs, kAlignBlock)), dim3(kAlignBlock), 0, s, A, J, F, G, segs);
    hipLaunchKernelGGL(k_rescue_rev<NW>, dim3(grid_for(J.n_jobs, kAlignBlock)), dim3(kAlignBlock), 0, s, A, J, R);
}

// *folded: k_rescue_fold has been launched, the placements and the pairs are no longer those of before
kmx_status rescue_run(const kmx::IndexAccess& X, const kmx_strand_reads* reads, const kmx::LociAccess& L, const kmx::AlignAccess& A,
                      const kmx_rescue_options& o, hipStream_t s, kmx_placements* pl, kmx_pairs* pr, kmx_rescues* h, bool* folded)
{
    const uint64_t nr2 = L.nr, np = nr2 / 4, cap = 2 * np;
    TRY_HIP(h->job_off.ensure((nr2 + 1) * 8));
    if (np == 0) {                                             // no pair: no launch indexes an empty array
        TRY_HIP(hipMemsetAsync(h->job_off.p, 0, 8, s));
        h->expose();
        return KMX_OK;
    }
    TRY_KMX(kmx::ensure_text(X, s));
    for (Buf* b : {&h->flag, &h->pcnt}) TRY_HIP(b->ensure(nr2 * 4 + 16));
    TRY_HIP(h->bsum.ensure(kmx::scan_blocks(nr2) * 8 + 16));
    TRY_HIP(h->peq_off.ensure((nr2 + 1) * 8));
    for (Buf* b : {&h->read, &h->lo, &h->hi, &h->start, &h->end}) TRY_HIP(b->ensure(cap * 4));
    for (Buf* b : std::initializer_list<Buf*>{&h->dist, &h->status, &h->cls}) TRY_HIP(b->ensure(cap));
    TRY_HIP(h->key.ensure(cap * 8));
    TRY_HIP(h->best.ensure(nr2 * 4));
    TRY_HIP(h->ctr.ensure(CTR_COUNT * 8));
    unsigned long long* ctr = h->ctr.as<unsigned long long>();
    TRY_HIP(hipMemsetAsync(ctr, 0, CTR_COUNT * 8, s));
    const RescueIn R{pl->locus.as<uint32_t>(), pl->strand.as<uint8_t>(), pl->dist.as<uint8_t>(), pl->start.as<uint32_t>(), pl->end.as<uint32_t>(),
                     pl->second.as<uint8_t>(), pl->best2.as<uint32_t>(), pr->cls.as<uint8_t>(), pr->tlen.as<int32_t>(), pr->score.as<uint16_t>(),
                     pr->second_score.as<uint16_t>(), np, X.n, o.unpaired_penalty, Insert{int64_t(o.min_insert), int64_t(o.max_insert), o.orientation},
                     o.max_edits, o.flags, A.ctg ? X.ctg_off : nullptr, A.ctg, A.nc, A.n_loci};
    Jobs J{h->job_off.as<uint64_t>(), h->read.as<uint32_t>(), h->lo.as<uint32_t>(), h->hi.as<uint32_t>(), h->dist.as<uint8_t>(), h->start.as<uint32_t>(),
           h->end.as<uint32_t>(), h->status.as<uint8_t>(), h->cls.as<uint8_t>(), h->key.as<unsigned long long>(), cap, 0};
    // the job reads take the place of the reads with loci: job_off that of locus_off (diag and span are not looked at)
    const AlignIn Q{reads->ranks2.as<uint8_t>(), reads->roff2.as<uint64_t>(), reads->letters2, J.job_off, nullptr, nullptr, nr2, 0, X.n,
                    X.text->d_words, X.text->w, X.sigma, o.max_edits, 0};
    const dim3 per_read(grid_for(nr2, kBlock)), block(kBlock);
    hipLaunchKernelGGL(k_rescue_plan, per_read, block, 0, s, R, h->flag.as<uint32_t>());
    kmx::launch_scan(s, h->flag.as<uint32_t>(), nr2, h->bsum.as<uint64_t>(), h->job_off.as<uint64_t>(), ctr + CTR_N_JOBS);
    hipLaunchKernelGGL(k_rescue_jobs, per_read, block, 0, s, R, Q, J, h->best.as<uint32_t>(), ctr);
    hipLaunchKernelGGL(k_align_count, per_read, block, 0, s, Q, h->pcnt.as<uint32_t>());
    kmx::launch_scan(s, h->pcnt.as<uint32_t>(), nr2, h->bsum.as<uint64_t>(), h->peq_off.as<uint64_t>(), ctr + CTR_PEQ_WORDS);
    TRY_HIP(hipGetLastError());
    TRY_KMX(kmx::read_back("kmx_pairs_rescue", s, ctr, h->h_ctr, CTR_COUNT * 8));
    uint64_t c[CTR_COUNT];
    std::memcpy(c, h->h_ctr.p, sizeof c);
    const uint64_t n_jobs = c[CTR_N_JOBS];
    if (n_jobs > cap) return kmx::set_error(KMX_ERR_HIP, "kmx_pairs_rescue: more jobs than mates");                   // (never: a guard for the arrays)
    J.n_jobs = n_jobs;
    if (n_jobs) {
        const uint64_t G = o.segment ? o.segment : kDefaultSegment;
        const uint64_t segs = (uint64_t(o.max_insert) + G - 1) / G;     // a window has max_insert columns at the most
        uint64_t served = 0;
        for (int k = 0; k < kClasses; ++k) served += c[CTR_CLASS + k];
        if (served && segs) {
            if (n_jobs * segs / kAlignBlock >= (uint64_t(1) << 31)) return kmx::set_error(KMX_ERR_TOO_LARGE, "kmx_pairs_rescue: too many segments: split the reads");
            const uint64_t n_words = c[CTR_PEQ_WORDS];
            TRY_HIP(h->peq.ensure(std::max<uint64_t>(n_words, 1) * 16));
            if (n_words)
                hipLaunchKernelGGL(k_align_peq, dim3(grid_for(n_words, kBlock)), block, 0, s, Q, h->peq_off.as<uint64_t>(), n_words, h->peq.as<uint64_t>());
            const RescuePass F{h->peq_off.as<uint64_t>(), h->peq.as<uint64_t>()};
            const RescuePass B{h->peq_off.as<uint64_t>(), h->peq.as<uint64_t>() + n_words};
            for (int k = 0; k < kClasses; ++k) {
                if (!c[CTR_CLASS + k]) continue;
                switch (k) {
                case 0: launch_passes<1>(s, Q, J, F, B, G, segs); break;
                case 1: launch_passes<2>(s, Q, J, F, B, G, segs); break;
                case 2: launch_passes<4>(s, Q, J, F, B, G, segs); break;
                case 3: launch_passes<8>(s, Q, J, F, B, G, segs); break;
                default: launch_passes<16>(s, Q, J, F, B, G, segs); break;
                }
            }
            TRY_HIP(hipGetLastError());
        }
        const LociIn Li{L.locus_off, A.dist, A.start, A.end, L.n_loci};
        *folded = true;
        pl->host_valid = pl->host_best2_valid = pr->host_valid = false;
        hipLaunchKernelGGL(k_rescue_fold, dim3(grid_for(np, kBlock / kWave)), block, 0, s, R, Li, J, h->best.as<uint32_t>(), ctr);
        TRY_HIP(hipGetLastError());
        TRY_KMX(kmx::read_back("kmx_pairs_rescue", s, ctr, h->h_ctr, CTR_COUNT * 8));
        const uint64_t* f = h->h_ctr.as<uint64_t>();
        pl->counts_from(f + CTR_FOLD);
        pr->counts_from(f + CTR_FOLD);
        h->n_found = f[CTR_N_FOUND];
        h->n_concordant = f[CTR_N_JOB_CONCORDANT];
        h->n_taken = f[CTR_N_TAKEN];
    }
    h->nr2 = nr2;
    h->n_jobs = n_jobs;
    h->expose();
    return KMX_OK;
}

} // namespace

extern "C" {

kmx_status kmx_pairs_rescue(const kmx_index* index, const kmx_strand_reads* reads, const kmx_loci* loci, const kmx_alignments* alignments,
                            const kmx_rescue_options* o, kmx_placements* placements, kmx_pairs* pairs, kmx_rescues** inout)
{
    const std::string who = "kmx_pairs_rescue: ";
    if (!index) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "index is NULL");
    if (!reads) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "strand reads handle is NULL");
    if (!loci) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "loci handle is NULL");
    if (!alignments) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "alignments handle is NULL");
    if (!o) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "options is NULL");
    if (!placements) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "placements handle is NULL");
    if (!pairs) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "pairs handle is NULL");
    if (!inout) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "inout is NULL");
    if (o->struct_size < sizeof(kmx_rescue_options)) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "options->struct_size is too small");
    if (o->flags & ~KMX_RESCUE_DISCORDANT) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "unknown flags");
    if (o->orientation > KMX_PAIR_FF) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "orientation is none of KMX_PAIR_FR, KMX_PAIR_RF, KMX_PAIR_FF");
    if (o->min_insert > o->max_insert) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "min_insert is greater than max_insert");
    if (o->max_insert > KMX_RESCUE_MAX_INSERT) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "max_insert > KMX_RESCUE_MAX_INSERT");
    if (o->max_edits > KMX_ALIGN_MAX_EDITS) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "max_edits > KMX_ALIGN_MAX_EDITS");
    const kmx::LociAccess L = kmx::loci_access(loci);
    const kmx::AlignAccess A = kmx::alignments_access(alignments);
    kmx_rescues* h = *inout;
    auto refuse = kmx::refuser(who, h);                        // (the placements and the pairs stay as they are)
    const uint64_t nr2 = L.nr;
    if (A.nr != nr2) return refuse(KMX_ERR_INVALID_ARGUMENT, "the alignments handle's nr differs from the loci handle's");
    if (reads->nr2 != nr2) return refuse(KMX_ERR_INVALID_ARGUMENT, "the reads are not those of the loci: nr2 differs");
    if (2 * placements->nr != nr2) return refuse(KMX_ERR_INVALID_ARGUMENT, "the placements are not those of these reads: nr differs");
    if (4 * pairs->np != nr2) return refuse(KMX_ERR_INVALID_ARGUMENT, "the pairs are not those of these reads: np differs");
    if (A.n_loci != L.n_loci) return refuse(KMX_ERR_INVALID_ARGUMENT, "the alignments handle's n_loci differs from the loci handle's");
    if (nr2 && (A.device != L.device || reads->device != L.device || placements->device != L.device || pairs->device != L.device))
        return refuse(KMX_ERR_INVALID_ARGUMENT, "the handles live on different devices");
    if (nr2 & 3) return refuse(KMX_ERR_INVALID_ARGUMENT, "the number of reads is no multiple of 4: not the loci of a doubled batch of pairs");
    kmx::IndexAccess X{};
    kmx_status no_st;
    std::string no_index;
    if (!kmx::index_for(index, L.device, "the loci", &X, &no_st, &no_index)) return refuse(no_st, no_index);
    if (A.nc != (X.ctg_off ? X.nc : 0) || A.ctg_gen != X.ctg_gen)
        return refuse(KMX_ERR_INVALID_ARGUMENT, "the alignments were made under another contig table of the index (kmx_index_set_contigs was called since): align again");
    kmx::DeviceGuard dg;
    TRY_KMX(kmx::bind_handle(inout, L.device));
    h = *inout;
    hipStream_t s = reads->stream;
    bool folded = false;
    const kmx_status st = kmx::run_into(h, s, [&] { return rescue_run(X, reads, L, A, *o, s, placements, pairs, h, &folded); });
    if (st != KMX_OK && folded) {                              // no handle holds half a result
        placements->clear();
        pairs->clear();
    }
    return st;
}

kmx_status kmx_rescues_counts(const kmx_rescues* h, uint64_t* nr2, uint64_t* n_jobs, uint64_t* n_found, uint64_t* n_concordant, uint64_t* n_taken)
{
    if (!h) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_rescues_counts: rescues handle is NULL");
    if (nr2) *nr2 = h->nr2;
    if (n_jobs) *n_jobs = h->n_jobs;
    if (n_found) *n_found = h->n_found;
    if (n_concordant) *n_concordant = h->n_concordant;
    if (n_taken) *n_taken = h->n_taken;
    return KMX_OK;
}

kmx_status kmx_rescues_view_device(const kmx_rescues* h, const uint64_t** d_job_off, const uint32_t** d_read, const uint32_t** d_lo, const uint32_t** d_hi,
                                   const uint8_t** d_dist, const uint32_t** d_start, const uint32_t** d_end, const uint8_t** d_status)
{
    if (!h) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_rescues_view_device: rescues handle is NULL");
    if (d_job_off) *d_job_off = h->job_off.dev();
    if (d_read) *d_read = h->read.dev();
    if (d_lo) *d_lo = h->lo.dev();
    if (d_hi) *d_hi = h->hi.dev();
    if (d_dist) *d_dist = h->dist.dev();
    if (d_start) *d_start = h->start.dev();
    if (d_end) *d_end = h->end.dev();
    if (d_status) *d_status = h->status.dev();
    return KMX_OK;
}

kmx_status kmx_rescues_view(kmx_rescues* h, const uint64_t** job_off, const uint32_t** read, const uint32_t** lo, const uint32_t** hi,
                            const uint8_t** dist, const uint32_t** start, const uint32_t** end, const uint8_t** status)
{
    if (!h) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_rescues_view: rescues handle is NULL");
    TRY_KMX(kmx::host_view("kmx_rescues_view", *h));           // 8 bytes per internal read, 22 per job
    if (job_off) *job_off = h->job_off.host();
    if (read) *read = h->read.host();
    if (lo) *lo = h->lo.host();
    if (hi) *hi = h->hi.host();
    if (dist) *dist = h->dist.host();
    if (start) *start = h->start.host();
    if (end) *end = h->end.host();
    if (status) *status = h->status.host();
    return KMX_OK;
}

kmx_status kmx_rescues_scripts(const kmx_index* index, const kmx_strand_reads* reads, const kmx_rescues* rescues, const kmx_script_options* options,
                               kmx_scripts** inout)
{
    const std::string who = "kmx_rescues_scripts: ";
    if (!reads) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "strand reads handle is NULL");
    if (!rescues) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "rescues handle is NULL");
    if (rescues->nr2 != reads->nr2) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "the rescues are not those of these reads: nr2 differs");
    if (rescues->nr2 && rescues->device != reads->device) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "the rescues and the reads live on different devices");
    // the jobs stand in for the loci and their alignments, best[] selects the taken ones
    const kmx::LociAccess L{reads->device, reads->stream, rescues->nr2, rescues->n_jobs, rescues->job_off.as<uint64_t>(), nullptr, nullptr, nullptr};
    const kmx::AlignAccess A{reads->device, reads->stream, rescues->nr2, rescues->n_jobs, rescues->dist.as<uint8_t>(), rescues->start.as<uint32_t>(),
                             rescues->end.as<uint32_t>(), rescues->best.as<uint32_t>()};
    return kmx::scripts_on_arrays("kmx_rescues_scripts", index, L, A, reads->ranks2.p, reads->roff2.p, reads->letters2, rescues->best.as<uint32_t>(), options,
                                  reads->stream, inout);
}

void kmx_rescues_free(kmx_rescues* h) { kmx::free_handle(h); }

} // extern "C"
