// Paired-end reads of the read-mapping chain (kmx_alignments_fold_pairs; include/kmx.h, KMX_MAP_PAIRS).  The doubled batch of
// kmx_reads_strands holds interleaved mates: internal reads 4p .. 4p + 3 are mate 1 forward, mate 1 reverse complement, mate 2
// forward, mate 2 reverse complement.  The two mates of every pair are folded into one concordant pair of loci where there is one,
// and into the single-read placements of kmx_alignments_fold_strands where there is none; the placements handle is that fold's.
//
//   k_pair_fold        a wave per pair: the single winners from best[4p .. 4p + 3]; then the aligned loci of the mate with fewer loci
//                      one after the other (wave-uniform) against the loci of the other mate, the lanes striding over them, once for
//                      the least (score, x, y) and, where a pair was taken, once more for the runner-up; the per-read `second` as
//                      in k_strand_fold, against the chosen loci; lane 0 writes; the batch totals go through LDS and one atomic per
//                      workgroup
#include <hip/hip_runtime.h>

#include <string>

#include "kmx_fold_core.h"
#include "kmx_strands.h"
#include "kmx_vote.h"

namespace {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kWave = 64;
constexpr uint32_t kNoBest = 0xFFFFFFFFu;
constexpr uint32_t kNoScore = 0xFFFFu;
constexpr int CTR_COUNT = kmx::PR_COUNT;                       // the placements' counters, then the pairs'

using kmx::Buf;
using Pinned = kmx::PinnedArr;
using kmx::grid_for;

struct PairIn {
    const uint64_t* locus_off;     // [4 np + 1]
    const uint8_t* dist;           // [n_loci]
    const uint32_t* start;
    const uint32_t* end;
    const uint32_t* best;          // [4 np]
    const uint32_t* ctg;           // [n_loci]: the contig of every locus; nullptr when the alignments were made without a contig table
    uint64_t np, n_loci;
    uint64_t penalty;
    Insert ins;
};

struct PairOut {
    uint32_t* locus;               // [2 np]: the placements
    uint8_t* strand;
    uint8_t* dist;
    uint32_t* start;
    uint32_t* end;
    uint8_t* second;
    uint32_t* best2;               // [4 np]
    uint8_t* cls;                  // [np]: the pairs
    int32_t* tlen;
    uint16_t* score;
    uint16_t* second_score;
    unsigned long long* ctr;       // [CTR_COUNT]
};

// A locus as the walk hands it on: its index, strand, interval and distance
struct Locus { uint32_t l, s, start, end, d; };

// Every concordant (x, y) of the pair whose offsets are o[0 .. 4] goes to visit(x, y) in some lane: the aligned loci of the mate with
// fewer loci one after the other, the lanes over the loci of the other mate.  With a contig table two loci of different contigs are
// never concordant (the test on the pointer is uniform across the grid).
template <typename Visit>
__device__ __forceinline__ void walk_concordant(const PairIn& P, const uint64_t* o, uint32_t lane, Visit visit)
{
    const bool outer1 = o[2] - o[0] <= o[4] - o[2];            // mate 1 in the outer loop
    const uint64_t oa = outer1 ? o[0] : o[2], ob = outer1 ? o[1] : o[3], oc = outer1 ? o[2] : o[4];
    const uint64_t ia = outer1 ? o[2] : o[0], ib = outer1 ? o[3] : o[1], ic = outer1 ? o[4] : o[2];
    for (uint64_t lo = oa; lo < oc; ++lo) {
        const uint32_t dlo = P.dist[lo];
        if (dlo >= KMX_ALIGN_SKIPPED) continue;
        const Locus out{uint32_t(lo), lo < ob ? 0u : 1u, P.start[lo], P.end[lo], dlo};
        const uint32_t co = P.ctg ? P.ctg[lo] : 0u;
        for (uint64_t li = ia + lane; li < ic; li += kWave) {
            const uint32_t dli = P.dist[li];
            if (dli >= KMX_ALIGN_SKIPPED) continue;
            const Locus in{uint32_t(li), li < ib ? 0u : 1u, P.start[li], P.end[li], dli};
            if (P.ctg && P.ctg[li] != co) continue;
            const Locus& x = outer1 ? out : in;
            const Locus& y = outer1 ? in : out;
            bool first;
            if (concordant_tlen(P.ins, x.s, x.start, x.end, y.s, y.start, y.end, &first) >= 0) visit(x, y);
        }
    }
}

__global__ __launch_bounds__(kBlock) void k_pair_fold(PairIn P, PairOut O)
{
    __shared__ unsigned int s_ctr[CTR_COUNT];
    if (threadIdx.x < CTR_COUNT) s_ctr[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x % kWave;
    const uint64_t p = uint64_t(blockIdx.x) * (kBlock / kWave) + threadIdx.x / kWave;
    if (p < P.np) {
        // the loci of the four internal reads: o[0] <= ... <= o[4], inside the arrays whatever the offsets hold
        uint64_t o[5];
        strand_ranges(P.locus_off, P.n_loci, 4 * p, &o[0], &o[1], &o[2]);
        strand_ranges(P.locus_off, P.n_loci, 4 * p + 2, &o[2], &o[3], &o[4], o[1]);
        // step 1: the single winner of each mate
        bool placed[2];
        uint64_t w[2];                                         // the chosen locus of each mate
        uint32_t wd[2];
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const Winner W = strand_winner(P.dist, P.best, 4 * p + 2 * m, o[2 * m], o[2 * m + 1], o[2 * m + 2]);
            placed[m] = W.placed;
            w[m] = W.locus;
            wd[m] = W.dist;
        }
        // step 2: the concordant (x, y) with the least (score, x, y)
        uint32_t cs = kNoBest, cx = kNoBest, cy = kNoBest;
        if (placed[0] && placed[1])
            walk_concordant(P, o, lane, [&](const Locus& x, const Locus& y) {
                const uint32_t sc = x.d + y.d;
                if (sc < cs || (sc == cs && (x.l < cx || (x.l == cx && y.l < cy)))) { cs = sc; cx = x.l; cy = y.l; }
            });
        for (int off = kWave / 2; off > 0; off >>= 1) {
            const uint32_t s2 = __shfl_xor(cs, off), x2 = __shfl_xor(cx, off), y2 = __shfl_xor(cy, off);
            if (s2 < cs || (s2 == cs && (x2 < cx || (x2 == cx && y2 < cy)))) { cs = s2; cx = x2; cy = y2; }
        }
        const bool taken = cs != kNoBest && uint64_t(cs) <= uint64_t(wd[0]) + wd[1] + P.penalty;
        uint32_t cls = placed[0] ? (placed[1] ? KMX_PAIR_DISCORDANT : KMX_PAIR_MATE1_ONLY) : (placed[1] ? KMX_PAIR_MATE2_ONLY : KMX_PAIR_UNPLACED);
        uint32_t score = cls == KMX_PAIR_UNPLACED ? kNoScore : (placed[0] ? wd[0] : 0u) + (placed[1] ? wd[1] : 0u);
        uint32_t second_score = kNoScore;
        int32_t tlen = 0;
        if (taken) {
            // step 3: the least score of a concordant pair of which one locus at least lies elsewhere from the winner's
            const uint32_t sx = cx < o[1] ? 0u : 1u, xs = P.start[cx], xe = P.end[cx];
            const uint32_t sy = cy < o[3] ? 0u : 1u, ys = P.start[cy], ye = P.end[cy];
            walk_concordant(P, o, lane, [&](const Locus& x, const Locus& y) {
                const bool x_else = x.l != cx && elsewhere(x.s, x.start, x.end, sx, xs, xe);
                const bool y_else = y.l != cy && elsewhere(y.s, y.start, y.end, sy, ys, ye);
                if (x_else || y_else) second_score = min(second_score, x.d + y.d);
            });
            for (int off = kWave / 2; off > 0; off >>= 1) second_score = min(second_score, uint32_t(__shfl_xor(second_score, off)));
            bool first;
            const int64_t t = concordant_tlen(P.ins, sx, xs, xe, sy, ys, ye, &first);
            tlen = first ? int32_t(t) : -int32_t(t);
            cls = KMX_PAIR_CONCORDANT;
            score = cs;
            w[0] = cx; w[1] = cy;
            wd[0] = P.dist[cx]; wd[1] = P.dist[cy];
        }
        // step 4: per read, the least distance of an aligned locus elsewhere from the chosen one; step 5: lane 0 writes
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const uint64_t a = o[2 * m], b = o[2 * m + 1], c = o[2 * m + 2], i = 2 * p + m;
            const uint32_t sw = w[m] < b ? 0u : 1u;
            uint32_t ws = 0, we = 0, second = KMX_ALIGN_NONE;
            if (placed[m]) {
                ws = P.start[w[m]]; we = P.end[w[m]];
                second = second_elsewhere(P.dist, P.start, P.end, a, b, c, lane, w[m], sw, ws, we);
            }
            if (lane == 0) {
                O.locus[i] = placed[m] ? uint32_t(w[m]) : kNoBest;
                O.strand[i] = placed[m] ? uint8_t(sw) : uint8_t(255);
                O.dist[i] = uint8_t(wd[m]);
                O.start[i] = ws;
                O.end[i] = we;
                O.second[i] = uint8_t(second);
                O.best2[2 * i] = placed[m] && sw == 0 ? uint32_t(w[m] - a) : kNoBest;
                O.best2[2 * i + 1] = placed[m] && sw == 1 ? uint32_t(w[m] - b) : kNoBest;
                count_placement(s_ctr, placed[m], sw, second, wd[m]);
            }
        }
        if (lane == 0) {
            O.cls[p] = uint8_t(cls);
            O.tlen[p] = tlen;
            O.score[p] = uint16_t(score);
            O.second_score[p] = uint16_t(second_score);
            count_pair(s_ctr, cls, score, second_score);
        }
    }
    __syncthreads();
    if (threadIdx.x < CTR_COUNT && s_ctr[threadIdx.x]) atomicAdd(&O.ctr[threadIdx.x], (unsigned long long)s_ctr[threadIdx.x]);
}

// ---- the host side ----------------------------------------------------------------------------------------------------------------
kmx_status pair_fold_run(const kmx::LociAccess& L, const kmx::AlignAccess& A, const kmx_pair_options& o, hipStream_t s, kmx_placements* pl, kmx_pairs* pr)
{
    const uint64_t np = L.nr / 4;
    pl->stream = pr->stream = s;
    pl->clear();
    pr->clear();
    (void)hipGetLastError();
    if (np == 0) return KMX_OK;
    TRY_HIP(pl->room(2 * np));
    TRY_HIP(pr->cls.ensure(np));
    TRY_HIP(pr->tlen.ensure(np * 4));
    for (kmx::Arr* a : {&pr->score, &pr->second_score}) TRY_HIP(a->ensure(np * 2));
    TRY_HIP(pr->ctr.ensure(CTR_COUNT * 8));
    unsigned long long* ctr = pr->ctr.as<unsigned long long>();
    TRY_HIP(hipMemsetAsync(ctr, 0, CTR_COUNT * 8, s));
    const PairIn P{L.locus_off, A.dist, A.start, A.end, A.best, A.ctg, np, L.n_loci, o.unpaired_penalty,
                   Insert{int64_t(o.min_insert), int64_t(o.max_insert), o.orientation}};
    const PairOut O{pl->locus.as<uint32_t>(), pl->strand.as<uint8_t>(), pl->dist.as<uint8_t>(), pl->start.as<uint32_t>(), pl->end.as<uint32_t>(),
                    pl->second.as<uint8_t>(), pl->best2.as<uint32_t>(), pr->cls.as<uint8_t>(), pr->tlen.as<int32_t>(), pr->score.as<uint16_t>(),
                    pr->second_score.as<uint16_t>(), ctr};
    hipLaunchKernelGGL(k_pair_fold, dim3(grid_for(np, kBlock / kWave)), dim3(kBlock), 0, s, P, O);
    TRY_HIP(hipGetLastError());
    TRY_KMX(kmx::read_back("kmx_alignments_fold_pairs", s, ctr, pr->h_ctr, CTR_COUNT * 8));
    const uint64_t* h = pr->h_ctr.as<uint64_t>();
    pl->expose(2 * np);
    pl->counts_from(h);
    pr->expose(np);
    pr->counts_from(h);
    return KMX_OK;
}

} // namespace

extern "C" {

kmx_status kmx_alignments_fold_pairs(const kmx_loci* loci, const kmx_alignments* alignments, const kmx_pair_options* o, void* stream,
                                     kmx_placements** inout_placements, kmx_pairs** inout_pairs)
{
    const std::string who = "kmx_alignments_fold_pairs: ";
    if (!loci) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "loci handle is NULL");
    if (!alignments) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "alignments handle is NULL");
    if (!o) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "options is NULL");
    if (!inout_placements) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "inout_placements is NULL");
    if (!inout_pairs) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "inout_pairs is NULL");
    if (o->struct_size < sizeof(kmx_pair_options)) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "options->struct_size is too small");
    if (o->flags != 0) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "flags must be 0");
    if (o->orientation > KMX_PAIR_FF) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "orientation is none of KMX_PAIR_FR, KMX_PAIR_RF, KMX_PAIR_FF");
    if (o->min_insert > o->max_insert) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "min_insert is greater than max_insert");
    if (o->max_insert >= (1u << 31)) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "max_insert must be less than 2^31");
    const kmx::LociAccess L = kmx::loci_access(loci);
    const kmx::AlignAccess A = kmx::alignments_access(alignments);
    kmx_placements* pl = *inout_placements;
    kmx_pairs* pr = *inout_pairs;
    auto refuse = [&](kmx_status st, const std::string& msg) {
        if (pl) pl->clear();
        if (pr) pr->clear();
        return kmx::set_error(st, who + msg);
    };
    if (L.nr != A.nr) return refuse(KMX_ERR_INVALID_ARGUMENT, "the alignments handle's nr differs from the loci handle's");
    if (L.nr & 3) return refuse(KMX_ERR_INVALID_ARGUMENT, "the number of reads is no multiple of 4: not the loci of a doubled batch of pairs");
    if (A.n_loci != L.n_loci) return refuse(KMX_ERR_INVALID_ARGUMENT, "the alignments handle's n_loci differs from the loci handle's");
    if (A.device != L.device) return refuse(KMX_ERR_INVALID_ARGUMENT, "the loci and the alignments live on different devices");
    kmx::DeviceGuard dg;
    kmx_status bound = kmx::bind_handle(inout_placements, L.device);
    if (bound == KMX_OK) bound = kmx::bind_handle(inout_pairs, L.device);
    pl = *inout_placements;
    pr = *inout_pairs;
    if (bound != KMX_OK) {
        if (pl) pl->clear();
        if (pr) pr->clear();
        return bound;
    }
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : A.stream;
    const kmx_status st = pair_fold_run(L, A, *o, s, pl, pr);
    if (st != KMX_OK) {                                        // both handles hold an empty result, not half of this one
        (void)hipStreamSynchronize(s);
        pl->clear();
        pr->clear();
    }
    return st;
}

kmx_status kmx_pairs_counts(const kmx_pairs* p, uint64_t* np, uint64_t* n_concordant, uint64_t* n_discordant, uint64_t* n_single, uint64_t* n_unplaced,
                            uint64_t* n_ambiguous)
{
    if (!p) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_pairs_counts: pairs handle is NULL");
    if (np) *np = p->np;
    if (n_concordant) *n_concordant = p->n_concordant;
    if (n_discordant) *n_discordant = p->n_discordant;
    if (n_single) *n_single = p->n_single;
    if (n_unplaced) *n_unplaced = p->n_unplaced;
    if (n_ambiguous) *n_ambiguous = p->n_ambiguous;
    return KMX_OK;
}

kmx_status kmx_pairs_view_device(const kmx_pairs* p, const uint8_t** d_cls, const int32_t** d_tlen, const uint16_t** d_score,
                                 const uint16_t** d_second_score)
{
    if (!p) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_pairs_view_device: pairs handle is NULL");
    if (d_cls) *d_cls = p->cls.dev();
    if (d_tlen) *d_tlen = p->tlen.dev();
    if (d_score) *d_score = p->score.dev();
    if (d_second_score) *d_second_score = p->second_score.dev();
    return KMX_OK;
}

kmx_status kmx_pairs_view(kmx_pairs* p, const uint8_t** cls, const int32_t** tlen, const uint16_t** score, const uint16_t** second_score)
{
    if (!p) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_pairs_view: pairs handle is NULL");
    TRY_KMX(kmx::host_view("kmx_pairs_view", *p));             // 9 bytes per pair
    if (cls) *cls = p->cls.host();
    if (tlen) *tlen = p->tlen.host();
    if (score) *score = p->score.host();
    if (second_score) *second_score = p->second_score.host();
    return KMX_OK;
}

void kmx_pairs_free(kmx_pairs* p) { kmx::free_handle(p); }

} // extern "C"
