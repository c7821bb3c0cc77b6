// Supplementary alignments of the read-mapping chain (kmx_clips_supplementaries; include/kmx.h, KMX_MAP_SUPPLEMENTARY): the parts of a
// split read.  Among the clipped entries of both strands of a read (the KMX_SCRIPT_ALL scripts of the doubled batch and their clips),
// up to N that cover read letters which the primary and the parts taken before do not cover, chosen greedily by (score, entry).
// Only per-entry values of the clips are read: the parts are the best-scoring parts of the edit-optimal scripts, not realignments.
//
//   k_supp_pick        a wave per public read.  The wave finds the primary's entry p with a strided search of the read's sel range
//                      and a min-reduction.  T, the parts taken so far (the primary first), lives in LDS: entry and read interval of
//                      at most N + 1 members per wave.  A round: the lanes stride over the entries of both strands, test every
//                      candidate against all of T, keep the greatest key score << 32 | ~e, and the wave max-reduces with
//                      __shfl_xor; lane 0 appends the winner to T and to picks[i N + j], in greedy order.  One more round without
//                      an append decides `more`.  Lane 0 writes cnt[i], prim[i] and more[i]; the batch totals go through LDS and one
//                      atomic per workgroup.  There is one path for every read, however many entries it has
//                      (kmx::launch_scan over cnt gives sup_off and n_sup)
//   k_supp_write       a wave per public read: lane j holds pick j and its rank, the number of smaller picks; for every pick one
//                      more strided pass over the candidates and a max-reduction give its second_score; lane j writes entry
//                      sup_off[i] + rank
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "kmx_kernels.h"
#include "kmx_strands.h"
#include "kmx_vote.h"

namespace {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kWave = 64;
constexpr uint32_t kWaves = kBlock / kWave;
constexpr uint32_t kMaxT = KMX_SUPPLEMENTARY_MAX + 1;
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kMaxRead = 65535;                           // the read length that is looked at (q0 and q1 are 16-bit)
enum { CTR_N_SUP = 0, CTR_N_SPLIT, CTR_N_TRUNCATED, CTR_COUNT };
static_assert(KMX_SUPPLEMENTARY_MAX <= kWave, "k_supp_write holds a pick per lane");

using kmx::Buf;
using Pinned = kmx::PinnedArr;
using kmx::grid_for;

// the doubled reads, the alignments, the placements, the all-loci scripts and their clips, the options
struct SupIn {
    const uint64_t* roff2;         // [2 nr + 1]
    const uint32_t* start;         // [n_loci]
    const uint32_t* end;
    const uint32_t* ctg;           // [n_loci], or nullptr
    const uint32_t* pl_locus;      // [nr]
    const uint8_t* pl_strand;
    const uint64_t* read_sel_off;  // [2 nr + 1]
    const uint32_t* sel;           // [n_sel]
    const int32_t* score;          // [n_sel]: the clips'
    const uint16_t* sl;
    const uint16_t* sr;
    const uint16_t* tl;
    const uint16_t* tr;
    const uint16_t* nm;
    const uint8_t* cflags;
    const uint64_t* cig_off;       // [n_sel + 1]
    uint64_t nr;                   // public reads
    uint32_t n_loci, n_sel;        // (clamped by the caller: kmx_loci_align leaves n_loci, and so n_sel, below 2^32)
    int32_t min_len, max_overlap, min_score;   // max_overlap clamped at kMaxRead, which no overlap exceeds
    uint32_t N;
};

// the entries of public read i: [ea, eb) forward, [eb, ec) reverse, inside the arrays whatever the offsets hold; m: its letters
struct Range {
    uint32_t ea, eb, ec;
    int32_t m;
};

__device__ __forceinline__ Range range_of(const SupIn& F, uint64_t i)
{
    Range R;
    R.ea = uint32_t(min(F.read_sel_off[2 * i], uint64_t(F.n_sel)));
    R.eb = uint32_t(min(max(F.read_sel_off[2 * i + 1], uint64_t(R.ea)), uint64_t(F.n_sel)));
    R.ec = uint32_t(min(max(F.read_sel_off[2 * i + 2], uint64_t(R.eb)), uint64_t(F.n_sel)));
    R.m = int32_t(min(F.roff2[2 * i + 1] - F.roff2[2 * i], uint64_t(kMaxRead)));
    return R;
}

// what entry e covers of the original read, and whether it is a candidate (e < n_sel)
struct Part {
    int32_t q0, q1, score;
    bool runs, cand;
};

__device__ __forceinline__ Part part_of(const SupIn& F, const Range& R, uint64_t e)
{
    Part P;
    const bool fwd = e < R.eb;
    const int32_t l = F.sl[e], r = F.sr[e];
    P.q0 = fwd ? l : r;
    P.q1 = R.m - (fwd ? r : l);
    P.score = F.score[e];
    P.runs = F.cig_off[e + 1] > F.cig_off[e];
    P.cand = P.runs && !(F.cflags[e] & KMX_CLIP_LOW) && F.sel[e] < F.n_loci && P.score >= F.min_score && P.q1 - P.q0 >= F.min_len;
    return P;
}

// (every q lies in [-kMaxRead, kMaxRead]: 32 bits hold the differences)
__device__ __forceinline__ int32_t overlap(int32_t a0, int32_t a1, int32_t b0, int32_t b1) { return max(0, min(a1, b1) - max(a0, b0)); }

__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(kBlock) void k_supp_pick(SupIn F, uint32_t* __restrict__ picks, uint32_t* __restrict__ cnt, uint32_t* __restrict__ prim,
                                                      uint8_t* __restrict__ more, unsigned long long* __restrict__ ctr)
{
    __shared__ uint32_t t_ent[kWaves][kMaxT];
    __shared__ int32_t t_q0[kWaves][kMaxT], t_q1[kWaves][kMaxT];
    __shared__ unsigned int s_split, s_trunc;
    if (threadIdx.x == 0) { s_split = 0; s_trunc = 0; }
    __syncthreads();
    const uint32_t lane = threadIdx.x % kWave, wv = threadIdx.x / kWave;
    const uint64_t i = uint64_t(blockIdx.x) * kWaves + wv;
    if (i < F.nr) {
        const Range R = range_of(F, i);
        const uint32_t pl = F.pl_locus[i];
        // the primary's entry: the least e of the read with sel[e] == locus[i]; none for an unplaced or a rescued read
        uint32_t p = kNone;
        if (F.pl_strand[i] != 255 && pl != kNone)
            for (uint64_t e = uint64_t(R.ea) + lane; e < R.ec; e += kWave)
                if (F.sel[e] == pl) p = min(p, uint32_t(e));
        for (int off = kWave / 2; off > 0; off >>= 1) p = min(p, uint32_t(__shfl_xor(p, off)));
        uint32_t* te = t_ent[wv];
        int32_t* t0 = t_q0[wv];
        int32_t* t1 = t_q1[wv];
        bool go = p != kNone;                                  // (the same in every lane)
        if (go) {
            const Part P = part_of(F, R, p);
            go = P.runs;
            if (lane == 0) { te[0] = p; t0[0] = P.q0; t1[0] = P.q1; }
        }
        wave_sync();
        uint32_t taken = 0, trunc = 0;
        while (go) {
            uint64_t key = 0;                                  // a candidate's key is above 0: its score is at least 1
            for (uint64_t e = uint64_t(R.ea) + lane; e < R.ec; e += kWave) {
                const Part c = part_of(F, R, e);
                if (!c.cand) continue;
                bool live = true;                              // not taken (nor the primary), and within max_overlap of every member of T
                for (uint32_t t = 0; t <= taken && live; ++t)
                    live = te[t] != uint32_t(e) && overlap(c.q0, c.q1, t0[t], t1[t]) <= F.max_overlap;
                if (live) key = max(key, (uint64_t(uint32_t(c.score)) << 32) | (kNone - uint32_t(e)));
            }
            for (int off = kWave / 2; off > 0; off >>= 1) key = max(key, uint64_t(__shfl_xor((unsigned long long)key, off)));
            if (key == 0) break;
            if (taken == F.N) { trunc = 1; break; }
            const uint32_t e = kNone - uint32_t(key);          // in [ea, ec): below n_sel
            if (lane == 0) {
                const Part c = part_of(F, R, e);
                te[taken + 1] = e;
                t0[taken + 1] = c.q0;
                t1[taken + 1] = c.q1;
                picks[i * F.N + taken] = e;
            }
            ++taken;
            wave_sync();
        }
        if (lane == 0) {
            cnt[i] = taken;
            prim[i] = p;
            more[i] = uint8_t(trunc);
            if (taken) atomicAdd(&s_split, 1u);
            if (trunc) atomicAdd(&s_trunc, 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_split) atomicAdd(&ctr[CTR_N_SPLIT], (unsigned long long)s_split);
        if (s_trunc) atomicAdd(&ctr[CTR_N_TRUNCATED], (unsigned long long)s_trunc);
    }
}

// the entry arrays; n_sup bounds every store
struct SupOut {
    uint32_t* ent;                 // [n_sup]
    uint32_t* locus;
    uint8_t* strand;
    uint16_t* q0;
    uint16_t* q1;
    uint32_t* t0;
    uint32_t* t1;
    int32_t* score;
    int32_t* second;
    uint16_t* nm;
    uint32_t* ctg;                 // or nullptr
    uint64_t n_sup;
};

__global__ __launch_bounds__(kBlock) void k_supp_write(SupIn F, const uint32_t* __restrict__ picks, const uint32_t* __restrict__ prim,
                                                       const uint64_t* __restrict__ sup_off, SupOut O)
{
    const uint32_t lane = threadIdx.x % kWave;
    const uint64_t i = uint64_t(blockIdx.x) * kWaves + threadIdx.x / kWave;
    if (i >= F.nr) return;
    const uint64_t e0 = sup_off[i], e1 = sup_off[i + 1];
    const uint32_t n = uint32_t(min(e1 >= e0 ? e1 - e0 : uint64_t(0), uint64_t(F.N)));   // (the picks of this read: at most N)
    if (n == 0) return;
    const Range R = range_of(F, i);
    const uint32_t p = prim[i];
    const uint32_t mine = lane < n ? picks[i * F.N + lane] : kNone;
    uint32_t rank = 0;
    int32_t second = 0;
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t x = uint32_t(__shfl(mine, int(k)));     // (the same in every lane)
        rank += x < mine ? 1u : 0u;
        if (x < R.ea || x >= R.ec) continue;                   // (never: the picks are entries of this read)
        const Part X = part_of(F, R, x);
        if (!X.cand) continue;                                 // (never: a pick is a candidate, so its sel is below n_loci)
        const uint32_t xl = F.sel[x];
        const bool xf = x < R.eb;
        const int64_t x0 = int64_t(F.start[xl]) + F.tl[x], x1 = int64_t(F.end[xl]) - F.tr[x];
        int32_t best = 0;                                      // the runner-up: the best candidate on the same read letters, elsewhere in the text
        for (uint64_t e = uint64_t(R.ea) + lane; e < R.ec; e += kWave) {
            if (e == x || e == p) continue;
            const Part c = part_of(F, R, e);
            if (!c.cand || overlap(c.q0, c.q1, X.q0, X.q1) <= F.max_overlap) continue;
            const uint32_t l = F.sel[e];                       // below n_loci: a candidate
            const int64_t c0 = int64_t(F.start[l]) + F.tl[e], c1 = int64_t(F.end[l]) - F.tr[e];
            if ((e < R.eb) != xf || max(c0, x0) >= min(c1, x1)) best = max(best, c.score);
        }
        for (int off = kWave / 2; off > 0; off >>= 1) best = max(best, __shfl_xor(best, off));
        if (lane == k) second = best;
    }
    const uint64_t o = e0 + rank;
    if (lane >= n || o >= O.n_sup || mine < R.ea || mine >= R.ec) return;
    const uint32_t l = F.sel[mine];
    if (l >= F.n_loci) return;                                 // (never: a pick is a candidate)
    const Part M = part_of(F, R, mine);
    O.ent[o] = mine;
    O.locus[o] = l;
    O.strand[o] = mine < R.eb ? uint8_t(0) : uint8_t(1);
    O.q0[o] = uint16_t(M.q0);
    O.q1[o] = uint16_t(M.q1);
    O.t0[o] = uint32_t(int64_t(F.start[l]) + F.tl[mine]);
    O.t1[o] = uint32_t(int64_t(F.end[l]) - F.tr[mine]);
    O.score[o] = M.score;
    O.second[o] = second;
    O.nm[o] = F.nm[mine];
    if (O.ctg) O.ctg[o] = F.ctg[l];
}

} // namespace

struct kmx_supplementaries {
    int device = 0;
    hipStream_t stream = nullptr;          // the stream of the call that filled the handle (the host view copies on it)
    uint64_t nr = 0, n_sup = 0, n_split = 0, n_truncated = 0;
    bool has_ctg = false;                  // the alignments carried a contig table: ctg holds n_sup entries
    // results: the offsets and more per public read, one entry per part
    kmx::ArrOf<uint64_t> sup_off{kmx::ARR_OFFSETS};
    kmx::ArrOf<uint32_t> ent, locus, t0, t1, ctg;
    kmx::ArrOf<int32_t> score, second;
    kmx::ArrOf<uint16_t> q0, q1, nm;
    kmx::ArrOf<uint8_t> strand, more;
    // scratch
    Buf picks, cnt, prim, bsum, ctr;
    Pinned h_ctr;
    bool host_valid = false;
    std::vector<kmx::Arr*> results() { return {&sup_off, &ent, &locus, &strand, &q0, &q1, &t0, &t1, &score, &second, &nm, &ctg, &more}; }
    std::vector<Buf*> scratch() { return {&picks, &cnt, &prim, &bsum, &ctr}; }
    void release() { kmx::release_arrays(*this); }
    void clear() { nr = n_sup = n_split = n_truncated = 0; has_ctg = false; kmx::clear_arrays(*this); }
    // a call has succeeded: the arrays expose what the counters say
    void expose()
    {
        kmx::expose(results(), n_sup);
        sup_off.n = nr + 1;
        more.n = nr;
        if (!has_ctg) ctg.n = 0;
    }
};

namespace {

kmx_status supplementaries_run(const kmx_strand_reads* reads, const kmx::AlignAccess& A, const kmx::PlacementsAccess& P, const kmx::ScriptsAccess& S,
                               const kmx::ClipsAccess& C, const kmx_supplementary_options& o, hipStream_t s, kmx_supplementaries* h)
{
    const uint64_t nr = reads->nr2 / 2;
    TRY_HIP(h->sup_off.ensure((nr + 1) * 8));
    if (nr == 0) {                                             // no read: no launch indexes an empty array
        TRY_HIP(hipMemsetAsync(h->sup_off.p, 0, 8, s));
        h->expose();
        return KMX_OK;
    }
    const uint32_t N = o.max_supplementary;
    TRY_HIP(h->picks.ensure(nr * N * 4));
    TRY_HIP(h->cnt.ensure(nr * 4 + 16));
    TRY_HIP(h->prim.ensure(nr * 4));
    TRY_HIP(h->bsum.ensure(kmx::scan_blocks(nr) * 8 + 16));
    TRY_HIP(h->more.ensure(nr));
    TRY_HIP(h->ctr.ensure(CTR_COUNT * 8));
    unsigned long long* ctr = h->ctr.as<unsigned long long>();
    TRY_HIP(hipMemsetAsync(ctr, 0, CTR_COUNT * 8, s));
    const SupIn F{reads->roff2.as<uint64_t>(), A.start, A.end, A.ctg, P.locus, P.strand, S.read_sel_off, S.sel, C.score, C.sl, C.sr, C.tl, C.tr, C.nm,
                  C.cflags, C.cig_off, nr, uint32_t(std::min<uint64_t>(A.n_loci, 0xFFFFFFFFull)), uint32_t(std::min<uint64_t>(S.n_sel, 0xFFFFFFFFull)),
                  int32_t(o.min_len), int32_t(std::min(o.max_overlap, kMaxRead)), o.min_score, N};
    const dim3 grid(grid_for(nr, kWaves)), block(kBlock);
    hipLaunchKernelGGL(k_supp_pick, grid, block, 0, s, F, h->picks.as<uint32_t>(), h->cnt.as<uint32_t>(), h->prim.as<uint32_t>(), h->more.as<uint8_t>(), ctr);
    kmx::launch_scan(s, h->cnt.as<uint32_t>(), nr, h->bsum.as<uint64_t>(), h->sup_off.as<uint64_t>(), ctr + CTR_N_SUP);
    TRY_HIP(hipGetLastError());
    TRY_KMX(kmx::read_back("kmx_clips_supplementaries", s, ctr, h->h_ctr, CTR_COUNT * 8));
    const uint64_t n_sup = h->h_ctr.as<uint64_t>()[CTR_N_SUP];
    if (n_sup > nr * N) return kmx::set_error(KMX_ERR_HIP, "kmx_clips_supplementaries: more entries than N per read");   // (never: a guard for the arrays)
    if (n_sup) {
        for (Buf* b : std::initializer_list<Buf*>{&h->ent, &h->locus, &h->t0, &h->t1, &h->score, &h->second}) TRY_HIP(b->ensure(n_sup * 4));
        for (Buf* b : {&h->q0, &h->q1, &h->nm}) TRY_HIP(b->ensure(n_sup * 2));
        TRY_HIP(h->strand.ensure(n_sup));
        if (A.ctg) TRY_HIP(h->ctg.ensure(n_sup * 4));
        const SupOut O{h->ent.as<uint32_t>(), h->locus.as<uint32_t>(), h->strand.as<uint8_t>(), h->q0.as<uint16_t>(), h->q1.as<uint16_t>(),
                       h->t0.as<uint32_t>(), h->t1.as<uint32_t>(), h->score.as<int32_t>(), h->second.as<int32_t>(), h->nm.as<uint16_t>(),
                       A.ctg ? h->ctg.as<uint32_t>() : nullptr, n_sup};
        hipLaunchKernelGGL(k_supp_write, grid, block, 0, s, F, h->picks.as<uint32_t>(), h->prim.as<uint32_t>(), h->sup_off.as<uint64_t>(), O);
        TRY_HIP(hipGetLastError());
    }
    h->nr = nr;
    h->n_sup = n_sup;
    h->n_split = h->h_ctr.as<uint64_t>()[CTR_N_SPLIT];
    h->n_truncated = h->h_ctr.as<uint64_t>()[CTR_N_TRUNCATED];
    h->has_ctg = A.ctg != nullptr;
    h->expose();
    return KMX_OK;
}

} // namespace

extern "C" {

kmx_status kmx_clips_supplementaries(const kmx_strand_reads* reads, const kmx_loci* loci, const kmx_alignments* alignments,
                                     const kmx_placements* placements, const kmx_scripts* scripts, const kmx_clips* clips,
                                     const kmx_supplementary_options* o, void* stream, kmx_supplementaries** inout)
{
    const std::string who = "kmx_clips_supplementaries: ";
    TRY_KMX(kmx::check_call(who, o, inout));
    if (o->flags != 0) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "flags must be 0");
    if (o->max_supplementary == 0 || o->max_supplementary > KMX_SUPPLEMENTARY_MAX)
        return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "max_supplementary is not in 1 .. KMX_SUPPLEMENTARY_MAX");
    if (o->min_len == 0 || o->min_len > 65535) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "min_len is not in 1 .. 65535");
    if (o->min_score < 1) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "min_score is below 1");
    if (!reads) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "strand reads handle is NULL");
    if (!loci) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "loci handle is NULL");
    if (!alignments) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "alignments handle is NULL");
    if (!placements) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "placements handle is NULL");
    if (!scripts) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "scripts handle is NULL");
    if (!clips) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "clips handle is NULL");
    const kmx::LociAccess L = kmx::loci_access(loci);
    const kmx::AlignAccess A = kmx::alignments_access(alignments);
    const kmx::PlacementsAccess P = kmx::placements_access(placements);
    const kmx::ScriptsAccess S = kmx::scripts_access(scripts);
    const kmx::ClipsAccess C = kmx::clips_access(clips);
    const uint64_t nr2 = reads->nr2;
    kmx_supplementaries* h = *inout;
    auto refuse = kmx::refuser(who, h);
    if (nr2 & 1) return refuse(KMX_ERR_INVALID_ARGUMENT, "an odd number of reads: not a doubled batch");
    if (L.nr != nr2) return refuse(KMX_ERR_INVALID_ARGUMENT, "the loci handle's nr differs from the reads' nr2");
    if (A.nr != nr2) return refuse(KMX_ERR_INVALID_ARGUMENT, "the alignments handle's nr differs from the reads' nr2");
    if (A.n_loci != L.n_loci) return refuse(KMX_ERR_INVALID_ARGUMENT, "the alignments handle's n_loci differs from the loci handle's");
    if (P.nr2 != nr2) return refuse(KMX_ERR_INVALID_ARGUMENT, "the placements are not those of these reads: nr differs");
    if (S.nr != nr2) return refuse(KMX_ERR_INVALID_ARGUMENT, "the scripts are not those of these reads: nr differs");
    if (S.flags & KMX_SCRIPT_M) return refuse(KMX_ERR_INVALID_ARGUMENT, "the scripts were made with KMX_SCRIPT_M: their clips carry no score");
    if (C.n_sel != S.n_sel) return refuse(KMX_ERR_INVALID_ARGUMENT, "the clips are not those of these scripts: n_sel differs");
    if (nr2 && (L.device != reads->device || A.device != reads->device || P.device != reads->device || S.device != reads->device ||
                (S.n_sel && C.device != reads->device)))
        return refuse(KMX_ERR_INVALID_ARGUMENT, "the handles live on different devices");
    if ((nr2 / 2) * uint64_t(o->max_supplementary) >= (uint64_t(1) << 32))
        return refuse(KMX_ERR_TOO_LARGE, "nr * max_supplementary is 2^32 or more: split the batch");
    kmx::DeviceGuard dg;
    TRY_KMX(kmx::bind_handle(inout, reads->device));
    h = *inout;
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : C.stream;
    return kmx::run_into(h, s, [&] { return supplementaries_run(reads, A, P, S, C, *o, s, h); });
}

kmx_status kmx_supplementaries_counts(const kmx_supplementaries* h, uint64_t* nr, uint64_t* n_sup, uint64_t* n_split, uint64_t* n_truncated)
{
    if (!h) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_supplementaries_counts: supplementaries handle is NULL");
    if (nr) *nr = h->nr;
    if (n_sup) *n_sup = h->n_sup;
    if (n_split) *n_split = h->n_split;
    if (n_truncated) *n_truncated = h->n_truncated;
    return KMX_OK;
}

kmx_status kmx_supplementaries_view_device(const kmx_supplementaries* h, const uint64_t** d_sup_off, const uint32_t** d_ent, const uint32_t** d_locus,
                                           const uint8_t** d_strand, const uint16_t** d_q0, const uint16_t** d_q1, const uint32_t** d_t0,
                                           const uint32_t** d_t1, const int32_t** d_score, const int32_t** d_second_score, const uint16_t** d_nm,
                                           const uint32_t** d_ctg, const uint8_t** d_more)
{
    if (!h) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_supplementaries_view_device: supplementaries handle is NULL");
    if (d_sup_off) *d_sup_off = h->sup_off.dev();
    if (d_ent) *d_ent = h->ent.dev();
    if (d_locus) *d_locus = h->locus.dev();
    if (d_strand) *d_strand = h->strand.dev();
    if (d_q0) *d_q0 = h->q0.dev();
    if (d_q1) *d_q1 = h->q1.dev();
    if (d_t0) *d_t0 = h->t0.dev();
    if (d_t1) *d_t1 = h->t1.dev();
    if (d_score) *d_score = h->score.dev();
    if (d_second_score) *d_second_score = h->second.dev();
    if (d_nm) *d_nm = h->nm.dev();
    if (d_ctg) *d_ctg = h->ctg.dev();
    if (d_more) *d_more = h->more.dev();
    return KMX_OK;
}

kmx_status kmx_supplementaries_view(kmx_supplementaries* h, const uint64_t** sup_off, const uint32_t** ent, const uint32_t** locus, const uint8_t** strand,
                                    const uint16_t** q0, const uint16_t** q1, const uint32_t** t0, const uint32_t** t1, const int32_t** score,
                                    const int32_t** second_score, const uint16_t** nm, const uint32_t** ctg, const uint8_t** more)
{
    if (!h) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_supplementaries_view: supplementaries handle is NULL");
    TRY_KMX(kmx::host_view("kmx_supplementaries_view", *h));   // 8 + 1 bytes per public read, 31 per entry (35 with ctg)
    if (sup_off) *sup_off = h->sup_off.host();
    if (ent) *ent = h->ent.host();
    if (locus) *locus = h->locus.host();
    if (strand) *strand = h->strand.host();
    if (q0) *q0 = h->q0.host();
    if (q1) *q1 = h->q1.host();
    if (t0) *t0 = h->t0.host();
    if (t1) *t1 = h->t1.host();
    if (score) *score = h->score.host();
    if (second_score) *second_score = h->second.host();
    if (nm) *nm = h->nm.host();
    if (ctg) *ctg = h->has_ctg ? h->ctg.host() : nullptr;
    if (more) *more = h->more.host();
    return KMX_OK;
}

void kmx_supplementaries_free(kmx_supplementaries* h) { kmx::free_handle(h); }

} // extern "C"
