// Secondary placements of the read-mapping chain (kmx_placements_secondaries, kmx_secondaries_scripts; include/kmx.h,
// KMX_MAP_SECONDARIES): up to N further places per read, chosen among the aligned loci of both strands by the ELSEWHERE rule of
// kmx_alignments_fold_strands applied transitively, so that two loci that describe one place give one entry.
//
//   k_sec_pick         a wave per public read.  T, the places taken so far (the primary first), lives in LDS: locus, strand, start and
//                      end of at most N + 1 members per wave.  A round: the lanes stride over the loci of both strands, test every live
//                      candidate against all of T, keep the least key dist << 32 | l, and the wave min-reduces with __shfl_xor;
//                      lane 0 appends the winner to T and to picks[i N + j], in greedy order.  One more round without an append
//                      decides `more`.  Lane 0 writes cnt[2i], cnt[2i + 1] and more[i]; the batch totals go through LDS and one
//                      atomic per workgroup.  There is one path for every read, however many loci it has
//                      (kmx::launch_scan over cnt gives sec_off and n_sec)
//   k_sec_write        a wave per public read: lane j holds pick j, its rank is the number of smaller picks (the picks of a read are
//                      distinct), and it gathers dist / start / end (and ctg) of its locus into entry sec_off[2i] + rank
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "kmx_fold_core.h"
#include "kmx_kernels.h"
#include "kmx_strands.h"
#include "kmx_vote.h"

namespace {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kWave = 64;
constexpr uint32_t kWaves = kBlock / kWave;
constexpr uint32_t kMaxT = KMX_SECONDARY_MAX + 1;
constexpr uint32_t kNoBest = 0xFFFFFFFFu;
constexpr uint64_t kNoKey = ~uint64_t(0);
enum { CTR_N_SEC = 0, CTR_N_MULTI, CTR_N_TRUNCATED, CTR_COUNT };
static_assert(KMX_SECONDARY_MAX <= kWave, "k_sec_write holds a pick per lane");

using kmx::Buf;
using Pinned = kmx::PinnedArr;
using kmx::grid_for;

// the loci and alignments of the doubled batch, the placements, the options
struct SecIn {
    const uint64_t* locus_off;     // [2 nr + 1]
    const uint8_t* dist;           // [n_loci]
    const uint32_t* start;
    const uint32_t* end;
    const uint32_t* ctg;           // [n_loci], or nullptr
    const uint32_t* pl_locus;      // [nr]
    const uint8_t* pl_strand;
    const uint8_t* pl_dist;
    const uint32_t* pl_start;
    const uint32_t* pl_end;
    uint64_t nr, n_loci;           // public reads; n_loci < 2^32 (clamped by the caller)
    uint32_t N, max_delta;
};

__global__ __launch_bounds__(kBlock) void k_sec_pick(SecIn F, uint32_t* __restrict__ picks, uint32_t* __restrict__ cnt, uint8_t* __restrict__ more,
                                                     unsigned long long* __restrict__ ctr)
{
    __shared__ uint32_t t_locus[kWaves][kMaxT], t_strand[kWaves][kMaxT], t_start[kWaves][kMaxT], t_end[kWaves][kMaxT];
    __shared__ unsigned int s_multi, s_trunc;
    if (threadIdx.x == 0) { s_multi = 0; s_trunc = 0; }
    __syncthreads();
    const uint32_t lane = threadIdx.x % kWave, wv = threadIdx.x / kWave;
    const uint64_t i = uint64_t(blockIdx.x) * kWaves + wv;
    if (i < F.nr) {
        uint64_t a, b, c;
        strand_ranges(F.locus_off, F.n_loci, 2 * i, &a, &b, &c);
        const uint32_t ps = F.pl_strand[i];
        const bool placed = ps != 255;                         // (a foreign strand of 2 .. 254 is a place that no locus overlaps)
        const int64_t limit = int64_t(F.pl_dist[i]) + int64_t(F.max_delta);
        uint32_t* tl = t_locus[wv];
        uint32_t* ts = t_strand[wv];
        uint32_t* t0 = t_start[wv];
        uint32_t* t1 = t_end[wv];
        if (lane == 0) { tl[0] = F.pl_locus[i]; ts[0] = ps; t0[0] = F.pl_start[i]; t1[0] = F.pl_end[i]; }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        uint32_t taken = 0, fwd = 0, trunc = 0;
        while (placed) {                                       // (the same in every lane)
            uint64_t key = kNoKey;
            for (uint64_t l = a + lane; l < c; l += kWave) {
                const uint32_t d = F.dist[l];
                if (d >= KMX_ALIGN_SKIPPED || int64_t(d) > limit) continue;
                const uint32_t s = l < b ? 0u : 1u, x0 = F.start[l], x1 = F.end[l];
                bool live = true;                              // not taken, and elsewhere from every member of T
                for (uint32_t t = 0; t <= taken && live; ++t)
                    live = tl[t] != uint32_t(l) && elsewhere(s, x0, x1, ts[t], t0[t], t1[t]);
                if (live) key = min(key, (uint64_t(d) << 32) | l);
            }
            for (int off = kWave / 2; off > 0; off >>= 1) key = min(key, uint64_t(__shfl_xor((unsigned long long)key, off)));
            if (key == kNoKey) break;
            if (taken == F.N) { trunc = 1; break; }
            const uint32_t l = uint32_t(key);                  // in [a, c): below n_loci
            if (lane == 0) {
                tl[taken + 1] = l;
                ts[taken + 1] = l < b ? 0u : 1u;
                t0[taken + 1] = F.start[l];
                t1[taken + 1] = F.end[l];
                picks[i * F.N + taken] = l;
            }
            if (l < b) ++fwd;
            ++taken;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
        if (lane == 0) {
            cnt[2 * i] = fwd;
            cnt[2 * i + 1] = taken - fwd;
            more[i] = uint8_t(trunc);
            if (taken) atomicAdd(&s_multi, 1u);
            if (trunc) atomicAdd(&s_trunc, 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_multi) atomicAdd(&ctr[CTR_N_MULTI], (unsigned long long)s_multi);
        if (s_trunc) atomicAdd(&ctr[CTR_N_TRUNCATED], (unsigned long long)s_trunc);
    }
}

// the entry arrays; n_sec bounds every store
struct SecOut {
    uint32_t* locus;               // [n_sec]
    uint8_t* dist;
    uint32_t* start;
    uint32_t* end;
    uint32_t* ctg;                 // or nullptr
    uint64_t n_sec;
};

__global__ __launch_bounds__(kBlock) void k_sec_write(SecIn F, const uint32_t* __restrict__ picks, const uint64_t* __restrict__ sec_off, SecOut O)
{
    const uint32_t lane = threadIdx.x % kWave;
    const uint64_t i = uint64_t(blockIdx.x) * kWaves + threadIdx.x / kWave;
    if (i >= F.nr) return;
    const uint64_t e0 = sec_off[2 * i], e1 = sec_off[2 * i + 2];
    const uint32_t n = uint32_t(min(e1 >= e0 ? e1 - e0 : uint64_t(0), uint64_t(F.N)));   // (the picks of this read: at most N)
    const uint32_t mine = lane < n ? picks[i * F.N + lane] : kNoBest;
    uint32_t rank = 0;
    for (uint32_t k = 0; k < n; ++k) rank += uint32_t(__shfl(mine, int(k))) < mine ? 1u : 0u;
    const uint64_t e = e0 + rank;
    if (lane >= n || e >= O.n_sec || mine >= F.n_loci) return;
    O.locus[e] = mine;
    O.dist[e] = F.dist[mine];
    O.start[e] = F.start[mine];
    O.end[e] = F.end[mine];
    if (O.ctg) O.ctg[e] = F.ctg[mine];
}

} // namespace

struct kmx_secondaries {
    int device = 0;
    hipStream_t stream = nullptr;          // the stream of the call that filled the handle (the host view copies on it)
    uint64_t nr = 0, n_sec = 0, n_multi = 0, n_truncated = 0;
    bool has_ctg = false;                  // the alignments carried a contig table: ctg holds n_sec entries
    // results: the offsets per internal read, one entry per place, more per public read
    kmx::ArrOf<uint64_t> sec_off{kmx::ARR_OFFSETS};
    kmx::ArrOf<uint32_t> locus, start, end, ctg;
    kmx::ArrOf<uint8_t> dist, more;
    // scratch
    Buf picks, cnt, bsum, ctr;
    Pinned h_ctr;
    bool host_valid = false;
    std::vector<kmx::Arr*> results() { return {&sec_off, &locus, &dist, &start, &end, &ctg, &more}; }
    std::vector<Buf*> scratch() { return {&picks, &cnt, &bsum, &ctr}; }
    void release() { kmx::release_arrays(*this); }
    void clear() { nr = n_sec = n_multi = n_truncated = 0; has_ctg = false; kmx::clear_arrays(*this); }
    // a call has succeeded: the arrays expose what the counters say
    void expose()
    {
        kmx::expose(results(), n_sec);
        sec_off.n = 2 * nr + 1;
        more.n = nr;
        if (!has_ctg) ctg.n = 0;
    }
};

kmx::JobsAccess kmx::secondaries_access(const kmx_secondaries* h)
{
    return JobsAccess{h->device, h->stream, h->n_sec, h->start.as<uint32_t>(), h->end.as<uint32_t>()};
}

namespace {

kmx_status secondaries_run(const kmx::LociAccess& L, const kmx::AlignAccess& A, const kmx::PlacementsAccess& P, const kmx_secondary_options& o,
                           hipStream_t s, kmx_secondaries* h)
{
    const uint64_t nr2 = L.nr, nr = nr2 / 2;
    TRY_HIP(h->sec_off.ensure((nr2 + 1) * 8));
    if (nr == 0) {                                             // no read: no launch indexes an empty array
        TRY_HIP(hipMemsetAsync(h->sec_off.p, 0, 8, s));
        h->expose();
        return KMX_OK;
    }
    const uint32_t N = o.max_secondary;
    TRY_HIP(h->picks.ensure(nr * N * 4));
    TRY_HIP(h->cnt.ensure(nr2 * 4 + 16));
    TRY_HIP(h->bsum.ensure(kmx::scan_blocks(nr2) * 8 + 16));
    TRY_HIP(h->more.ensure(nr));
    TRY_HIP(h->ctr.ensure(CTR_COUNT * 8));
    unsigned long long* ctr = h->ctr.as<unsigned long long>();
    TRY_HIP(hipMemsetAsync(ctr, 0, CTR_COUNT * 8, s));
    const SecIn F{L.locus_off, A.dist, A.start, A.end, A.ctg, P.locus, P.strand, P.dist, P.start, P.end, nr,
                  std::min<uint64_t>(L.n_loci, 0xFFFFFFFFull), N, o.max_delta};
    const dim3 grid(grid_for(nr, kWaves)), block(kBlock);
    hipLaunchKernelGGL(k_sec_pick, grid, block, 0, s, F, h->picks.as<uint32_t>(), h->cnt.as<uint32_t>(), h->more.as<uint8_t>(), ctr);
    kmx::launch_scan(s, h->cnt.as<uint32_t>(), nr2, h->bsum.as<uint64_t>(), h->sec_off.as<uint64_t>(), ctr + CTR_N_SEC);
    TRY_HIP(hipGetLastError());
    TRY_KMX(kmx::read_back("kmx_placements_secondaries", s, ctr, h->h_ctr, CTR_COUNT * 8));
    const uint64_t n_sec = h->h_ctr.as<uint64_t>()[CTR_N_SEC];
    if (n_sec > nr * N) return kmx::set_error(KMX_ERR_HIP, "kmx_placements_secondaries: more entries than N per read");   // (never: a guard for the arrays)
    if (n_sec) {
        for (Buf* b : {&h->locus, &h->start, &h->end}) TRY_HIP(b->ensure(n_sec * 4));
        TRY_HIP(h->dist.ensure(n_sec));
        if (A.ctg) TRY_HIP(h->ctg.ensure(n_sec * 4));
        const SecOut O{h->locus.as<uint32_t>(), h->dist.as<uint8_t>(), h->start.as<uint32_t>(), h->end.as<uint32_t>(),
                       A.ctg ? h->ctg.as<uint32_t>() : nullptr, n_sec};
        hipLaunchKernelGGL(k_sec_write, grid, block, 0, s, F, h->picks.as<uint32_t>(), h->sec_off.as<uint64_t>(), O);
        TRY_HIP(hipGetLastError());
    }
    h->nr = nr;
    h->n_sec = n_sec;
    h->n_multi = h->h_ctr.as<uint64_t>()[CTR_N_MULTI];
    h->n_truncated = h->h_ctr.as<uint64_t>()[CTR_N_TRUNCATED];
    h->has_ctg = A.ctg != nullptr;
    h->expose();
    return KMX_OK;
}

} // namespace

extern "C" {

kmx_status kmx_placements_secondaries(const kmx_loci* loci, const kmx_alignments* alignments, const kmx_placements* placements,
                                      const kmx_secondary_options* o, void* stream, kmx_secondaries** inout)
{
    const std::string who = "kmx_placements_secondaries: ";
    if (!loci) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "loci handle is NULL");
    if (!alignments) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "alignments handle is NULL");
    if (!placements) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "placements handle is NULL");
    TRY_KMX(kmx::check_call(who, o, inout));
    if (o->flags != 0) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "flags must be 0");
    if (o->max_secondary == 0 || o->max_secondary > KMX_SECONDARY_MAX)
        return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "max_secondary is not in 1 .. KMX_SECONDARY_MAX");
    const kmx::LociAccess L = kmx::loci_access(loci);
    const kmx::AlignAccess A = kmx::alignments_access(alignments);
    const kmx::PlacementsAccess P = kmx::placements_access(placements);
    kmx_secondaries* h = *inout;
    auto refuse = kmx::refuser(who, h);
    if (L.nr != A.nr) return refuse(KMX_ERR_INVALID_ARGUMENT, "the alignments handle's nr differs from the loci handle's");
    if (L.nr & 1) return refuse(KMX_ERR_INVALID_ARGUMENT, "an odd number of reads: not the loci of a doubled batch");
    if (A.n_loci != L.n_loci) return refuse(KMX_ERR_INVALID_ARGUMENT, "the alignments handle's n_loci differs from the loci handle's");
    if (P.nr2 != L.nr) return refuse(KMX_ERR_INVALID_ARGUMENT, "the placements are not those of these reads: nr differs");
    if (A.device != L.device || (L.nr && P.device != L.device)) return refuse(KMX_ERR_INVALID_ARGUMENT, "the handles live on different devices");
    if ((L.nr / 2) * uint64_t(o->max_secondary) >= (uint64_t(1) << 32)) return refuse(KMX_ERR_TOO_LARGE, "nr * max_secondary is 2^32 or more: split the batch");
    kmx::DeviceGuard dg;
    TRY_KMX(kmx::bind_handle(inout, L.device));
    h = *inout;
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : P.stream;
    return kmx::run_into(h, s, [&] { return secondaries_run(L, A, P, *o, s, h); });
}

kmx_status kmx_secondaries_counts(const kmx_secondaries* h, uint64_t* nr, uint64_t* n_sec, uint64_t* n_multi, uint64_t* n_truncated)
{
    if (!h) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_secondaries_counts: secondaries handle is NULL");
    if (nr) *nr = h->nr;
    if (n_sec) *n_sec = h->n_sec;
    if (n_multi) *n_multi = h->n_multi;
    if (n_truncated) *n_truncated = h->n_truncated;
    return KMX_OK;
}

kmx_status kmx_secondaries_view_device(const kmx_secondaries* h, const uint64_t** d_sec_off, const uint32_t** d_locus, const uint8_t** d_dist,
                                       const uint32_t** d_start, const uint32_t** d_end, const uint32_t** d_ctg, const uint8_t** d_more)
{
    if (!h) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_secondaries_view_device: secondaries handle is NULL");
    if (d_sec_off) *d_sec_off = h->sec_off.dev();
    if (d_locus) *d_locus = h->locus.dev();
    if (d_dist) *d_dist = h->dist.dev();
    if (d_start) *d_start = h->start.dev();
    if (d_end) *d_end = h->end.dev();
    if (d_ctg) *d_ctg = h->ctg.dev();
    if (d_more) *d_more = h->more.dev();
    return KMX_OK;
}

kmx_status kmx_secondaries_view(kmx_secondaries* h, const uint64_t** sec_off, const uint32_t** locus, const uint8_t** dist, const uint32_t** start,
                                const uint32_t** end, const uint32_t** ctg, const uint8_t** more)
{
    if (!h) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_secondaries_view: secondaries handle is NULL");
    TRY_KMX(kmx::host_view("kmx_secondaries_view", *h));       // 8 bytes per internal read, 1 per public read, 13 per entry (17 with ctg)
    if (sec_off) *sec_off = h->sec_off.host();
    if (locus) *locus = h->locus.host();
    if (dist) *dist = h->dist.host();
    if (start) *start = h->start.host();
    if (end) *end = h->end.host();
    if (ctg) *ctg = h->has_ctg ? h->ctg.host() : nullptr;
    if (more) *more = h->more.host();
    return KMX_OK;
}

kmx_status kmx_secondaries_scripts(const kmx_index* index, const kmx_strand_reads* reads, const kmx_secondaries* secondaries,
                                   const kmx_script_options* options, kmx_scripts** inout)
{
    const std::string who = "kmx_secondaries_scripts: ";
    if (!reads) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "strand reads handle is NULL");
    if (!secondaries) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "secondaries handle is NULL");
    const uint64_t nr2 = 2 * secondaries->nr;
    if (nr2 != reads->nr2) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "the secondaries are not those of these reads: nr2 differs");
    if (nr2 && secondaries->device != reads->device) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "the secondaries and the reads live on different devices");
    // the entries stand in for the loci and their alignments, and every one is selected
    const kmx::LociAccess L{reads->device, reads->stream, nr2, secondaries->n_sec, secondaries->sec_off.as<uint64_t>(), nullptr, nullptr, nullptr};
    const kmx::AlignAccess A{reads->device, reads->stream, nr2, secondaries->n_sec, secondaries->dist.as<uint8_t>(), secondaries->start.as<uint32_t>(),
                             secondaries->end.as<uint32_t>(), nullptr};
    return kmx::scripts_on_arrays("kmx_secondaries_scripts", index, L, A, reads->ranks2.p, reads->roff2.p, reads->letters2, nullptr, options, reads->stream,
                                  inout, true);
}

void kmx_secondaries_free(kmx_secondaries* h) { kmx::free_handle(h); }

} // extern "C"
