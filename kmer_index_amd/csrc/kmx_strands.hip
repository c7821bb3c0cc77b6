// Both strands of the read-mapping chain (kmx_reads_strands, kmx_alignments_fold_strands, kmx_placements_scripts; include/kmx.h).
// The reverse complement of a read is just another read: the doubled batch goes through kmx_search_windows_device,
// kmx_windows_vote, kmx_loci_align_device and kmx_alignments_scripts_device as they are, and the two strands of every read are
// folded into one placement on the device.
//
//   k_strand_reads     a wave per public read: lane j copies letter j to internal read 2i and the complement of letter m - 1 - j
//                      to internal read 2i + 1, 64 neighbouring bytes per load and per store; lane 0 writes the two offsets
//   k_strand_fold      a wave per public read: the winner from best[2i] / best[2i + 1], then the lanes stride over the loci of both
//                      strands and min-reduce the distances of those that lie elsewhere; lane 0 writes; the batch totals go
//                      through LDS and one atomic per workgroup
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "kmx_approx.h"
#include "kmx_fold_core.h"
#include "kmx_kernels.h"
#include "kmx_strands.h"
#include "kmx_vote.h"

namespace {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kWave = 64;
constexpr uint32_t kNoBest = 0xFFFFFFFFu;
constexpr uint64_t kMaxReads = uint64_t(1) << 30;
constexpr uint64_t kMaxLetters = uint64_t(1) << 62;
constexpr int CTR_COUNT = kmx::PL_COUNT;

using kmx::Buf;
using Pinned = kmx::PinnedArr;
using kmx::grid_for;

// the complement table as kernel arguments: 256 entries, the identity outside the alphabet
struct CompWords { uint32_t w[64]; };

// ---- the doubled batch ---------------------------------------------------------------------------------------------------------------
// total = roff[nr]: a read whose offsets decrease or leave [0, total] is written as an empty pair (device form: foreign offsets), so
// every store lands inside ranks2[2 * total]
__global__ __launch_bounds__(kBlock) void k_strand_reads(const uint8_t* __restrict__ ranks, const uint64_t* __restrict__ roff, uint64_t nr,
                                                         uint64_t total, CompWords comp, uint8_t* __restrict__ ranks2, uint64_t* __restrict__ roff2)
{
    __shared__ uint32_t s_comp[64];
    if (threadIdx.x < 64) s_comp[threadIdx.x] = comp.w[threadIdx.x];
    __syncthreads();
    const uint8_t* table = reinterpret_cast<const uint8_t*>(s_comp);
    const uint32_t lane = threadIdx.x % kWave;
    const uint64_t i = uint64_t(blockIdx.x) * (kBlock / kWave) + threadIdx.x / kWave;
    if (i >= nr) return;
    const uint64_t a = min(roff[i], total), b = roff[i + 1];
    const uint64_t m = b >= a && b <= total ? b - a : 0;
    const uint8_t* q = ranks + a;
    uint8_t* fw = ranks2 + 2 * a;
    uint8_t* rv = fw + m;
    for (uint64_t j = lane; j < m; j += kWave) {
        fw[j] = q[j];
        rv[j] = table[q[m - 1 - j]];
    }
    if (lane == 0) {
        roff2[2 * i] = 2 * a;
        roff2[2 * i + 1] = 2 * a + m;
        if (i + 1 == nr) roff2[2 * nr] = 2 * total;
    }
}

// ---- the fold ------------------------------------------------------------------------------------------------------------------------
struct FoldIn {
    const uint64_t* locus_off;     // [nr2 + 1]
    const uint8_t* dist;           // [n_loci]
    const uint32_t* start;
    const uint32_t* end;
    const uint32_t* best;          // [nr2]
    uint64_t nr, n_loci;           // public reads
};

struct FoldOut {
    uint32_t* locus;               // [nr]
    uint8_t* strand;
    uint8_t* dist;
    uint32_t* start;
    uint32_t* end;
    uint8_t* second;
    uint32_t* best2;               // [nr2]
    unsigned long long* ctr;
};

__global__ __launch_bounds__(kBlock) void k_strand_fold(FoldIn F, FoldOut O)
{
    __shared__ unsigned int s_ctr[CTR_COUNT];
    if (threadIdx.x < CTR_COUNT) s_ctr[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x % kWave;
    const uint64_t i = uint64_t(blockIdx.x) * (kBlock / kWave) + threadIdx.x / kWave;
    if (i < F.nr) {
        uint64_t a, b, c;
        strand_ranges(F.locus_off, F.n_loci, 2 * i, &a, &b, &c);
        // step 1: the winner; step 2: the least distance of an aligned locus elsewhere
        const Winner W = strand_winner(F.dist, F.best, 2 * i, a, b, c);
        uint32_t ws = 0, we = 0, second = KMX_ALIGN_NONE;
        if (W.placed) {
            ws = F.start[W.locus];
            we = F.end[W.locus];
            second = second_elsewhere(F.dist, F.start, F.end, a, b, c, lane, W.locus, W.strand, ws, we);
        }
        if (lane == 0) {
            O.locus[i] = W.placed ? uint32_t(W.locus) : kNoBest;
            O.strand[i] = W.placed ? uint8_t(W.strand) : uint8_t(255);
            O.dist[i] = uint8_t(W.dist);
            O.start[i] = ws;
            O.end[i] = we;
            O.second[i] = uint8_t(second);
            O.best2[2 * i] = W.placed && W.strand == 0 ? uint32_t(W.locus - a) : kNoBest;
            O.best2[2 * i + 1] = W.placed && W.strand == 1 ? uint32_t(W.locus - b) : kNoBest;
            count_placement(s_ctr, W.placed, W.strand, second, W.dist);
        }
    }
    __syncthreads();
    if (threadIdx.x < CTR_COUNT && s_ctr[threadIdx.x]) atomicAdd(&O.ctr[threadIdx.x], (unsigned long long)s_ctr[threadIdx.x]);
}

} // namespace

kmx::PlacementsAccess kmx::placements_access(const kmx_placements* p)
{
    return PlacementsAccess{p->device, p->stream, 2 * p->nr, p->best2.as<uint32_t>(), p->nr, p->locus.as<uint32_t>(), p->strand.as<uint8_t>(),
                            p->dist.as<uint8_t>(), p->start.as<uint32_t>(), p->end.as<uint32_t>()};
}

namespace {

// host == true: ranks / roff are host arrays that go up on the handle's own stream; else device arrays and the caller's stream
kmx_status strands_call(const char* fn, const kmx_index* index, const void* ranks, const void* roff, uint64_t nr, const uint8_t* complement,
                        bool host, hipStream_t stream, kmx_strand_reads** inout)
{
    const std::string who = std::string(fn) + ": ";
    if (!index) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "index is NULL");
    if (!inout) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "inout is NULL");
    kmx_strand_reads* h = *inout;
    auto refuse = kmx::refuser(who, h);
    if (!complement) return refuse(KMX_ERR_INVALID_ARGUMENT, "NULL complement table");
    kmx::IndexAccess X = kmx::index_access(index);
    uint8_t comp[256];
    if (kmx::check_complement(who, complement, X.sigma, comp) != KMX_OK) { if (h) h->clear(); return KMX_ERR_INVALID_ARGUMENT; }
    if (nr && !roff) return refuse(KMX_ERR_INVALID_ARGUMENT, "roff is NULL");
    if (nr >= kMaxReads) return refuse(KMX_ERR_TOO_LARGE, "2^30 or more reads: split the batch");
    uint64_t total = 0;
    if (host) {
        const char* why = kmx::check_host_reads(ranks, static_cast<const uint64_t*>(roff), nr, &total);
        if (why) return refuse(KMX_ERR_INVALID_ARGUMENT, why);
        if (total > kMaxLetters) return refuse(KMX_ERR_TOO_LARGE, "more than 2^62 letters: split the batch");
    } else if (nr) {                                           // the replica on the device that owns the reads
        hipPointerAttribute_t attr{};
        if (hipPointerGetAttributes(&attr, ranks ? ranks : roff) != hipSuccess) {
            (void)hipGetLastError();
            return refuse(KMX_ERR_INVALID_ARGUMENT, "d_ranks is not a device pointer");
        }
        if (!kmx::index_access_on(index, attr.device, &X)) return refuse(KMX_ERR_INVALID_ARGUMENT, "the reads live on a device that holds no replica of this index");
    }
    kmx::DeviceGuard dg;
    TRY_KMX(kmx::bind_handle(inout, X.device));
    h = *inout;
    h->clear();
    auto run = [&]() -> kmx_status {
        (void)hipGetLastError();
        if (host && !h->own) TRY_HIP(hipStreamCreateWithFlags(&h->own, hipStreamNonBlocking));
        hipStream_t s = host ? h->own : stream;
        h->stream = s;
        TRY_HIP(h->roff2.ensure((2 * nr + 1) * 8));
        if (nr == 0) {
            TRY_HIP(h->ranks2.ensure(1));
            TRY_HIP(hipMemsetAsync(h->roff2.p, 0, 8, s));
            return KMX_OK;
        }
        const uint8_t* d_ranks = static_cast<const uint8_t*>(ranks);
        const uint64_t* d_roff = static_cast<const uint64_t*>(roff);
        if (host) {
            TRY_KMX(kmx::upload_reads(ranks, roff, nr, total, h->raw, h->roff, s));
            d_ranks = h->raw.as<uint8_t>();
            d_roff = h->roff.as<uint64_t>();
        } else {                                               // one 8-byte read-back: the letters of the batch
            TRY_KMX(kmx::read_back(fn, s, d_roff + nr, h->h_total, 8));
            total = h->h_total.as<uint64_t>()[0];
            if (total > kMaxLetters) return kmx::set_error(KMX_ERR_TOO_LARGE, who + "more than 2^62 letters: split the batch");
        }
        TRY_HIP(h->ranks2.ensure(std::max<uint64_t>(2 * total, 1)));
        CompWords cw;
        std::memcpy(cw.w, comp, sizeof cw.w);
        hipLaunchKernelGGL(k_strand_reads, dim3(grid_for(nr, kBlock / kWave)), dim3(kBlock), 0, s, d_ranks, d_roff, nr, total, cw, h->ranks2.as<uint8_t>(),
                           h->roff2.as<uint64_t>());
        TRY_HIP(hipGetLastError());
        h->letters2 = 2 * total;
        return KMX_OK;
    };
    const kmx_status st = run();
    if ((host || st != KMX_OK) && h->stream) (void)hipStreamSynchronize(h->stream);   // the caller's arrays are free again
    if (st == KMX_OK) h->nr2 = 2 * nr;
    else h->clear();
    return st;
}

kmx_status fold_run(const kmx::LociAccess& L, const kmx::AlignAccess& A, hipStream_t s, kmx_placements* p)
{
    const uint64_t nr = L.nr / 2;
    if (nr == 0) return KMX_OK;
    TRY_HIP(p->room(nr));
    TRY_HIP(p->ctr.ensure(CTR_COUNT * 8));
    unsigned long long* ctr = p->ctr.as<unsigned long long>();
    TRY_HIP(hipMemsetAsync(ctr, 0, CTR_COUNT * 8, s));
    const FoldIn F{L.locus_off, A.dist, A.start, A.end, A.best, nr, L.n_loci};
    const FoldOut O{p->locus.as<uint32_t>(), p->strand.as<uint8_t>(), p->dist.as<uint8_t>(), p->start.as<uint32_t>(), p->end.as<uint32_t>(),
                    p->second.as<uint8_t>(), p->best2.as<uint32_t>(), ctr};
    hipLaunchKernelGGL(k_strand_fold, dim3(grid_for(nr, kBlock / kWave)), dim3(kBlock), 0, s, F, O);
    TRY_HIP(hipGetLastError());
    TRY_KMX(kmx::read_back("kmx_alignments_fold_strands", s, ctr, p->h_ctr, CTR_COUNT * 8));
    p->expose(nr);
    p->counts_from(p->h_ctr.as<uint64_t>());
    return KMX_OK;
}

} // namespace

extern "C" {

kmx_status kmx_reads_strands(const kmx_index* index, const uint8_t* ranks, const uint64_t* roff, uint64_t nr, const uint8_t* complement,
                             kmx_strand_reads** inout)
{
    return strands_call("kmx_reads_strands", index, ranks, roff, nr, complement, true, nullptr, inout);
}

kmx_status kmx_reads_strands_device(const kmx_index* index, const void* d_ranks, const void* d_roff, uint64_t nr, const uint8_t* complement,
                                    void* stream, kmx_strand_reads** inout)
{
    return strands_call("kmx_reads_strands_device", index, d_ranks, d_roff, nr, complement, false, static_cast<hipStream_t>(stream), inout);
}

kmx_status kmx_strand_reads_view_device(const kmx_strand_reads* h, const uint8_t** d_ranks2, const uint64_t** d_roff2, uint64_t* nr2, void** stream)
{
    if (!h) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_strand_reads_view_device: strand reads handle is NULL");
    if (d_ranks2) *d_ranks2 = h->ranks2.as<uint8_t>();
    if (d_roff2) *d_roff2 = h->roff2.as<uint64_t>();
    if (nr2) *nr2 = h->nr2;
    if (stream) *stream = h->stream;
    return KMX_OK;
}

void kmx_strand_reads_free(kmx_strand_reads* h) { kmx::free_handle(h); }

kmx_status kmx_alignments_fold_strands(const kmx_loci* loci, const kmx_alignments* alignments, const kmx_fold_options* o, void* stream,
                                       kmx_placements** inout)
{
    const std::string who = "kmx_alignments_fold_strands: ";
    if (!loci) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "loci handle is NULL");
    if (!alignments) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "alignments handle is NULL");
    TRY_KMX(kmx::check_call(who, o, inout));
    if (o->flags != 0) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "flags must be 0");
    const kmx::LociAccess L = kmx::loci_access(loci);
    const kmx::AlignAccess A = kmx::alignments_access(alignments);
    kmx_placements* p = *inout;
    auto refuse = kmx::refuser(who, p);
    if (L.nr != A.nr) return refuse(KMX_ERR_INVALID_ARGUMENT, "the alignments handle's nr differs from the loci handle's");
    if (L.nr & 1) return refuse(KMX_ERR_INVALID_ARGUMENT, "an odd number of reads: not the loci of a doubled batch");
    if (A.n_loci != L.n_loci) return refuse(KMX_ERR_INVALID_ARGUMENT, "the alignments handle's n_loci differs from the loci handle's");
    if (A.device != L.device) return refuse(KMX_ERR_INVALID_ARGUMENT, "the loci and the alignments live on different devices");
    kmx::DeviceGuard dg;
    TRY_KMX(kmx::bind_handle(inout, L.device));
    p = *inout;
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : A.stream;
    return kmx::run_into(p, s, [&] { return fold_run(L, A, s, p); });
}

kmx_status kmx_placements_counts(const kmx_placements* p, uint64_t* nr, uint64_t* n_placed, uint64_t* n_reverse, uint64_t* n_ambiguous)
{
    if (!p) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_placements_counts: placements handle is NULL");
    if (nr) *nr = p->nr;
    if (n_placed) *n_placed = p->n_placed;
    if (n_reverse) *n_reverse = p->n_reverse;
    if (n_ambiguous) *n_ambiguous = p->n_ambiguous;
    return KMX_OK;
}

kmx_status kmx_placements_view_device(const kmx_placements* p, const uint32_t** d_locus, const uint8_t** d_strand, const uint8_t** d_dist,
                                      const uint32_t** d_start, const uint32_t** d_end, const uint8_t** d_second, const uint32_t** d_best2)
{
    if (!p) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_placements_view_device: placements handle is NULL");
    if (d_locus) *d_locus = p->locus.dev();
    if (d_strand) *d_strand = p->strand.dev();
    if (d_dist) *d_dist = p->dist.dev();
    if (d_start) *d_start = p->start.dev();
    if (d_end) *d_end = p->end.dev();
    if (d_second) *d_second = p->second.dev();
    if (d_best2) *d_best2 = p->best2.dev();
    return KMX_OK;
}

kmx_status kmx_placements_view(kmx_placements* p, const uint32_t** locus, const uint8_t** strand, const uint8_t** dist, const uint32_t** start,
                               const uint32_t** end, const uint8_t** second, const uint32_t** best2)
{
    if (!p) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_placements_view: placements handle is NULL");
    const bool want_best2 = best2 && !p->host_best2_valid;     // 15 bytes per read; best2 (a pair per read) only when asked for
    TRY_KMX(kmx::host_view("kmx_placements_view", *p, want_best2 ? &p->best2 : nullptr));
    if (best2) p->host_best2_valid = true;
    if (locus) *locus = p->locus.host();
    if (strand) *strand = p->strand.host();
    if (dist) *dist = p->dist.host();
    if (start) *start = p->start.host();
    if (end) *end = p->end.host();
    if (second) *second = p->second.host();
    if (best2) *best2 = p->best2.host();
    return KMX_OK;
}

void kmx_placements_free(kmx_placements* p) { kmx::free_handle(p); }

kmx_status kmx_placements_scripts(const kmx_index* index, const kmx_strand_reads* reads, const kmx_loci* loci, const kmx_alignments* alignments,
                                  const kmx_placements* placements, const kmx_script_options* options, kmx_scripts** inout)
{
    const std::string who = "kmx_placements_scripts: ";
    if (!reads) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "strand reads handle is NULL");
    if (!placements) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "placements handle is NULL");
    const kmx::PlacementsAccess P = kmx::placements_access(placements);
    return kmx::scripts_with_best("kmx_placements_scripts", index, loci, alignments, reads->ranks2.p, reads->roff2.p, reads->nr2, reads->letters2, options,
                                  reads->stream, P, inout);
}

} // extern "C"
