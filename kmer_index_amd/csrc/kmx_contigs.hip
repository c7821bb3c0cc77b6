// Contig coordinates of the read-mapping chain (kmx_placements_locate; include/kmx.h, KMX_MAP_CONTIGS).  The index holds a contig
// table (kmx_index_set_contigs, kmx_capi.hip) and kmx_loci_align has stored the contig of every locus (kmx_align.hip), so a placement
// is turned into (contig, position inside it) without any search: a read placed by a locus takes that locus's contig, a rescued mate
// its partner's (the rescue window lies inside the anchor's contig).
//
//   k_locate           a thread per public read: ctg[i], pos[i]; an entry that fails a bound is written as unplaced and counted; the
//                      batch totals go through LDS and one atomic per workgroup
#include <hip/hip_runtime.h>

#include <string>

#include "kmx_approx.h"
#include "kmx_strands.h"
#include "kmx_vote.h"

namespace {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kNone = 0xFFFFFFFFu;
enum { LC_N_LOCATED = 0, LC_N_MISMATCHED, LC_COUNT };

using kmx::Buf;
using Pinned = kmx::PinnedArr;
using kmx::grid_for;

struct LocateIn {
    const uint32_t* locus;         // [nr]: the placements
    const uint8_t* strand;
    const uint32_t* start;
    const uint32_t* lctg;          // [n_loci]: the contig of every locus (the alignments')
    const uint64_t* ctg_off;       // [nc + 1]: the index's table
    uint64_t nr, n_loci, nc;
    uint32_t flags;
};

__global__ __launch_bounds__(kBlock) void k_locate(LocateIn Q, uint32_t* __restrict__ ctg, uint32_t* __restrict__ pos, unsigned long long* __restrict__ ctr)
{
    __shared__ unsigned int s_ctr[LC_COUNT];
    if (threadIdx.x < LC_COUNT) s_ctr[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (i < Q.nr) {
        uint32_t c = kNone, at = 0;
        if (Q.strand[i] != 255) {
            uint32_t l = Q.locus[i];
            if (l == kNone && (Q.flags & KMX_LOCATE_MATES)) {  // a rescued mate: its partner's locus (nr is even: i ^ 1 < nr)
                const uint64_t mate = i ^ 1;
                if (Q.strand[mate] != 255) l = Q.locus[mate];
            }
            bool ok = false;
            if (l < Q.n_loci) {                                // (kNone fails here: n_loci < 2^32)
                c = Q.lctg[l];
                if (c < Q.nc) {
                    const uint64_t b0 = Q.ctg_off[c], b1 = Q.ctg_off[c + 1], s = Q.start[i];
                    if (s >= b0 && s <= b1) {
                        at = uint32_t(s - b0);
                        ok = true;
                    }
                }
            }
            if (!ok) { c = kNone; at = 0; }
            atomicAdd(&s_ctr[ok ? LC_N_LOCATED : LC_N_MISMATCHED], 1u);
        }
        ctg[i] = c;
        pos[i] = at;
    }
    __syncthreads();
    if (threadIdx.x < LC_COUNT && s_ctr[threadIdx.x]) atomicAdd(&ctr[threadIdx.x], (unsigned long long)s_ctr[threadIdx.x]);
}

} // namespace

struct kmx_located {
    int device = 0;
    hipStream_t stream = nullptr;          // the stream of the call that filled the handle (the host view copies on it)
    uint64_t nr = 0, n_located = 0, n_mismatched = 0;
    kmx::ArrOf<uint32_t> ctg, pos;         // the results: one entry per public read
    Buf ctr;
    Pinned h_ctr;
    bool host_valid = false;
    std::vector<kmx::Arr*> results() { return {&ctg, &pos}; }
    std::vector<Buf*> scratch() { return {&ctr}; }
    void release() { kmx::release_arrays(*this); }
    void clear() { nr = n_located = n_mismatched = 0; kmx::clear_arrays(*this); }
};

namespace {

kmx_status locate_run(const kmx::IndexAccess& X, const kmx::AlignAccess& A, const kmx_placements* pl, uint32_t flags, hipStream_t s, kmx_located* h)
{
    const uint64_t nr = pl->nr;
    if (nr == 0) return KMX_OK;
    for (Buf* b : {&h->ctg, &h->pos}) TRY_HIP(b->ensure(nr * 4));
    TRY_HIP(h->ctr.ensure(LC_COUNT * 8));
    unsigned long long* ctr = h->ctr.as<unsigned long long>();
    TRY_HIP(hipMemsetAsync(ctr, 0, LC_COUNT * 8, s));
    // (alignments without a locus have no ctg array: n_loci = 0 then, and no entry passes the first bound)
    const LocateIn Q{pl->locus.as<uint32_t>(), pl->strand.as<uint8_t>(), pl->start.as<uint32_t>(), A.ctg, X.ctg_off, nr, A.ctg ? A.n_loci : 0, X.nc, flags};
    hipLaunchKernelGGL(k_locate, dim3(grid_for(nr, kBlock)), dim3(kBlock), 0, s, Q, h->ctg.as<uint32_t>(), h->pos.as<uint32_t>(), ctr);
    TRY_HIP(hipGetLastError());
    TRY_KMX(kmx::read_back("kmx_placements_locate", s, ctr, h->h_ctr, LC_COUNT * 8));
    h->nr = h->ctg.n = h->pos.n = nr;
    h->n_located = h->h_ctr.as<uint64_t>()[LC_N_LOCATED];
    h->n_mismatched = h->h_ctr.as<uint64_t>()[LC_N_MISMATCHED];
    return KMX_OK;
}

} // namespace

extern "C" {

kmx_status kmx_placements_locate(const kmx_index* index, const kmx_alignments* alignments, const kmx_placements* placements,
                                 const kmx_locate_options* o, void* stream, kmx_located** inout)
{
    const std::string who = "kmx_placements_locate: ";
    if (!index) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "index is NULL");
    if (!alignments) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "alignments handle is NULL");
    if (!placements) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "placements handle is NULL");
    TRY_KMX(kmx::check_call(who, o, inout));
    if (o->flags & ~KMX_LOCATE_MATES) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "unknown flags");
    const kmx::AlignAccess A = kmx::alignments_access(alignments);
    kmx_located* h = *inout;
    auto refuse = kmx::refuser(who, h);
    if ((o->flags & KMX_LOCATE_MATES) && (placements->nr & 1)) return refuse(KMX_ERR_INVALID_ARGUMENT, "KMX_LOCATE_MATES with an odd number of reads: not interleaved mates");
    if (2 * placements->nr != A.nr) return refuse(KMX_ERR_INVALID_ARGUMENT, "the placements are not those of these alignments: 2 nr differs from the alignments' nr");
    if (placements->nr && placements->device != A.device) return refuse(KMX_ERR_INVALID_ARGUMENT, "the alignments and the placements live on different devices");
    kmx::IndexAccess X{};
    kmx_status no_st;
    std::string no_index;
    if (!kmx::index_for(index, A.device, "the alignments", &X, &no_st, &no_index)) return refuse(no_st, no_index);
    if (A.nc != (X.ctg_off ? X.nc : 0) || A.ctg_gen != X.ctg_gen)
        return refuse(KMX_ERR_INVALID_ARGUMENT, "the alignments were made under another contig table of the index (kmx_index_set_contigs was called since): align again");
    if (!X.ctg_off || X.nc == 0) return refuse(KMX_ERR_INVALID_ARGUMENT, "the index has no contig table (kmx_index_set_contigs)");
    kmx::DeviceGuard dg;
    TRY_KMX(kmx::bind_handle(inout, A.device));
    h = *inout;
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : placements->stream;
    return kmx::run_into(h, s, [&] { return locate_run(X, A, placements, o->flags, s, h); });
}

kmx_status kmx_located_counts(const kmx_located* h, uint64_t* nr, uint64_t* n_located, uint64_t* n_mismatched)
{
    if (!h) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_located_counts: located handle is NULL");
    if (nr) *nr = h->nr;
    if (n_located) *n_located = h->n_located;
    if (n_mismatched) *n_mismatched = h->n_mismatched;
    return KMX_OK;
}

kmx_status kmx_located_view_device(const kmx_located* h, const uint32_t** d_ctg, const uint32_t** d_pos)
{
    if (!h) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_located_view_device: located handle is NULL");
    if (d_ctg) *d_ctg = h->ctg.dev();
    if (d_pos) *d_pos = h->pos.dev();
    return KMX_OK;
}

kmx_status kmx_located_view(kmx_located* h, const uint32_t** ctg, const uint32_t** pos)
{
    if (!h) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_located_view: located handle is NULL");
    if (h->nr == 0) {                                          // the empty result: no array
        if (ctg) *ctg = nullptr;
        if (pos) *pos = nullptr;
        return KMX_OK;
    }
    TRY_KMX(kmx::host_view("kmx_located_view", *h));           // 8 bytes per read
    if (ctg) *ctg = h->ctg.host();
    if (pos) *pos = h->pos.host();
    return KMX_OK;
}

void kmx_located_free(kmx_located* h) { kmx::free_handle(h); }

} // extern "C"
