// SAM tags of the read-mapping chain (kmx_scripts_md, kmx_rescues_md, kmx_secondaries_md, kmx_placements_mapq; include/kmx.h, KMX_SAM_TAGS): the MD string
// of every entry of a scripts handle, from its runs and the packed text, and a MAPQ per public read from the placements and the pairs.
// kmx_clips_md and kmx_clips_rescues_md (KMX_SOFT_CLIP) run the same two MD kernels over the runs of a clips handle (kmx_clip.hip), with the
// text letters clipped off either side as a per-entry offset pair; only that path accepts an S run.
//
//   k_md_count         a thread per entry: validates the entry (sel inside its bound, s <= t <= n, only = X I D, the = X D lengths sum
//                      to t - s) and counts the bytes of its MD from the run lengths alone: the digits of every match counter, 2 bytes
//                      per further X, 1 + len per D.  The text is not touched.  n_mismatched through LDS and one atomic per workgroup
//                      (kmx::launch_scan over the counts gives md_off and the total; one read-back sizes md)
//   k_md_write         a thread per entry: the same walk again, now with the text cursor; the letters come from the packed text (2 / 4 /
//                      8 bits per letter, the words as k_script_dp reads them) through the letters table, which arrives by value and is
//                      staged in LDS
//   k_mapq             a thread per public read: the gap rule of kmx.h in int64; n_zero / n_cap through LDS and one atomic per workgroup
// Thread-per-entry is the shape of k_script_walk: an entry has at most 2 dist + 1 runs.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "kmx_approx.h"
#include "kmx_kernels.h"
#include "kmx_runs.h"
#include "kmx_strands.h"
#include "kmx_vote.h"

namespace {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kNoScore = 0xFFFFu;
enum { MD_N_BYTES = 0, MD_N_MISMATCHED, MD_COUNT };
enum { MQ_N_ZERO = 0, MQ_N_CAP, MQ_COUNT };

using kmx::Buf;
using Pinned = kmx::PinnedArr;
using kmx::grid_for;

// the letters table as kernel arguments: 256 entries, of which the first sigma are looked at
struct LetterWords { uint32_t w[64]; };

// what the two MD kernels read: the scripts arrays, the start / end arrays that sel indexes (of the alignments or of the rescue jobs)
// and the packed text
struct MdIn {
    const uint32_t* sel;           // [n_sel]
    const uint64_t* cig_off;       // [n_sel + 1]
    const uint32_t* cigar;         // [n_ops]
    const uint32_t* start;         // [bound]
    const uint32_t* end;
    uint64_t n_sel, n_ops, bound, n;
    const uint64_t* text;          // packed at w bits per letter
    uint32_t w;
    const uint16_t* tl;            // [n_sel]: the text letters clipped off either side (kmx_clips_md: cig_off / cigar / n_ops then are the
    const uint16_t* tr;            // clips', and an S run counts as an I); nullptr for the unclipped scripts
};

__device__ __forceinline__ uint32_t digits_of(uint64_t c)
{
    uint32_t nd = 1;
    while (c >= 10) { c /= 10; ++nd; }
    return nd;
}

// ---- MD --------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_md_count(MdIn M, uint32_t* __restrict__ cnt, unsigned long long* __restrict__ ctr)
{
    __shared__ unsigned int s_bad;
    if (threadIdx.x == 0) s_bad = 0;
    __syncthreads();
    const uint64_t e = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (e < M.n_sel) {
        uint64_t a, b;
        runs_of(M.cig_off, M.n_ops, e, &a, &b);
        uint64_t bytes = 0;
        if (b > a) {                                           // (an entry without runs: an empty MD, not counted)
            const uint32_t l = M.sel[e];
            bool bad = l >= M.bound;
            uint64_t want = 0;
            if (!bad) {
                const uint32_t s = M.start[l], t = M.end[l];
                bad = !(s <= t && t <= M.n);
                want = uint64_t(t) - s;
                if (M.tl && !bad) {                            // the clipped interval [s + tl, t - tr)
                    const uint64_t off = uint64_t(M.tl[e]) + M.tr[e];
                    bad = off > want;
                    want -= off;
                }
            }
            uint64_t c = 0, sum = 0;
            for (uint64_t k = a; k < b && !bad; ++k) {
                const uint32_t v = M.cigar[k], op = run_op(v);
                const uint64_t len = run_len(v);
                if (op == OP_EQ) { c += len; sum += len; }
                else if (op == OP_X) {
                    if (len) { bytes += digits_of(c) + 1 + 2 * (len - 1); c = 0; }
                    sum += len;
                } else if (op == OP_D) { bytes += digits_of(c) + 1 + len; c = 0; sum += len; }
                else if (op != OP_I && !(op == OP_S && M.tl)) bad = true;
            }
            bytes += digits_of(c);
            bad = bad || sum != want || bytes > 0xFFFFFFFFull;  // (2^32 bytes or more: the counts are 32-bit; needs t - s > 2^30)
            if (bad) { bytes = 0; atomicAdd(&s_bad, 1u); }
        }
        cnt[e] = uint32_t(bytes);
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_bad) atomicAdd(&ctr[MD_N_MISMATCHED], (unsigned long long)s_bad);
}

// c in decimal at out[pos ...), no byte at or past `lim`; returns the position behind it
__device__ __forceinline__ uint64_t put_decimal(uint8_t* __restrict__ out, uint64_t pos, uint64_t lim, uint64_t c)
{
    const uint32_t nd = digits_of(c);
    for (uint32_t k = nd; k-- > 0;) {
        if (pos + k < lim) out[pos + k] = uint8_t('0' + c % 10);
        c /= 10;
    }
    return pos + nd;
}

__global__ __launch_bounds__(kBlock) void k_md_write(MdIn M, const uint64_t* __restrict__ md_off, LetterWords letters, uint8_t* __restrict__ md)
{
    __shared__ uint32_t s_letters[64];
    if (threadIdx.x < 64) s_letters[threadIdx.x] = letters.w[threadIdx.x];
    __syncthreads();
    const uint8_t* table = reinterpret_cast<const uint8_t*>(s_letters);
    const uint64_t e = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (e >= M.n_sel) return;
    uint64_t pos = md_off[e];
    const uint64_t lim = md_off[e + 1];
    if (lim <= pos) return;                                    // no runs, or mismatched: k_md_count left 0 bytes
    const uint32_t l = M.sel[e];
    if (l >= M.bound) return;                                  // (cannot happen: k_md_count saw the same arrays)
    uint64_t a, b;
    runs_of(M.cig_off, M.n_ops, e, &a, &b);
    auto letter_at = [&](uint64_t j) -> uint8_t {              // the text letter j through the table; past the text: a '?' nobody sees
        return j < M.n ? table[text_letter(M.text, M.w, j)] : uint8_t('?');
    };
    uint64_t c = 0, j = uint64_t(M.start[l]) + (M.tl ? M.tl[e] : 0);
    for (uint64_t k = a; k < b; ++k) {
        const uint32_t v = M.cigar[k], op = run_op(v);
        const uint64_t len = run_len(v);
        if (op == OP_EQ) { c += len; j += len; }
        else if (op == OP_X) {
            for (uint64_t x = 0; x < len; ++x) {
                pos = put_decimal(md, pos, lim, c);
                if (pos < lim) md[pos] = letter_at(j);
                ++pos;
                c = 0;
                ++j;
            }
        } else if (op == OP_D) {
            pos = put_decimal(md, pos, lim, c);
            if (pos < lim) md[pos] = uint8_t('^');
            ++pos;
            for (uint64_t x = 0; x < len; ++x, ++pos)
                if (pos < lim) md[pos] = letter_at(j + x);
            c = 0;
            j += len;
        }
    }
    put_decimal(md, pos, lim, c);
}

// ---- MAPQ ------------------------------------------------------------------------------------------------------------------------------
struct MapqIn {
    const uint8_t* strand;         // [nr]: the placements
    const uint8_t* dist;
    const uint8_t* second;
    const uint8_t* cls;            // [nr / 2]: the pairs, nullptr for single reads
    const uint16_t* score;
    const uint16_t* second_score;
    uint64_t nr;
    int64_t max_edits, cap, per_edit, pair_bonus;
};

// the gap rule: d the distance, s the runner-up's (none: one past the budget B)
__device__ __forceinline__ int64_t gap_q(const MapqIn& Q, int64_t d, int64_t s, bool none, int64_t B)
{
    const int64_t s1 = none ? B + 1 : s;
    return min(Q.cap, Q.per_edit * max(int64_t(0), s1 - d));
}

__global__ __launch_bounds__(kBlock) void k_mapq(MapqIn Q, uint8_t* __restrict__ mapq, unsigned long long* __restrict__ ctr)
{
    __shared__ unsigned int s_ctr[MQ_COUNT];
    if (threadIdx.x < MQ_COUNT) s_ctr[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (i < Q.nr) {
        const bool placed = Q.strand[i] != 255;
        int64_t q = 0;
        if (placed) {
            const uint32_t sec = Q.second[i];
            q = gap_q(Q, Q.dist[i], sec, sec == KMX_ALIGN_NONE, Q.max_edits);
            if (Q.cls && Q.cls[i >> 1] == KMX_PAIR_CONCORDANT) {
                const uint32_t ss = Q.second_score[i >> 1];
                const int64_t q_pe = gap_q(Q, Q.score[i >> 1], ss, ss == kNoScore, 2 * Q.max_edits);
                q = min(Q.cap, max(q, min(q_pe, q + Q.pair_bonus)));
            }
        }
        mapq[i] = uint8_t(q);
        if (placed && q == 0) atomicAdd(&s_ctr[MQ_N_ZERO], 1u);
        if (q == Q.cap) atomicAdd(&s_ctr[MQ_N_CAP], 1u);
    }
    __syncthreads();
    if (threadIdx.x < MQ_COUNT && s_ctr[threadIdx.x]) atomicAdd(&ctr[threadIdx.x], (unsigned long long)s_ctr[threadIdx.x]);
}

} // namespace

struct kmx_md {
    int device = 0;
    hipStream_t stream = nullptr;          // the stream of the call that filled the handle (the host view copies on it)
    uint64_t n_sel = 0, n_bytes = 0, n_mismatched = 0;
    // results: the offsets per entry and the bytes of the strings
    kmx::ArrOf<uint64_t> md_off{kmx::ARR_OFFSETS};
    kmx::ArrOf<uint8_t> md;
    Buf cnt, bsum, ctr;
    Pinned h_ctr;
    bool host_valid = false;
    std::vector<kmx::Arr*> results() { return {&md_off, &md}; }
    std::vector<Buf*> scratch() { return {&cnt, &bsum, &ctr}; }
    void release() { kmx::release_arrays(*this); }
    void clear() { n_sel = n_bytes = n_mismatched = 0; kmx::clear_arrays(*this); }
    // a call has succeeded: the arrays expose what the counters say
    void expose()
    {
        md_off.n = n_sel + 1;
        md.n = n_bytes;
    }
};

struct kmx_mapq {
    int device = 0;
    hipStream_t stream = nullptr;          // the stream of the call that filled the handle (the host view copies on it)
    uint64_t nr = 0, n_zero = 0, n_cap = 0;
    kmx::ArrOf<uint8_t> mapq;              // the result: one value per public read
    Buf ctr;
    Pinned h_ctr;
    bool host_valid = false;
    std::vector<kmx::Arr*> results() { return {&mapq}; }
    std::vector<Buf*> scratch() { return {&ctr}; }
    void release() { kmx::release_arrays(*this); }
    void clear() { nr = n_zero = n_cap = 0; kmx::clear_arrays(*this); }
};

namespace {

kmx_status md_run(const char* fn, const kmx::IndexAccess& X, const kmx::ScriptsAccess& S, const uint32_t* start, const uint32_t* end, uint64_t bound,
                  const uint8_t* letters, hipStream_t s, kmx_md* h, const kmx::ClipsAccess* K)
{
    const uint64_t ns = S.n_sel;
    TRY_HIP(h->md_off.ensure((ns + 1) * 8));
    if (ns == 0) {                                             // no entry: no launch indexes an empty array
        TRY_HIP(hipMemsetAsync(h->md_off.p, 0, 8, s));
        h->expose();
        return KMX_OK;
    }
    TRY_KMX(kmx::ensure_text(X, s));
    TRY_HIP(h->cnt.ensure(ns * 4 + 16));
    TRY_HIP(h->bsum.ensure(kmx::scan_blocks(ns) * 8 + 16));
    TRY_HIP(h->ctr.ensure(MD_COUNT * 8));
    unsigned long long* ctr = h->ctr.as<unsigned long long>();
    TRY_HIP(hipMemsetAsync(ctr, 0, MD_COUNT * 8, s));
    const MdIn M{S.sel, K ? K->cig_off : S.cig_off, K ? K->cigar : S.cigar, start, end, ns, K ? K->n_ops : S.n_ops, bound, X.n, X.text->d_words,
                 X.text->w, K ? K->tl : nullptr, K ? K->tr : nullptr};
    const dim3 grid(grid_for(ns, kBlock)), block(kBlock);
    hipLaunchKernelGGL(k_md_count, grid, block, 0, s, M, h->cnt.as<uint32_t>(), ctr);
    kmx::launch_scan(s, h->cnt.as<uint32_t>(), ns, h->bsum.as<uint64_t>(), h->md_off.as<uint64_t>(), ctr + MD_N_BYTES);
    TRY_HIP(hipGetLastError());
    TRY_KMX(kmx::read_back(fn, s, ctr, h->h_ctr, MD_COUNT * 8));   // the one read-back: the bytes size md
    const uint64_t n_bytes = h->h_ctr.as<uint64_t>()[MD_N_BYTES];
    if (n_bytes) {
        TRY_HIP(h->md.ensure(n_bytes));
        LetterWords lw;
        std::memset(lw.w, 0, sizeof lw.w);
        std::memcpy(lw.w, letters, std::min<uint32_t>(X.sigma, 256));
        hipLaunchKernelGGL(k_md_write, grid, block, 0, s, M, h->md_off.as<uint64_t>(), lw, h->md.as<uint8_t>());
        TRY_HIP(hipGetLastError());
    }
    h->n_sel = ns;
    h->n_bytes = n_bytes;
    h->n_mismatched = h->h_ctr.as<uint64_t>()[MD_N_MISMATCHED];
    h->expose();
    return KMX_OK;
}

// the refusals that need no handle: NULL arguments, the options, the letters table (sigma is the index's: a host field)
kmx_status md_front(const std::string& who, const kmx_index* index, const void* scripts, const void* source, const char* source_name,
                    const uint8_t* letters, const kmx_md_options* o, kmx_md** inout)
{
    TRY_KMX(kmx::check_call(who, o, inout));
    if (o->flags != 0) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "flags must be 0");
    if (!letters) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "NULL letters table");
    if (!index) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "index is NULL");
    if (!scripts) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "scripts handle is NULL");
    if (!source) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + source_name + " handle is NULL");
    const uint32_t sigma = kmx::index_access(index).sigma;
    for (uint32_t c = 0; c < sigma && c < 256; ++c)
        if (letters[c] == 0 || letters[c] == '^' || (letters[c] >= '0' && letters[c] <= '9'))
            return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "letters[" + std::to_string(c) + "] is 0, a digit or '^': no letter of an MD string");
    return KMX_OK;
}

// the MD strings of the scripts S over the start / end arrays (of `bound` entries, on `device`) that their sel indexes; K: the clips
// of S, whose runs and offsets then stand in for the scripts' own
kmx_status md_on_arrays(const char* fn, const kmx_index* index, const kmx::ScriptsAccess& S, int device, const uint32_t* start, const uint32_t* end,
                        uint64_t bound, const uint8_t* letters, hipStream_t stream, kmx_md** inout, const kmx::ClipsAccess* K = nullptr)
{
    const std::string who = std::string(fn) + ": ";
    kmx_md* h = *inout;
    auto refuse = kmx::refuser(who, h);
    if (S.flags & KMX_SCRIPT_M) return refuse(KMX_ERR_INVALID_ARGUMENT, "the scripts were made with KMX_SCRIPT_M: an MD needs '=' and 'X' apart");
    if (S.n_sel && S.device != device) return refuse(KMX_ERR_INVALID_ARGUMENT, "the handles live on different devices");
    if (K && K->n_sel != S.n_sel) return refuse(KMX_ERR_INVALID_ARGUMENT, "the clips are not those of these scripts: n_sel differs");
    if (K && K->n_sel && K->device != S.device) return refuse(KMX_ERR_INVALID_ARGUMENT, "the clips and the scripts live on different devices");
    kmx::IndexAccess X{};
    kmx_status no_st;
    std::string no_index;
    if (!kmx::index_for(index, S.device, "the scripts", &X, &no_st, &no_index)) return refuse(no_st, no_index);
    kmx::DeviceGuard dg;
    TRY_KMX(kmx::bind_handle(inout, S.device));
    h = *inout;
    hipStream_t s = stream ? stream : S.stream;
    return kmx::run_into(h, s, [&] { return md_run(fn, X, S, start, end, bound, letters, s, h, K); });
}

kmx_status mapq_run(const kmx_placements* pl, const kmx_pairs* pr, const kmx_mapq_options& o, hipStream_t s, kmx_mapq* h)
{
    const uint64_t nr = pl->nr;
    if (nr == 0) return KMX_OK;
    TRY_HIP(h->mapq.ensure(nr));
    TRY_HIP(h->ctr.ensure(MQ_COUNT * 8));
    unsigned long long* ctr = h->ctr.as<unsigned long long>();
    TRY_HIP(hipMemsetAsync(ctr, 0, MQ_COUNT * 8, s));
    const MapqIn Q{pl->strand.as<uint8_t>(), pl->dist.as<uint8_t>(), pl->second.as<uint8_t>(), pr ? pr->cls.as<uint8_t>() : nullptr,
                   pr ? pr->score.as<uint16_t>() : nullptr, pr ? pr->second_score.as<uint16_t>() : nullptr, nr, int64_t(o.max_edits), int64_t(o.cap),
                   int64_t(o.per_edit), int64_t(o.pair_bonus)};
    hipLaunchKernelGGL(k_mapq, dim3(grid_for(nr, kBlock)), dim3(kBlock), 0, s, Q, h->mapq.as<uint8_t>(), ctr);
    TRY_HIP(hipGetLastError());
    TRY_KMX(kmx::read_back("kmx_placements_mapq", s, ctr, h->h_ctr, MQ_COUNT * 8));
    h->nr = h->mapq.n = nr;
    h->n_zero = h->h_ctr.as<uint64_t>()[MQ_N_ZERO];
    h->n_cap = h->h_ctr.as<uint64_t>()[MQ_N_CAP];
    return KMX_OK;
}

} // namespace

extern "C" {

kmx_status kmx_scripts_md(const kmx_index* index, const kmx_scripts* scripts, const kmx_alignments* alignments, const uint8_t* letters,
                          const kmx_md_options* options, void* stream, kmx_md** inout)
{
    TRY_KMX(md_front("kmx_scripts_md: ", index, scripts, alignments, "alignments", letters, options, inout));
    const kmx::AlignAccess A = kmx::alignments_access(alignments);
    return md_on_arrays("kmx_scripts_md", index, kmx::scripts_access(scripts), A.device, A.start, A.end, A.n_loci, letters,
                        static_cast<hipStream_t>(stream), inout);
}

kmx_status kmx_rescues_md(const kmx_index* index, const kmx_scripts* scripts, const kmx_rescues* rescues, const uint8_t* letters,
                          const kmx_md_options* options, void* stream, kmx_md** inout)
{
    TRY_KMX(md_front("kmx_rescues_md: ", index, scripts, rescues, "rescues", letters, options, inout));
    const kmx::JobsAccess J = kmx::rescues_access(rescues);
    return md_on_arrays("kmx_rescues_md", index, kmx::scripts_access(scripts), J.device, J.start, J.end, J.n_jobs, letters,
                        static_cast<hipStream_t>(stream), inout);
}

kmx_status kmx_secondaries_md(const kmx_index* index, const kmx_scripts* scripts, const kmx_secondaries* secondaries, const uint8_t* letters,
                              const kmx_md_options* options, void* stream, kmx_md** inout)
{
    TRY_KMX(md_front("kmx_secondaries_md: ", index, scripts, secondaries, "secondaries", letters, options, inout));
    const kmx::JobsAccess J = kmx::secondaries_access(secondaries);
    return md_on_arrays("kmx_secondaries_md", index, kmx::scripts_access(scripts), J.device, J.start, J.end, J.n_jobs, letters,
                        static_cast<hipStream_t>(stream), inout);
}

kmx_status kmx_clips_md(const kmx_index* index, const kmx_scripts* scripts, const kmx_clips* clips, const kmx_alignments* alignments,
                        const uint8_t* letters, const kmx_md_options* options, void* stream, kmx_md** inout)
{
    if (!clips) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_clips_md: clips handle is NULL");
    TRY_KMX(md_front("kmx_clips_md: ", index, scripts, alignments, "alignments", letters, options, inout));
    const kmx::AlignAccess A = kmx::alignments_access(alignments);
    const kmx::ClipsAccess K = kmx::clips_access(clips);
    return md_on_arrays("kmx_clips_md", index, kmx::scripts_access(scripts), A.device, A.start, A.end, A.n_loci, letters,
                        static_cast<hipStream_t>(stream), inout, &K);
}

kmx_status kmx_clips_rescues_md(const kmx_index* index, const kmx_scripts* scripts, const kmx_clips* clips, const kmx_rescues* rescues,
                                const uint8_t* letters, const kmx_md_options* options, void* stream, kmx_md** inout)
{
    if (!clips) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_clips_rescues_md: clips handle is NULL");
    TRY_KMX(md_front("kmx_clips_rescues_md: ", index, scripts, rescues, "rescues", letters, options, inout));
    const kmx::JobsAccess J = kmx::rescues_access(rescues);
    const kmx::ClipsAccess K = kmx::clips_access(clips);
    return md_on_arrays("kmx_clips_rescues_md", index, kmx::scripts_access(scripts), J.device, J.start, J.end, J.n_jobs, letters,
                        static_cast<hipStream_t>(stream), inout, &K);
}

kmx_status kmx_md_counts(const kmx_md* h, uint64_t* n_sel, uint64_t* n_bytes, uint64_t* n_mismatched)
{
    if (!h) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_md_counts: md handle is NULL");
    if (n_sel) *n_sel = h->n_sel;
    if (n_bytes) *n_bytes = h->n_bytes;
    if (n_mismatched) *n_mismatched = h->n_mismatched;
    return KMX_OK;
}

kmx_status kmx_md_view_device(const kmx_md* h, const uint64_t** d_md_off, const uint8_t** d_md)
{
    if (!h) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_md_view_device: md handle is NULL");
    if (d_md_off) *d_md_off = h->md_off.dev();
    if (d_md) *d_md = h->md.dev();
    return KMX_OK;
}

kmx_status kmx_md_view(kmx_md* h, const uint64_t** md_off, const uint8_t** md)
{
    if (!h) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_md_view: md handle is NULL");
    TRY_KMX(kmx::host_view("kmx_md_view", *h));                // 8 bytes per entry and its string
    if (md_off) *md_off = h->md_off.host();
    if (md) *md = h->md.host();
    return KMX_OK;
}

void kmx_md_free(kmx_md* h) { kmx::free_handle(h); }

kmx_status kmx_placements_mapq(const kmx_placements* placements, const kmx_pairs* pairs, const kmx_mapq_options* o, void* stream, kmx_mapq** inout)
{
    const std::string who = "kmx_placements_mapq: ";
    TRY_KMX(kmx::check_call(who, o, inout));
    if (o->flags != 0) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "flags must be 0");
    if (o->max_edits > KMX_ALIGN_MAX_EDITS) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "max_edits > KMX_ALIGN_MAX_EDITS");
    if (o->cap > 254) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "cap > 254 (255 is SAM's \"unavailable\")");
    if (!placements) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "placements handle is NULL");
    kmx_mapq* h = *inout;
    auto refuse = kmx::refuser(who, h);
    if (pairs && 2 * pairs->np != placements->nr) return refuse(KMX_ERR_INVALID_ARGUMENT, "the pairs are not those of these placements: 2 np differs from nr");
    if (pairs && placements->nr && pairs->device != placements->device) return refuse(KMX_ERR_INVALID_ARGUMENT, "the placements and the pairs live on different devices");
    kmx::DeviceGuard dg;
    TRY_KMX(kmx::bind_handle(inout, placements->device));
    h = *inout;
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : placements->stream;
    return kmx::run_into(h, s, [&] { return mapq_run(placements, pairs, *o, s, h); });
}

kmx_status kmx_mapq_counts(const kmx_mapq* h, uint64_t* nr, uint64_t* n_zero, uint64_t* n_cap)
{
    if (!h) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_mapq_counts: mapq handle is NULL");
    if (nr) *nr = h->nr;
    if (n_zero) *n_zero = h->n_zero;
    if (n_cap) *n_cap = h->n_cap;
    return KMX_OK;
}

kmx_status kmx_mapq_view_device(const kmx_mapq* h, const uint8_t** d_mapq)
{
    if (!h) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_mapq_view_device: mapq handle is NULL");
    if (d_mapq) *d_mapq = h->mapq.dev();
    return KMX_OK;
}

kmx_status kmx_mapq_view(kmx_mapq* h, const uint8_t** mapq)
{
    if (!h) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_mapq_view: mapq handle is NULL");
    if (h->nr == 0) {                                          // the empty result: no array
        if (mapq) *mapq = nullptr;
        return KMX_OK;
    }
    TRY_KMX(kmx::host_view("kmx_mapq_view", *h));              // 1 byte per read
    if (mapq) *mapq = h->mapq.host();
    return KMX_OK;
}

void kmx_mapq_free(kmx_mapq* h) { kmx::free_handle(h); }

} // extern "C"
