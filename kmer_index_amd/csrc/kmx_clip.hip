// Soft clipping of the read-mapping chain (kmx_scripts_clip; include/kmx.h, KMX_SOFT_CLIP): every entry of a scripts handle trimmed to
// the best-scoring part of its runs under an affine scoring, with the score, the letters clipped off either side and the new runs
// ('S' at the clipped ends).  Post-alignment trimming of the edit-optimal script, not a realignment: only the runs are read.
//
//   k_clip_pick        a thread per entry: one pass over the runs with the prefix sum W, the running minimum of W[i] + p [i > 0] over
//                      the left cuts seen so far and the best (V, i, j) under the tie rule (greatest V, smallest i, largest j); a
//                      second pass over the same runs sums the letters in front of i, from j on and the edits between; writes the
//                      seven per-entry values, the cuts and the run count.  n_clipped / n_low through LDS and one atomic per workgroup
//                      (kmx::launch_scan over the run counts gives cig_off and n_ops)
//   k_clip_write       a thread per entry: sl S, the kept runs, sr S, inside the entry's range of the output
// Thread-per-entry is the shape of k_md_count / k_md_write: an entry has at most 2 dist + 1 runs.  The output holds n_ops + 2 n_sel
// runs, an entry's bound, so nothing is read back in front of the write; the one read-back at the end fetches the counts.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "kmx_kernels.h"
#include "kmx_vote.h"

namespace {

constexpr uint32_t kBlock = 256;
constexpr uint64_t kMaxRuns = 0x7FFFFFFFull;                   // the runs of one entry that are looked at (its count, + 2, is 32-bit)
enum { OP_I = 1, OP_D = 2, OP_S = 4, OP_EQ = 7, OP_X = 8 };
enum { CL_N_OPS = 0, CL_N_CLIPPED, CL_N_LOW, CL_COUNT };

using kmx::Buf;
using Pinned = kmx::PinnedArr;
using kmx::grid_for;

struct ClipIn {
    const uint64_t* cig_off;       // [n_sel + 1]: the scripts'
    const uint32_t* cigar;         // [n_ops]
    uint64_t n_sel, n_ops;
    int64_t a, b, o, x, p, min_score;
};

struct ClipOut {
    int32_t* score;                // [n_sel]
    uint16_t* sl;
    uint16_t* sr;
    uint16_t* tl;
    uint16_t* tr;
    uint16_t* nm;
    uint8_t* cflags;
    uint32_t* cut_i;               // scratch: the cuts, for k_clip_write
    uint32_t* cut_j;
    uint32_t* cnt;                 // the runs of the clipped entry
};

// the runs of entry e, inside cigar[n_ops] whatever the offsets hold
__device__ __forceinline__ void runs_of(const ClipIn& C, uint64_t e, uint64_t* a, uint64_t* b)
{
    *a = min(C.cig_off[e], C.n_ops);
    *b = min(min(max(C.cig_off[e + 1], *a), C.n_ops), *a + kMaxRuns);
}

__device__ __forceinline__ uint16_t sat16(uint64_t v) { return uint16_t(min(v, uint64_t(0xFFFF))); }

__global__ __launch_bounds__(kBlock) void k_clip_pick(ClipIn C, ClipOut O, unsigned long long* __restrict__ ctr)
{
    __shared__ unsigned int s_ctr[2];                          // clipped, low
    if (threadIdx.x < 2) s_ctr[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t e = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (e < C.n_sel) {
        uint64_t a, b;
        runs_of(C, e, &a, &b);
        const uint32_t R = uint32_t(b - a);
        // the best (V, i, j): (0, R) is a candidate for every R, the loop meets it at its last run
        int64_t W = 0, min_left = 0, best_v = 0;
        uint32_t min_i = 0, bi = 0, bj = R;
        bool bad = false, have = R == 0;
        for (uint32_t k = 0; k < R; ++k) {
            const uint32_t v = C.cigar[a + k], op = v & 15u;
            const int64_t len = int64_t(v >> 4);
            if (op == OP_EQ) {
                if (k > 0 && W + C.p < min_left) { min_left = W + C.p; min_i = k; }   // a left cut; among equals the smallest stays
                W += len * C.a;
            } else if (op == OP_X) W -= len * C.b;
            else if (op == OP_I || op == OP_D) W -= C.o + len * C.x;
            else bad = true;
            if (op == OP_EQ || k + 1 == R) {                   // a right cut behind run k
                const int64_t val = W - (k + 1 < R ? C.p : 0) - min_left;
                if (!have || val > best_v || (val == best_v && min_i <= bi)) {        // (equal i: this j is the larger one)
                    have = true;
                    best_v = val;
                    bi = min_i;
                    bj = k + 1;
                }
            }
        }
        const bool low = bad || best_v < C.min_score;
        if (low) { bi = 0; bj = R; best_v = bad ? 0 : W; }
        uint64_t sl = 0, sr = 0, tl = 0, tr = 0, nm = 0;
        for (uint32_t k = 0; k < R && !bad; ++k) {
            const uint32_t v = C.cigar[a + k], op = v & 15u;
            const uint64_t len = v >> 4;
            const uint64_t rd = op == OP_D ? 0 : len, tx = op == OP_I ? 0 : len;
            if (k < bi) { sl += rd; tl += tx; }
            else if (k >= bj) { sr += rd; tr += tx; }
            else if (op != OP_EQ) nm += len;
        }
        O.score[e] = int32_t(max(int64_t(INT32_MIN), min(int64_t(INT32_MAX), best_v)));
        O.sl[e] = sat16(sl);
        O.sr[e] = sat16(sr);
        O.tl[e] = sat16(tl);
        O.tr[e] = sat16(tr);
        O.nm[e] = sat16(nm);
        O.cflags[e] = low ? uint8_t(KMX_CLIP_LOW) : uint8_t(0);
        O.cut_i[e] = bi;
        O.cut_j[e] = bj;
        O.cnt[e] = (bj - bi) + (sl ? 1u : 0u) + (sr ? 1u : 0u);
        if (sl + sr) atomicAdd(&s_ctr[0], 1u);
        if (low) atomicAdd(&s_ctr[1], 1u);
    }
    __syncthreads();
    if (threadIdx.x < 2 && s_ctr[threadIdx.x]) atomicAdd(&ctr[CL_N_CLIPPED + threadIdx.x], (unsigned long long)s_ctr[threadIdx.x]);
}

__global__ __launch_bounds__(kBlock) void k_clip_write(ClipIn C, const uint16_t* __restrict__ sl, const uint16_t* __restrict__ sr,
                                                       const uint32_t* __restrict__ cut_i, const uint32_t* __restrict__ cut_j,
                                                       const uint64_t* __restrict__ out_off, uint64_t cap, uint32_t* __restrict__ out)
{
    const uint64_t e = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (e >= C.n_sel) return;
    uint64_t a, b;
    runs_of(C, e, &a, &b);
    const uint64_t j = min(uint64_t(cut_j[e]), b - a), i = min(uint64_t(cut_i[e]), j);
    uint64_t pos = out_off[e];
    const uint64_t lim = min(out_off[e + 1], cap);             // no run at or past lim (k_clip_pick counted exactly these)
    if (sl[e]) {
        if (pos < lim) out[pos] = (uint32_t(sl[e]) << 4) | OP_S;
        ++pos;
    }
    for (uint64_t k = i; k < j; ++k, ++pos)
        if (pos < lim) out[pos] = C.cigar[a + k];
    if (sr[e] && pos < lim) out[pos] = (uint32_t(sr[e]) << 4) | OP_S;
}

} // namespace

struct kmx_clips {
    int device = 0;
    hipStream_t stream = nullptr;          // the stream of the call that filled the handle (the host view copies on it)
    uint64_t n_sel = 0, n_ops = 0, n_clipped = 0, n_low = 0;
    bool filled = false;                   // a call has succeeded since the last refusal or error: cig_off holds n_sel + 1 offsets
    // results
    Buf score, sl, sr, tl, tr, nm, cflags, cig_off, cigar;
    // scratch
    Buf cut_i, cut_j, cnt, bsum, ctr;
    Buf extra[kmx::kClipsExtra];           // the scratch of kmx_scripts_realign (kmx_realign.hip)
    Pinned h_extra;
    Pinned h_ctr, h_score, h_sl, h_sr, h_tl, h_tr, h_nm, h_cflags, h_cig_off, h_cigar;
    bool host_valid = false;
    void release()
    {
        for (Buf* b : {&score, &sl, &sr, &tl, &tr, &nm, &cflags, &cig_off, &cigar, &cut_i, &cut_j, &cnt, &bsum, &ctr}) b->release();
        for (Buf& b : extra) b.release();
        for (Pinned* b : {&h_extra, &h_ctr, &h_score, &h_sl, &h_sr, &h_tl, &h_tr, &h_nm, &h_cflags, &h_cig_off, &h_cigar}) b->release();
    }
    void clear() { n_sel = n_ops = n_clipped = n_low = 0; filled = false; host_valid = false; }
};

namespace {

kmx_status clip_run(const kmx::ScriptsAccess& S, const kmx_clip_options& o, hipStream_t s, kmx_clips* h)
{
    const uint64_t ns = S.n_sel;
    h->stream = s;
    h->clear();
    (void)hipGetLastError();
    TRY_HIP(h->cig_off.ensure((ns + 1) * 8));
    if (ns == 0) {                                             // no entry: no launch indexes an empty array
        TRY_HIP(hipMemsetAsync(h->cig_off.p, 0, 8, s));
        h->filled = true;
        return KMX_OK;
    }
    const uint64_t cap = S.n_ops + 2 * ns;                     // an entry gets at most its runs and an S at either end
    TRY_HIP(h->score.ensure(ns * 4));
    for (Buf* b : {&h->sl, &h->sr, &h->tl, &h->tr, &h->nm}) TRY_HIP(b->ensure(ns * 2));
    TRY_HIP(h->cflags.ensure(ns));
    for (Buf* b : {&h->cut_i, &h->cut_j, &h->cnt}) TRY_HIP(b->ensure(ns * 4 + 16));
    TRY_HIP(h->bsum.ensure(kmx::scan_blocks(ns) * 8 + 16));
    TRY_HIP(h->cigar.ensure(cap * 4));
    TRY_HIP(h->ctr.ensure(CL_COUNT * 8));
    unsigned long long* ctr = h->ctr.as<unsigned long long>();
    TRY_HIP(hipMemsetAsync(ctr, 0, CL_COUNT * 8, s));
    const ClipIn C{S.cig_off, S.cigar, ns, S.n_ops, int64_t(o.match), int64_t(o.mismatch), int64_t(o.gap_open), int64_t(o.gap_extend),
                   int64_t(o.clip_penalty), int64_t(o.min_score)};
    const ClipOut O{h->score.as<int32_t>(), h->sl.as<uint16_t>(), h->sr.as<uint16_t>(), h->tl.as<uint16_t>(), h->tr.as<uint16_t>(),
                    h->nm.as<uint16_t>(), h->cflags.as<uint8_t>(), h->cut_i.as<uint32_t>(), h->cut_j.as<uint32_t>(), h->cnt.as<uint32_t>()};
    const dim3 grid(grid_for(ns, kBlock)), block(kBlock);
    hipLaunchKernelGGL(k_clip_pick, grid, block, 0, s, C, O, ctr);
    kmx::launch_scan(s, h->cnt.as<uint32_t>(), ns, h->bsum.as<uint64_t>(), h->cig_off.as<uint64_t>(), ctr + CL_N_OPS);
    hipLaunchKernelGGL(k_clip_write, grid, block, 0, s, C, h->sl.as<uint16_t>(), h->sr.as<uint16_t>(), h->cut_i.as<uint32_t>(),
                       h->cut_j.as<uint32_t>(), h->cig_off.as<uint64_t>(), cap, h->cigar.as<uint32_t>());
    TRY_HIP(hipGetLastError());
    TRY_KMX(kmx::read_back("kmx_scripts_clip", s, ctr, h->h_ctr, CL_COUNT * 8));   // the one synchronisation: the counts
    const uint64_t* c = h->h_ctr.as<uint64_t>();
    if (c[CL_N_OPS] > cap) return kmx::set_error(KMX_ERR_HIP, "kmx_scripts_clip: more runs than the bound");   // (never: a guard for the views)
    h->n_sel = ns;
    h->n_ops = c[CL_N_OPS];
    h->n_clipped = c[CL_N_CLIPPED];
    h->n_low = c[CL_N_LOW];
    h->filled = true;
    return KMX_OK;
}

} // namespace

kmx::ClipsAccess kmx::clips_access(const kmx_clips* c)
{
    return ClipsAccess{c->device, c->n_sel, c->n_ops, c->tl.as<uint16_t>(), c->tr.as<uint16_t>(), c->cig_off.as<uint64_t>(),
                       c->cigar.as<uint32_t>(), c->stream, c->score.as<int32_t>(), c->sl.as<uint16_t>(), c->sr.as<uint16_t>(), c->nm.as<uint16_t>(),
                       c->cflags.as<uint8_t>()};
}

kmx_status kmx::clips_bind(kmx_clips** inout, int device) { return kmx::bind_handle(inout, device); }

kmx_status kmx::clips_begin(kmx_clips* h, hipStream_t s, uint64_t ns, ClipsFill* out)
{
    h->stream = s;
    h->clear();
    (void)hipGetLastError();
    TRY_HIP(h->cig_off.ensure((ns + 1) * 8));
    if (ns == 0) {                                             // no entry: no launch indexes an empty array
        TRY_HIP(hipMemsetAsync(h->cig_off.p, 0, 8, s));
        h->filled = true;
    } else {
        TRY_HIP(h->score.ensure(ns * 4));
        for (Buf* b : {&h->sl, &h->sr, &h->tl, &h->tr, &h->nm}) TRY_HIP(b->ensure(ns * 2));
        TRY_HIP(h->cflags.ensure(ns));
        TRY_HIP(h->cnt.ensure(ns * 4 + 16));
        TRY_HIP(h->bsum.ensure(kmx::scan_blocks(ns) * 8 + 16));
    }
    *out = ClipsFill{h->score.as<int32_t>(), h->sl.as<uint16_t>(), h->sr.as<uint16_t>(), h->tl.as<uint16_t>(), h->tr.as<uint16_t>(),
                     h->nm.as<uint16_t>(), h->cflags.as<uint8_t>(), h->cig_off.as<uint64_t>(), h->cnt.as<uint32_t>(), h->bsum.as<uint64_t>(),
                     h->extra, &h->h_extra};
    return KMX_OK;
}

kmx_status kmx::clips_runs(kmx_clips* h, uint64_t n_ops, uint32_t** cigar)
{
    TRY_HIP(h->cigar.ensure(std::max<uint64_t>(n_ops, 1) * 4));
    *cigar = h->cigar.as<uint32_t>();
    return KMX_OK;
}

void kmx::clips_finish(kmx_clips* h, uint64_t n_sel, uint64_t n_ops, uint64_t n_clipped, uint64_t n_low)
{
    h->n_sel = n_sel;
    h->n_ops = n_ops;
    h->n_clipped = n_clipped;
    h->n_low = n_low;
    h->filled = true;
}

void kmx::clips_clear(kmx_clips* h) { h->clear(); }

extern "C" {

kmx_status kmx_scripts_clip(const kmx_scripts* scripts, const kmx_clip_options* o, void* stream, kmx_clips** inout)
{
    const std::string who = "kmx_scripts_clip: ";
    if (!o) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "options is NULL");
    if (!inout) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "inout is NULL");
    if (o->struct_size < sizeof(kmx_clip_options)) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "options->struct_size is too small");
    if (o->flags != 0) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "flags must be 0");
    if (o->match < 1 || o->match > 255) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "match outside 1 .. 255");
    if (o->mismatch > 255) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "mismatch > 255");
    if (o->gap_open > 255) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "gap_open > 255");
    if (o->gap_extend > 255) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "gap_extend > 255");
    if (o->clip_penalty > 65535) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "clip_penalty > 65535");
    if (!scripts) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "scripts handle is NULL");
    const kmx::ScriptsAccess S = kmx::scripts_access(scripts);
    kmx_clips* h = *inout;
    if (S.flags & KMX_SCRIPT_M) {
        if (h) h->clear();
        return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "the scripts were made with KMX_SCRIPT_M: a score needs '=' and 'X' apart");
    }
    kmx::DeviceGuard dg;
    const kmx_status bound = kmx::bind_handle(inout, S.device);
    h = *inout;
    if (bound != KMX_OK) {
        if (h) h->clear();
        return bound;
    }
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : S.stream;
    const kmx_status st = clip_run(S, *o, s, h);
    if (st != KMX_OK) {                                        // the handle holds an empty result, not half of this one
        (void)hipStreamSynchronize(s);
        h->clear();
    }
    return st;
}

kmx_status kmx_clips_counts(const kmx_clips* h, uint64_t* n_sel, uint64_t* n_ops, uint64_t* n_clipped, uint64_t* n_low)
{
    if (!h) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_clips_counts: clips handle is NULL");
    if (n_sel) *n_sel = h->n_sel;
    if (n_ops) *n_ops = h->n_ops;
    if (n_clipped) *n_clipped = h->n_clipped;
    if (n_low) *n_low = h->n_low;
    return KMX_OK;
}

kmx_status kmx_clips_view_device(const kmx_clips* h, const int32_t** d_score, const uint16_t** d_sl, const uint16_t** d_sr, const uint16_t** d_tl,
                                 const uint16_t** d_tr, const uint16_t** d_nm, const uint8_t** d_cflags, const uint64_t** d_cig_off,
                                 const uint32_t** d_cigar)
{
    if (!h) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_clips_view_device: clips handle is NULL");
    const bool any = h->n_sel != 0;
    if (d_score) *d_score = any ? h->score.as<int32_t>() : nullptr;
    if (d_sl) *d_sl = any ? h->sl.as<uint16_t>() : nullptr;
    if (d_sr) *d_sr = any ? h->sr.as<uint16_t>() : nullptr;
    if (d_tl) *d_tl = any ? h->tl.as<uint16_t>() : nullptr;
    if (d_tr) *d_tr = any ? h->tr.as<uint16_t>() : nullptr;
    if (d_nm) *d_nm = any ? h->nm.as<uint16_t>() : nullptr;
    if (d_cflags) *d_cflags = any ? h->cflags.as<uint8_t>() : nullptr;
    if (d_cig_off) *d_cig_off = h->filled ? h->cig_off.as<uint64_t>() : nullptr;
    if (d_cigar) *d_cigar = h->n_ops ? h->cigar.as<uint32_t>() : nullptr;
    return KMX_OK;
}

kmx_status kmx_clips_view(kmx_clips* h, const int32_t** score, const uint16_t** sl, const uint16_t** sr, const uint16_t** tl, const uint16_t** tr,
                          const uint16_t** nm, const uint8_t** cflags, const uint64_t** cig_off, const uint32_t** cigar)
{
    if (!h) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_clips_view: clips handle is NULL");
    if (!h->host_valid) {                                      // 15 bytes per entry, 8 per entry for cig_off, 4 per run
        const uint64_t ns = h->n_sel;
        const bool f = h->filled;                              // else the empty result: one offset, 0
        const kmx::HostCopy items[] = {{h->h_score, h->score, ns, 4}, {h->h_sl, h->sl, ns, 2}, {h->h_sr, h->sr, ns, 2}, {h->h_tl, h->tl, ns, 2},
                                       {h->h_tr, h->tr, ns, 2}, {h->h_nm, h->nm, ns, 2}, {h->h_cflags, h->cflags, ns, 1},
                                       {h->h_cig_off, h->cig_off, f ? ns + 1 : 0, 8}, {h->h_cigar, h->cigar, h->n_ops, 4}};
        TRY_KMX(kmx::host_view("kmx_clips_view", h->device, h->stream, items, std::size(items)));
        if (!f) h->h_cig_off.as<uint64_t>()[0] = 0;
        h->host_valid = true;
    }
    if (score) *score = h->h_score.as<int32_t>();
    if (sl) *sl = h->h_sl.as<uint16_t>();
    if (sr) *sr = h->h_sr.as<uint16_t>();
    if (tl) *tl = h->h_tl.as<uint16_t>();
    if (tr) *tr = h->h_tr.as<uint16_t>();
    if (nm) *nm = h->h_nm.as<uint16_t>();
    if (cflags) *cflags = h->h_cflags.as<uint8_t>();
    if (cig_off) *cig_off = h->h_cig_off.as<uint64_t>();
    if (cigar) *cigar = h->h_cigar.as<uint32_t>();
    return KMX_OK;
}

void kmx_clips_free(kmx_clips* h) { kmx::free_handle(h); }

} // extern "C"
