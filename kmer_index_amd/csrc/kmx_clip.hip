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

#include "kmx_clips.h"
#include "kmx_kernels.h"
#include "kmx_runs.h"
#include "kmx_vote.h"

namespace {

constexpr uint32_t kBlock = 256;

using kmx::Buf;
using kmx::grid_for;

struct ClipIn {
    const uint64_t* cig_off;       // [n_sel + 1]: the scripts'
    const uint32_t* cigar;         // [n_ops]
    uint64_t n_sel, n_ops;
    Scoring G;
};

// cut_i / cut_j: scratch, the cuts for k_clip_write
__global__ __launch_bounds__(kBlock) void k_clip_pick(ClipIn C, ClipOut O, uint32_t* __restrict__ cut_i, uint32_t* __restrict__ cut_j,
                                                      unsigned long long* __restrict__ ctr)
{
    __shared__ unsigned int s_ctr[2];                          // clipped, low
    if (threadIdx.x < 2) s_ctr[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t e = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (e < C.n_sel) {
        const Scoring& G = C.G;
        uint64_t a, b;
        runs_of(C.cig_off, C.n_ops, e, &a, &b);
        const uint32_t R = uint32_t(b - a);
        // the best (V, i, j): (0, R) is a candidate for every R, the loop meets it at its last run
        int64_t W = 0, min_left = 0, best_v = 0;
        uint32_t min_i = 0, bi = 0, bj = R;
        bool bad = false, have = R == 0;
        for (uint32_t k = 0; k < R; ++k) {
            const uint32_t v = C.cigar[a + k];
            const bool eq = run_op(v) == OP_EQ;
            if (eq && k > 0 && W + G.p < min_left) { min_left = W + G.p; min_i = k; }   // a left cut; among equals the smallest stays
            W += run_score(G, v, &bad);
            if (eq || k + 1 == R) {                            // a right cut behind run k
                const int64_t val = W - (k + 1 < R ? G.p : 0) - min_left;
                if (!have || val > best_v || (val == best_v && min_i <= bi)) {        // (equal i: this j is the larger one)
                    have = true;
                    best_v = val;
                    bi = min_i;
                    bj = k + 1;
                }
            }
        }
        const bool low = bad || best_v < G.min_score;
        if (low) {
            whole_entry(G, C.cigar + a, R, nullptr, O, e);
            cut_i[e] = 0;
            cut_j[e] = R;
        } else {
            uint64_t sl = 0, sr = 0, tl = 0, tr = 0, nm = 0;
            for (uint32_t k = 0; k < R; ++k) {
                const uint32_t v = C.cigar[a + k], op = run_op(v);
                const uint64_t len = run_len(v);
                const uint64_t rd = op == OP_D ? 0 : len, tx = op == OP_I ? 0 : len;
                if (k < bi) { sl += rd; tl += tx; }
                else if (k >= bj) { sr += rd; tr += tx; }
                else if (op != OP_EQ) nm += len;
            }
            O.score[e] = sat32(best_v);
            O.sl[e] = sat16(sl);
            O.sr[e] = sat16(sr);
            O.tl[e] = sat16(tl);
            O.tr[e] = sat16(tr);
            O.nm[e] = sat16(nm);
            O.cflags[e] = uint8_t(0);
            O.cnt[e] = (bj - bi) + (sl ? 1u : 0u) + (sr ? 1u : 0u);
            cut_i[e] = bi;
            cut_j[e] = bj;
            if (sl + sr) atomicAdd(&s_ctr[0], 1u);
        }
        if (low) atomicAdd(&s_ctr[1], 1u);
    }
    __syncthreads();
    if (threadIdx.x < 2 && s_ctr[threadIdx.x]) atomicAdd(&ctr[kmx::CL_N_CLIPPED + threadIdx.x], (unsigned long long)s_ctr[threadIdx.x]);
}

__global__ __launch_bounds__(kBlock) void k_clip_write(ClipIn C, const uint16_t* __restrict__ sl, const uint16_t* __restrict__ sr,
                                                       const uint32_t* __restrict__ cut_i, const uint32_t* __restrict__ cut_j,
                                                       const uint64_t* __restrict__ out_off, uint64_t cap, uint32_t* __restrict__ out)
{
    const uint64_t e = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (e >= C.n_sel) return;
    uint64_t a, b;
    runs_of(C.cig_off, C.n_ops, e, &a, &b);
    const uint64_t j = min(uint64_t(cut_j[e]), b - a), i = min(uint64_t(cut_i[e]), j);
    uint64_t pos = out_off[e];
    const uint64_t lim = min(out_off[e + 1], cap);             // no run at or past lim (k_clip_pick counted exactly these)
    if (sl[e]) {
        if (pos < lim) out[pos] = make_run(sl[e], OP_S);
        ++pos;
    }
    for (uint64_t k = i; k < j; ++k, ++pos)
        if (pos < lim) out[pos] = C.cigar[a + k];
    if (sr[e] && pos < lim) out[pos] = make_run(sr[e], OP_S);
}

kmx_status clip_run(const kmx::ScriptsAccess& S, const kmx_clip_options& o, hipStream_t s, kmx_clips* h)
{
    const uint64_t ns = S.n_sel;
    TRY_KMX(h->begin(s, ns));
    if (ns == 0) return KMX_OK;
    const uint64_t cap = S.n_ops + 2 * ns;                     // an entry gets at most its runs and an S at either end
    for (Buf* b : {&h->cut_i, &h->cut_j}) TRY_HIP(b->ensure(ns * 4));
    TRY_KMX(h->runs(cap));
    TRY_HIP(h->ctr.ensure(kmx::CL_COUNT * 8));
    unsigned long long* ctr = h->ctr.as<unsigned long long>();
    TRY_HIP(hipMemsetAsync(ctr, 0, kmx::CL_COUNT * 8, s));
    const ClipIn C{S.cig_off, S.cigar, ns, S.n_ops,
                   Scoring{int(o.match), int(o.mismatch), int(o.gap_open), int(o.gap_extend), int(o.clip_penalty), o.min_score}};
    const ClipOut O{h->score.as<int32_t>(), h->sl.as<uint16_t>(), h->sr.as<uint16_t>(), h->tl.as<uint16_t>(), h->tr.as<uint16_t>(),
                    h->nm.as<uint16_t>(), h->cflags.as<uint8_t>(), h->cnt.as<uint32_t>()};
    const dim3 grid(grid_for(ns, kBlock)), block(kBlock);
    hipLaunchKernelGGL(k_clip_pick, grid, block, 0, s, C, O, h->cut_i.as<uint32_t>(), h->cut_j.as<uint32_t>(), ctr);
    kmx::launch_scan(s, h->cnt.as<uint32_t>(), ns, h->bsum.as<uint64_t>(), h->cig_off.as<uint64_t>(), ctr + kmx::CL_N_OPS);
    hipLaunchKernelGGL(k_clip_write, grid, block, 0, s, C, h->sl.as<uint16_t>(), h->sr.as<uint16_t>(), h->cut_i.as<uint32_t>(),
                       h->cut_j.as<uint32_t>(), h->cig_off.as<uint64_t>(), cap, h->cigar.as<uint32_t>());
    TRY_HIP(hipGetLastError());
    TRY_KMX(kmx::read_back("kmx_scripts_clip", s, ctr, h->h_ctr, kmx::CL_COUNT * 8));   // the one synchronisation: the counts
    const uint64_t* c = h->h_ctr.as<uint64_t>();
    if (c[kmx::CL_N_OPS] > cap) return kmx::set_error(KMX_ERR_HIP, "kmx_scripts_clip: more runs than the bound");   // (never: a guard for the views)
    h->finish(ns, c);
    return KMX_OK;
}

} // namespace

kmx::ClipsAccess kmx::clips_access(const kmx_clips* c)
{
    return ClipsAccess{c->device, c->n_sel, c->n_ops, c->tl.as<uint16_t>(), c->tr.as<uint16_t>(), c->cig_off.as<uint64_t>(),
                       c->cigar.as<uint32_t>(), c->stream, c->score.as<int32_t>(), c->sl.as<uint16_t>(), c->sr.as<uint16_t>(), c->nm.as<uint16_t>(),
                       c->cflags.as<uint8_t>()};
}

extern "C" {

kmx_status kmx_scripts_clip(const kmx_scripts* scripts, const kmx_clip_options* o, void* stream, kmx_clips** inout)
{
    const std::string who = "kmx_scripts_clip: ";
    TRY_KMX(kmx::check_call(who, o, inout));
    TRY_KMX(kmx::check_scoring(who, *o));
    if (!scripts) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "scripts handle is NULL");
    const kmx::ScriptsAccess S = kmx::scripts_access(scripts);
    kmx_clips* h = *inout;
    if (S.flags & KMX_SCRIPT_M) {
        if (h) h->clear();
        return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, who + "the scripts were made with KMX_SCRIPT_M: a score needs '=' and 'X' apart");
    }
    kmx::DeviceGuard dg;
    TRY_KMX(kmx::bind_handle(inout, S.device));
    h = *inout;
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
    if (d_score) *d_score = h->score.dev();
    if (d_sl) *d_sl = h->sl.dev();
    if (d_sr) *d_sr = h->sr.dev();
    if (d_tl) *d_tl = h->tl.dev();
    if (d_tr) *d_tr = h->tr.dev();
    if (d_nm) *d_nm = h->nm.dev();
    if (d_cflags) *d_cflags = h->cflags.dev();
    if (d_cig_off) *d_cig_off = h->cig_off.dev();
    if (d_cigar) *d_cigar = h->cigar.dev();
    return KMX_OK;
}

kmx_status kmx_clips_view(kmx_clips* h, const int32_t** score, const uint16_t** sl, const uint16_t** sr, const uint16_t** tl, const uint16_t** tr,
                          const uint16_t** nm, const uint8_t** cflags, const uint64_t** cig_off, const uint32_t** cigar)
{
    if (!h) return kmx::set_error(KMX_ERR_INVALID_ARGUMENT, "kmx_clips_view: clips handle is NULL");
    TRY_KMX(kmx::host_view("kmx_clips_view", *h));             // 15 bytes per entry, 8 per entry for cig_off, 4 per run
    if (score) *score = h->score.host();
    if (sl) *sl = h->sl.host();
    if (sr) *sr = h->sr.host();
    if (tl) *tl = h->tl.host();
    if (tr) *tr = h->tr.host();
    if (nm) *nm = h->nm.host();
    if (cflags) *cflags = h->cflags.host();
    if (cig_off) *cig_off = h->cig_off.host();
    if (cigar) *cigar = h->cigar.host();
    return KMX_OK;
}

void kmx_clips_free(kmx_clips* h) { kmx::free_handle(h); }

} // extern "C"
