// The clips handle, which two calls fill: kmx_scripts_clip (kmx_clip.hip, which owns the accessor and the views) and
// kmx_scripts_realign (kmx_realign.hip); the MD of clipped entries (kmx_tags.hip) and the supplementary alignments
// (kmx_supplementary.hip) read it through kmx::ClipsAccess (kmx_vote.h).  Private to the library.
#pragma once
#include "kmx_handle.h"
#include "kmx_kernels.h"

namespace kmx {
// the batch counters a filler's kernels add up, in this order wherever its counter array has them
enum { CL_N_OPS = 0, CL_N_CLIPPED, CL_N_LOW, CL_COUNT };

// the refusals of the flags and the scoring of kmx_clip_options / kmx_realign_options
template <typename O>
kmx_status check_scoring(const std::string& who, const O& o)
{
    if (o.flags != 0) return set_error(KMX_ERR_INVALID_ARGUMENT, who + "flags must be 0");
    if (o.match < 1 || o.match > 255) return set_error(KMX_ERR_INVALID_ARGUMENT, who + "match outside 1 .. 255");
    if (o.mismatch > 255) return set_error(KMX_ERR_INVALID_ARGUMENT, who + "mismatch > 255");
    if (o.gap_open > 255) return set_error(KMX_ERR_INVALID_ARGUMENT, who + "gap_open > 255");
    if (o.gap_extend > 255) return set_error(KMX_ERR_INVALID_ARGUMENT, who + "gap_extend > 255");
    if (o.clip_penalty > 65535) return set_error(KMX_ERR_INVALID_ARGUMENT, who + "clip_penalty > 65535");
    return KMX_OK;
}
} // namespace kmx

struct kmx_clips {
    int device = 0;
    hipStream_t stream = nullptr;          // the stream of the call that filled the handle (the host view copies on it)
    uint64_t n_sel = 0, n_ops = 0, n_clipped = 0, n_low = 0;
    // results: one entry per entry of the scripts, the offsets of their runs and the runs
    kmx::ArrOf<int32_t> score;
    kmx::ArrOf<uint16_t> sl, sr, tl, tr, nm;
    kmx::ArrOf<uint8_t> cflags;
    kmx::ArrOf<uint64_t> cig_off{kmx::ARR_OFFSETS};
    kmx::ArrOf<uint32_t> cigar;
    // scratch of both fillers: the runs of every entry and the block sums of the scan that gives cig_off, the counters
    kmx::Buf cnt, bsum, ctr;
    // scratch of kmx_scripts_clip: the cuts
    kmx::Buf cut_i, cut_j;
    // scratch of kmx_scripts_realign: the uploaded reads (host form), the per-entry values of the band and of the walk, the
    // traceback codes of a chunk and the run reservations
    struct Realign {
        kmx::Buf ranks, roff, eread, estat, ecode, eres, code_off, res_off, end_i, end_j, end_v, arena, runs;
    } re;
    kmx::PinnedArr h_ctr;
    bool host_valid = false;
    std::vector<kmx::Arr*> results() { return {&score, &sl, &sr, &tl, &tr, &nm, &cflags, &cig_off, &cigar}; }
    std::vector<kmx::Buf*> scratch()
    {
        return {&cnt, &bsum, &ctr, &cut_i, &cut_j, &re.ranks, &re.roff, &re.eread, &re.estat, &re.ecode, &re.eres, &re.code_off, &re.res_off, &re.end_i,
                &re.end_j, &re.end_v, &re.arena, &re.runs};
    }
    void release() { kmx::release_arrays(*this); }
    void clear() { n_sel = n_ops = n_clipped = n_low = 0; kmx::clear_arrays(*this); }
    // a filler has succeeded: the arrays expose what the counters say
    void expose()
    {
        kmx::expose(results(), n_sel);
        cig_off.n = n_sel + 1;
        cigar.n = n_ops;
    }

    // The steps of a filler, in this order.  begin: an empty result on stream s, then room for the per-entry arrays of ns entries, cnt
    // and bsum; with ns == 0 the one offset 0 is written and the handle is filled, and the filler is done.
    kmx_status begin(hipStream_t s, uint64_t ns)
    {
        stream = s;
        clear();
        (void)hipGetLastError();
        TRY_HIP(cig_off.ensure((ns + 1) * 8));
        if (ns == 0) {                                         // no entry: no launch indexes an empty array
            TRY_HIP(hipMemsetAsync(cig_off.p, 0, 8, s));
            expose();
            return KMX_OK;
        }
        TRY_HIP(score.ensure(ns * 4));
        for (kmx::Arr* a : {&sl, &sr, &tl, &tr, &nm}) TRY_HIP(a->ensure(ns * 2));
        TRY_HIP(cflags.ensure(ns));
        TRY_HIP(cnt.ensure(ns * 4 + 16));
        TRY_HIP(bsum.ensure(kmx::scan_blocks(ns) * 8 + 16));
        return KMX_OK;
    }
    // room for n runs in cigar
    kmx_status runs(uint64_t n)
    {
        TRY_HIP(cigar.ensure(std::max<uint64_t>(n, 1) * 4));
        return KMX_OK;
    }
    // the handle is filled with ns entries; counts: the CL_* counters as they were read back
    void finish(uint64_t ns, const uint64_t* counts)
    {
        n_sel = ns;
        n_ops = counts[kmx::CL_N_OPS];
        n_clipped = counts[kmx::CL_N_CLIPPED];
        n_low = counts[kmx::CL_N_LOW];
        expose();
    }
};
