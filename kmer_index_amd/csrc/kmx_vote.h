// What seed voting (kmx_vote.hip) needs from the result of a windows search (kmx_capi.hip owns struct kmx_result).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <functional>

#include "kmx_handle.h"

namespace kmx {

// The last search into a result, when it was a windows search with positions on one device (all pointers are device pointers
// that belong to the result and stay as they are: voting only reads them).
struct WindowsAccess {
    int device;
    hipStream_t stream;            // the stream of that search: the result's own (host form) or the caller's (device form)
    const kmx_index* index;        // for the kernel statistics only; nullptr once the index has been freed
    uint64_t nr, nq, n_hits;       // reads, windows, hits
    uint64_t n;                    // text length of the index that was searched
    uint32_t w, stride;
    const uint64_t* win_off;       // [nr + 1]
    const uint64_t* hit_off;       // [nq + 1]
    const uint32_t* positions;     // [n_hits]
};
// kmx_capi.hip: completes a pending search; the refusals "after looking at the handle" of kmx_windows_vote
kmx_status windows_access(kmx_result* r, WindowsAccess* out);
// kmx_capi.hip: launch() timed under the name k_vote when the index collects statistics
void vote_timed(const kmx_index* ix, hipStream_t s, const std::function<void()>& launch);

// What alignment at the loci (kmx_align.hip) needs from a loci handle (kmx_vote.hip owns struct kmx_loci): device pointers that
// belong to the handle and stay as they are (aligning only reads them).  A handle that no vote has filled yet has nr = 0.
struct LociAccess {
    int device;
    hipStream_t stream;            // the stream of the vote that filled the handle
    uint64_t nr, n_loci;
    const uint64_t* locus_off;     // [nr + 1]
    const int64_t* diag;           // [n_loci]
    const uint32_t* span;
    const uint32_t* votes;
};
LociAccess loci_access(const kmx_loci* l);   // kmx_vote.hip

// What the edit scripts (kmx_script.hip) need from an alignments handle (kmx_align.hip owns struct kmx_alignments): device
// pointers that belong to the handle and stay as they are (the scripts only read them).  dist / start / end are only looked at
// when n_loci > 0.  A handle that no call has filled yet has nr = 0.
struct AlignAccess {
    int device;
    hipStream_t stream;            // the stream of the call that filled the handle
    uint64_t nr, n_loci;
    const uint8_t* dist;           // [n_loci]
    const uint32_t* start;
    const uint32_t* end;
    const uint32_t* best;          // [nr]
    const uint32_t* ctg;           // [n_loci]: the contig of every locus; nullptr when the handle was made without a contig table
    uint64_t nc, ctg_gen;          // the contigs and the generation of the table the call saw (kmx_approx.h: ContigTable)
};
AlignAccess alignments_access(const kmx_alignments* a);   // kmx_align.hip

// What the scripts of the winners (kmx_placements_scripts) need from a placements handle (kmx_strands.hip owns struct
// kmx_placements): best2 belongs to the handle and stays as it is (the scripts only read it).  A handle that no fold has filled yet
// has nr2 = 0.  The secondary placements (kmx_secondary.hip) read the five placement arrays of the nr public reads as well.
struct PlacementsAccess {
    int device;
    hipStream_t stream;            // the stream of the fold that filled the handle
    uint64_t nr2;                  // internal reads: twice the public ones
    const uint32_t* best2;         // [nr2]: best[] of the alignments with the losing strand's entry cleared
    uint64_t nr;                   // public reads
    const uint32_t* locus;         // [nr]
    const uint8_t* strand;
    const uint8_t* dist;
    const uint32_t* start;
    const uint32_t* end;
};
PlacementsAccess placements_access(const kmx_placements* p);   // kmx_strands.hip
// kmx_script.hip: kmx_alignments_scripts_device on the reads d_ranks / d_roff (at most ranks_len letters) with P.best2 in the place
// of the alignments' best; `fn` names the entry point in the error text
kmx_status scripts_with_best(const char* fn, const kmx_index* index, const kmx_loci* loci, const kmx_alignments* alignments, const void* d_ranks,
                             const void* d_roff, uint64_t nr, uint64_t ranks_len, const kmx_script_options* options, hipStream_t stream,
                             const PlacementsAccess& P, kmx_scripts** inout);
// kmx_script.hip: the scripts of the entries that best[L.nr] selects among arrays shaped like loci and alignments (L: nr, n_loci and
// locus_off; A: dist / start / end) over the reads d_ranks / d_roff, on `stream`; the refusals of the options and of the index are
// those of kmx_alignments_scripts_device, and KMX_SCRIPT_ALL in the options is refused.  every == true: every entry with a distance
// is selected and best is not looked at (the KMX_SCRIPT_ALL path, which only a caller inside the library may ask for).
// kmx_rescues_scripts (kmx_rescue.hip) and kmx_secondaries_scripts (kmx_secondary.hip, every == true) are its callers.
kmx_status scripts_on_arrays(const char* fn, const kmx_index* index, const LociAccess& L, const AlignAccess& A, const void* d_ranks,
                             const void* d_roff, uint64_t ranks_len, const uint32_t* best, const kmx_script_options* options,
                             hipStream_t stream, kmx_scripts** inout, bool every = false);

// What the MD strings (kmx_tags.hip) need from a scripts handle (kmx_script.hip owns struct kmx_scripts): device pointers that belong
// to the handle and stay as they are (the MD only reads them).  sel is only looked at when n_sel > 0, cigar when n_ops > 0; a handle
// that no call has filled (or whose last call was refused) has n_sel = 0.  flags: the kmx_script_options::flags of the call that
// filled it.
struct ScriptsAccess {
    int device;
    hipStream_t stream;            // the stream of the call that filled the handle
    uint64_t n_sel, n_ops;
    uint32_t flags;
    const uint32_t* sel;           // [n_sel]
    const uint64_t* cig_off;       // [n_sel + 1]
    const uint32_t* cigar;         // [n_ops]
    uint64_t nr;                   // the reads the entries run over (kmx_supplementary.hip)
    const uint64_t* read_sel_off;  // [nr + 1]
};
ScriptsAccess scripts_access(const kmx_scripts* s);   // kmx_script.hip

// ... and from the job arrays of a rescues handle (kmx_rescue.hip owns struct kmx_rescues), which the sel of kmx_rescues_scripts indexes
struct JobsAccess {
    int device;
    hipStream_t stream;            // the stream of the rescue that filled the handle
    uint64_t n_jobs;
    const uint32_t* start;         // [n_jobs]
    const uint32_t* end;
};
JobsAccess rescues_access(const kmx_rescues* r);   // kmx_rescue.hip
// ... and from the entry arrays of a secondaries handle (kmx_secondary.hip owns struct kmx_secondaries; n_jobs = n_sec), which the
// sel of kmx_secondaries_scripts indexes
JobsAccess secondaries_access(const kmx_secondaries* s);   // kmx_secondary.hip

// What the MD of clipped entries (kmx_clips_md, kmx_clips_rescues_md; kmx_tags.hip) needs from a clips handle (kmx_clips.h holds
// struct kmx_clips): the clipped runs and the text letters clipped off either side.  The per-entry arrays are only looked at when
// n_sel > 0, cigar when n_ops > 0; a handle that no call has filled (or whose last call was refused) has n_sel = 0.  The supplementary
// alignments (kmx_supplementary.hip) read the other per-entry values as well.
struct ClipsAccess {
    int device;
    uint64_t n_sel, n_ops;
    const uint16_t* tl;            // [n_sel]
    const uint16_t* tr;
    const uint64_t* cig_off;       // [n_sel + 1]
    const uint32_t* cigar;         // [n_ops]
    hipStream_t stream;            // the stream of the call that filled the handle
    const int32_t* score;          // [n_sel]
    const uint16_t* sl;
    const uint16_t* sr;
    const uint16_t* nm;
    const uint8_t* cflags;
};
ClipsAccess clips_access(const kmx_clips* c);   // kmx_clip.hip

} // namespace kmx
