// The placements handle, which two folds fill: kmx_alignments_fold_strands (kmx_strands.hip, which owns the accessors and the scripts
// of the winners) and kmx_alignments_fold_pairs (kmx_pairs.hip); the doubled reads (kmx_strands.hip) and the pairs (kmx_pairs.hip),
// which the mate rescue (kmx_rescue.hip) reads and, with the placements, rewrites; the secondary placements (kmx_secondary.hip) read
// the placements through kmx::PlacementsAccess (kmx_vote.h).  Private to the library.
#pragma once
#include "kmx_handle.h"

namespace kmx {
// the batch counters a fold kernel adds up, in the order of kmx_placements_counts
enum { PL_N_PLACED = 0, PL_N_REVERSE, PL_N_AMBIGUOUS, PL_COUNT };
// ... and, behind them in the same array where a kernel counts both (k_pair_fold, k_rescue_fold), the pairs', in the order of
// kmx_pairs_counts
enum { PR_N_CONCORDANT = PL_COUNT, PR_N_DISCORDANT, PR_N_SINGLE, PR_N_UNPLACED, PR_N_AMBIGUOUS, PR_COUNT };
} // namespace kmx

struct kmx_placements {
    int device = 0;
    hipStream_t stream = nullptr;          // the stream of the call that filled the handle (the host view copies on it)
    uint64_t nr = 0, n_placed = 0, n_reverse = 0, n_ambiguous = 0;
    // results, one entry per public read; best2, a pair per read, goes to the host only when a caller asks for it
    kmx::ArrOf<uint32_t> locus, start, end, best2{kmx::ARR_OWN_VIEW};
    kmx::ArrOf<uint8_t> strand, dist, second;
    kmx::Buf ctr;
    kmx::PinnedArr h_ctr;
    bool host_valid = false, host_best2_valid = false;
    std::vector<kmx::Arr*> results() { return {&locus, &strand, &dist, &start, &end, &second, &best2}; }
    std::vector<kmx::Buf*> scratch() { return {&ctr}; }
    void release() { kmx::release_arrays(*this); }
    void clear() { nr = n_placed = n_reverse = n_ambiguous = 0; kmx::clear_arrays(*this); host_best2_valid = false; }
    // the fold has filled the arrays of n public reads
    void expose(uint64_t n) { nr = n; kmx::expose(results(), n); best2.n = 2 * n; }
    // c: the counters of a fold as they were read back, c[kmx::PL_*] the placements'
    void counts_from(const uint64_t* c) { n_placed = c[kmx::PL_N_PLACED]; n_reverse = c[kmx::PL_N_REVERSE]; n_ambiguous = c[kmx::PL_N_AMBIGUOUS]; }
    // the seven arrays of n public reads
    hipError_t room(uint64_t n)
    {
        for (kmx::Arr* a : results())
            if (hipError_t e = a->ensure((a == &best2 ? 2 : 1) * n * a->elem); e != hipSuccess) return e;
        return hipSuccess;
    }
};

// the doubled batch of kmx_reads_strands
struct kmx_strand_reads {
    int device = 0;
    hipStream_t stream = nullptr;          // the stream of the call that filled the handle
    hipStream_t own = nullptr;             // the stream of the host form, created at its first call
    uint64_t nr2 = 0, letters2 = 0;        // internal reads and their letters
    kmx::Buf raw, roff, ranks2, roff2;
    kmx::PinnedArr h_total;
    void release()
    {
        for (kmx::Buf* b : {&raw, &roff, &ranks2, &roff2}) b->release();
        h_total.release();
        if (own) {                                             // nothing of this handle's is in flight on the stream that goes
            (void)hipStreamSynchronize(own);
            (void)hipStreamDestroy(own);
        }
        own = stream = nullptr;
    }
    void clear() { nr2 = 0; letters2 = 0; }
};

// one entry per pair: kmx_alignments_fold_pairs fills it
struct kmx_pairs {
    int device = 0;
    hipStream_t stream = nullptr;          // the stream of the fold that filled the handle (the host view copies on it)
    uint64_t np = 0, n_concordant = 0, n_discordant = 0, n_single = 0, n_unplaced = 0, n_ambiguous = 0;
    // results, one entry per pair
    kmx::ArrOf<uint8_t> cls;
    kmx::ArrOf<int32_t> tlen;
    kmx::ArrOf<uint16_t> score, second_score;
    kmx::Buf ctr;
    kmx::PinnedArr h_ctr;
    bool host_valid = false;
    std::vector<kmx::Arr*> results() { return {&cls, &tlen, &score, &second_score}; }
    std::vector<kmx::Buf*> scratch() { return {&ctr}; }
    void release() { kmx::release_arrays(*this); }
    void clear() { np = n_concordant = n_discordant = n_single = n_unplaced = n_ambiguous = 0; kmx::clear_arrays(*this); }
    // the fold has filled the arrays of n pairs
    void expose(uint64_t n) { np = n; kmx::expose(results(), n); }
    // c: the counters of a fold as they were read back, c[kmx::PR_*] the pairs'
    void counts_from(const uint64_t* c)
    {
        n_concordant = c[kmx::PR_N_CONCORDANT];
        n_discordant = c[kmx::PR_N_DISCORDANT];
        n_single = c[kmx::PR_N_SINGLE];
        n_unplaced = c[kmx::PR_N_UNPLACED];
        n_ambiguous = c[kmx::PR_N_AMBIGUOUS];
    }
};
