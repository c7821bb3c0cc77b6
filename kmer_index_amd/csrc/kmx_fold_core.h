// What the folds of the read-mapping chain share (k_strand_fold, k_pair_fold, k_rescue_fold, k_sec_pick): the two strand ranges of a
// read among the loci, the winner of a read, the ELSEWHERE rule and the runner-up it defines, the concordance of two mates, and the
// batch counters of the placements and the pairs.  A wave works on one read, so every argument but `lane` is the same in all its
// lanes.  Everything here has internal linkage: each source compiles its own.  Private to the library.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kmx_strands.h"

namespace {

constexpr uint32_t kFoldWave = 64;
constexpr uint64_t kNoLocus = ~uint64_t(0);                    // second_elsewhere: no locus is the chosen one

// The loci of the two strands of the read whose forward strand is internal read `first`: [a, b) forward, [b, c) reverse, inside the
// arrays whatever the offsets hold.  floor: where the ranges of the read before it end (its mate's, in a pair).
__device__ __forceinline__ void strand_ranges(const uint64_t* locus_off, uint64_t n_loci, uint64_t first, uint64_t* a, uint64_t* b, uint64_t* c,
                                              uint64_t floor = 0)
{
    *a = min(max(locus_off[first], floor), n_loci);
    *b = min(max(locus_off[first + 1], *a), n_loci);
    *c = min(max(locus_off[first + 2], *b), n_loci);
}

// The single winner of a read: the better of the bests of its two strands, the forward strand wins a tie.
struct Winner {
    bool placed;
    uint32_t strand, dist;         // dist: KMX_ALIGN_NONE when not placed
    uint64_t locus;                // only when placed
};

__device__ __forceinline__ Winner strand_winner(const uint8_t* dist, const uint32_t* best, uint64_t first, uint64_t a, uint64_t b, uint64_t c)
{
    const uint32_t none = 0xFFFFFFFFu, bf = best[first], br = best[first + 1];
    uint32_t df = KMX_ALIGN_NONE, dr = KMX_ALIGN_NONE;
    if (bf != none && bf < b - a) df = dist[a + bf];
    if (br != none && br < c - b) dr = dist[b + br];
    const bool okf = df < KMX_ALIGN_SKIPPED, okr = dr < KMX_ALIGN_SKIPPED;
    const bool fwd = okf && (!okr || df <= dr);
    Winner W;
    W.placed = okf || okr;
    W.strand = fwd ? 0u : 1u;
    W.dist = W.placed ? (fwd ? df : dr) : uint32_t(KMX_ALIGN_NONE);
    W.locus = fwd ? a + bf : b + br;
    return W;
}

// [start, end) on strand s lies elsewhere from [ws, we) on strand sw: on the other strand, or the two do not overlap
__device__ __forceinline__ bool elsewhere(uint32_t s, uint32_t start, uint32_t end, uint32_t sw, uint32_t ws, uint32_t we)
{
    return s != sw || max(start, ws) >= min(end, we);
}

// The least distance of an aligned locus of [a, c) other than `skip` that lies elsewhere from [ws, we) on strand sw, KMX_ALIGN_NONE
// when there is none: the lanes stride over the loci, the wave min-reduces, every lane returns the result.
__device__ __forceinline__ uint32_t second_elsewhere(const uint8_t* dist, const uint32_t* start, const uint32_t* end, uint64_t a, uint64_t b, uint64_t c,
                                                     uint32_t lane, uint64_t skip, uint32_t sw, uint32_t ws, uint32_t we)
{
    uint32_t second = KMX_ALIGN_NONE;
    for (uint64_t l = a + lane; l < c; l += kFoldWave) {
        const uint32_t d = dist[l];
        if (d >= KMX_ALIGN_SKIPPED || l == skip) continue;
        if (elsewhere(l < b ? 0u : 1u, start[l], end[l], sw, ws, we)) second = min(second, d);
    }
    for (int off = kFoldWave / 2; off > 0; off >>= 1) second = min(second, uint32_t(__shfl_xor(second, off)));
    return second;
}

// the insert rule of a pair (kmx_pair_options, kmx_rescue_options); in this order, and behind `penalty` in PairIn, the kernel arguments
// of k_pair_fold load as they did when these were fields of PairIn (another order costs it 13 SGPRs: DESIGN.md 7l)
struct Insert {
    int64_t min_insert, max_insert;
    uint32_t orientation;
};

// Mate 1 on strand sx at [xs, xe), mate 2 on strand sy at [ys, ye): the template length when the two are concordant, else -1;
// *first: the upstream one is mate 1 (false when the strands do not fit the orientation)
__device__ __forceinline__ int64_t concordant_tlen(const Insert& I, uint32_t sx, uint32_t xs, uint32_t xe, uint32_t sy, uint32_t ys, uint32_t ye,
                                                   bool* first)
{
    *first = false;
    if ((sx == sy) != (I.orientation == KMX_PAIR_FF)) return -1;
    const bool f = sx == (I.orientation == KMX_PAIR_RF ? 1u : 0u);
    const int64_t us = f ? xs : ys, ue = f ? xe : ye, vs = f ? ys : xs, ve = f ? ye : xe;
    const int64_t t = ve - us;
    *first = f;
    return us <= vs && ue <= ve && t >= I.min_insert && t <= I.max_insert ? t : -1;
}

// One read into the LDS counters s_ctr[kmx::PL_*]: placed, on the reverse strand, ambiguous (a runner-up as near as the placement)
__device__ __forceinline__ void count_placement(unsigned int* s_ctr, bool placed, uint32_t strand, uint32_t second, uint32_t dist)
{
    if (!placed) return;
    atomicAdd(&s_ctr[kmx::PL_N_PLACED], 1u);
    if (strand == 1u) atomicAdd(&s_ctr[kmx::PL_N_REVERSE], 1u);
    if (second == dist) atomicAdd(&s_ctr[kmx::PL_N_AMBIGUOUS], 1u);
}

// ... and one pair into s_ctr[kmx::PR_*]: its class, and ambiguous (a concordant runner-up with the same score)
__device__ __forceinline__ void count_pair(unsigned int* s_ctr, uint32_t cls, uint32_t score, uint32_t second_score)
{
    atomicAdd(&s_ctr[cls == KMX_PAIR_CONCORDANT ? kmx::PR_N_CONCORDANT : cls == KMX_PAIR_DISCORDANT ? kmx::PR_N_DISCORDANT
                     : cls == KMX_PAIR_UNPLACED ? kmx::PR_N_UNPLACED : kmx::PR_N_SINGLE], 1u);
    if (cls == KMX_PAIR_CONCORDANT && second_score == score) atomicAdd(&s_ctr[kmx::PR_N_AMBIGUOUS], 1u);
}

} // namespace
