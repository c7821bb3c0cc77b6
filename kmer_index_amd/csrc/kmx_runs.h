// What the kernels behind the edit scripts share (kmx_script.hip, kmx_clip.hip, kmx_tags.hip, kmx_realign.hip): the BAM-style run word
// of a script, the runs of an entry, the packed-text letter fetch, and the affine scoring of a script's runs with the one rule for an
// entry that stays whole (KMX_CLIP_LOW).  Everything here has internal linkage: each source compiles its own.  Private to the library.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kmx_types.h"

namespace {

// a run is len << 4 | op, the op codes BAM's
enum { OP_M = 0, OP_I = 1, OP_D = 2, OP_S = 4, OP_EQ = 7, OP_X = 8, OP_NONE = 15 };
constexpr uint64_t kMaxRuns = 0x7FFFFFFFull;                   // the runs of one entry that are looked at (its count, + 2, is 32-bit)

__device__ __forceinline__ uint32_t run_op(uint32_t v) { return v & 15u; }
__device__ __forceinline__ uint32_t run_len(uint32_t v) { return v >> 4; }
__device__ __forceinline__ uint32_t make_run(uint32_t len, uint32_t op) { return (len << 4) | op; }

// the runs [*a, *b) of entry e, inside cigar[n_ops] whatever the offsets hold
__device__ __forceinline__ void runs_of(const uint64_t* cig_off, uint64_t n_ops, uint64_t e, uint64_t* a, uint64_t* b)
{
    *a = min(cig_off[e], n_ops);
    *b = min(min(max(cig_off[e + 1], *a), n_ops), *a + kMaxRuns);
}

__device__ __forceinline__ uint16_t sat16(uint64_t v) { return uint16_t(min(v, uint64_t(0xFFFF))); }
__device__ __forceinline__ int32_t sat32(int64_t v) { return int32_t(max(int64_t(INT32_MIN), min(int64_t(INT32_MAX), v))); }

// letter `at` of the text packed at w bits per letter (w = 2, 4 or 8: a letter never straddles a word)
__device__ __forceinline__ uint32_t text_letter(const uint64_t* text, uint32_t w, uint64_t at)
{
    const uint32_t per = 64 / w;
    return uint32_t((text[at / per] >> ((at % per) * w)) & ((uint64_t(1) << w) - 1));
}

// The affine scoring of kmx_scripts_clip and kmx_scripts_realign: a = match, b = mismatch, o = gap_open, x = gap_extend,
// p = clip_penalty.  The fields are as narrow as the options allow (a, b, o, x <= 255, p <= 65535), which is what the band of the
// realignment computes in; a sum over runs is made in int64, where a run of 2^28 letters cannot overflow it.
struct Scoring {
    int a, b, o, x, p, min_score;
};

// what run v adds to the score of its script; a run that is none of = X I D adds nothing and sets *bad
__device__ __forceinline__ int64_t run_score(const Scoring& G, uint32_t v, bool* bad)
{
    const uint32_t op = run_op(v);
    const int64_t len = int64_t(run_len(v));
    if (op == OP_EQ) return len * G.a;
    if (op == OP_X) return -(len * G.b);
    if (op == OP_I || op == OP_D) return -(G.o + len * G.x);
    *bad = true;
    return 0;
}

// the per-entry values of a clips handle as a kernel writes them
struct ClipOut {
    int32_t* score;                // [n_sel]
    uint16_t* sl;
    uint16_t* sr;
    uint16_t* tl;
    uint16_t* tr;
    uint16_t* nm;
    uint8_t* cflags;
    uint32_t* cnt;                 // the runs of the entry, for the scan that gives cig_off
};

// Entry e stays whole (KMX_CLIP_LOW): nothing is clipped, its runs are the R runs of its script at `runs`, its score their affine
// score and nm their X + I + D lengths; a script with a run that is none of = X I D gets score 0 and nm 0.  out != nullptr: the runs
// are copied there as well.
__device__ __forceinline__ void whole_entry(const Scoring& G, const uint32_t* __restrict__ runs, uint64_t R, uint32_t* __restrict__ out, const ClipOut& O,
                                            uint64_t e)
{
    int64_t W = 0;
    uint64_t nm = 0;
    bool bad = false;
    for (uint64_t k = 0; k < R; ++k) {
        const uint32_t v = runs[k];
        W += run_score(G, v, &bad);
        if (run_op(v) != OP_EQ) nm += run_len(v);
        if (out) out[k] = v;
    }
    O.score[e] = bad ? 0 : sat32(W);
    O.sl[e] = O.sr[e] = O.tl[e] = O.tr[e] = 0;
    O.nm[e] = bad ? uint16_t(0) : sat16(nm);
    O.cflags[e] = uint8_t(KMX_CLIP_LOW);
    O.cnt[e] = uint32_t(R);
}

} // namespace
